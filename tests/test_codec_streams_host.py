"""Census of the hand-assembled decoder cases (codec_streams.py): walks the exact lists test_gpu_codec_streams.py feeds to the GPU and
asserts that they hold what they claim -- every copy kind and literal length form, the whole overlap matrix, every header form at every
phase of the parse window, destinations on every byte phase, every PFOR width at every header position, a raw mini-block at every
position, every tail length and byte count -- and that both CPU oracles refuse every malformed block.  No device.  (That both oracles
READ every well-formed block as the assembler does is asserted when a column is built: codec_streams.both_oracles_*.)"""
import numpy as np
import pytest

import codec_streams as cs
from oracle import oracle_np


def snappy_elements(col):
    return [e for b in col.blocks for c in b.chunks if c.kind == "snappy" for e in c.elements]


def test_assembler_known_answers(oracle):
    # the streams of test_oracle_snappy.py's known answers, rebuilt by the assembler byte for byte
    raw, exp = cs.payload([cs.literal(b"abc"), cs.copy(4, 3, 1), cs.copy(4, 7, 2)])
    assert raw == bytes([11, 0x08]) + b"abc" + bytes([0x01, 0x03, 0x0E, 0x07, 0x00]) and exp == b"abcabcaabca"
    raw, exp = cs.payload([cs.literal(b"wxyz"), cs.copy(4, 4, 3)])
    assert raw == bytes([8, 0x0C]) + b"wxyz" + bytes([(3 << 2) | 3, 4, 0, 0, 0]) and exp == b"wxyzwxyz"
    assert cs.literal(bytes(61)).encode()[:2] == bytes([60 << 2, 60]) and cs.literal(bytes(5), 4).encode()[:5] == bytes([63 << 2, 4, 0, 0, 0])
    assert cs.varint(300) == bytes([0xAC, 0x02]) and cs.varint(5, 3) == bytes([0x85, 0x80, 0x00]) and cs.varint(0, 1) == b"\0"
    data = b"hello hello hello hello"
    blk = cs.block([("stored", data)])
    assert blk.raw == b"snappy\x00" + bytes([0, 0, len(data)]) + oracle_np.crc32c_masked(data).to_bytes(4, "big") + data
    # test_oracle_pfor.py's: the tail packing (byte 0 of a tail word is the low byte of the big-endian word), a width-3 stream, raw
    be = lambda ws: b"".join(int(w & 0xFFFFFFFF).to_bytes(4, "big") for w in ws)
    raw, exp = cs.pfor_block([], [(5, 1), (295, 2), (0, 1)])
    assert raw == be([3, 0x80822785]) + bytes(8) and exp.tolist() == [5, 300, 300]
    raw, exp = cs.pfor_block([(3, [5] * 32)], [])
    stream = sum(5 << (3 * i) for i in range(32))
    assert raw == be([32, 3] + [(stream >> (32 * k)) & 0xFFFFFFFF for k in range(3)]) + bytes(8) and exp.tolist() == (np.arange(1, 33) * 5).tolist()
    raw, exp = cs.pfor_block([(32, [7] + [6] * 31)], [])
    assert raw == be([32, 32, 7] + [6] * 31) + bytes(8)
    raw, exp = cs.pfor_block([(1, [0] + [1] * 31)] + [(1, [1] * 32)] * 3, [])
    assert raw == be([128, 0x01010101, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]) + bytes(8) and exp.tolist() == list(range(128))
    # unusual but valid: a declared width above what the deltas need, a padded tail value
    raw, exp = cs.pfor_block([(7, [1] * 32)], [(3, 4)])
    assert oracle.pfor_decode_block(raw).tolist() == exp.tolist() == list(range(1, 33)) + [35] == oracle_np.pfor_decode_block(raw).tolist()


def test_snappy_forms_hold_every_kind_and_length_form(oracle):
    f = cs.snappy_forms()
    el = snappy_elements(f["decodes"])
    assert {e.form for e in el} == set(cs.FORMS)
    lits = {(len(e.data), e.nb) for e in el if isinstance(e, cs.Lit)}
    for n in cs.FORM_LITERALS:
        assert (n, cs.minimal_length_bytes(n)) in lits
    for n in cs.FORM_LONGER:
        assert {nb for m, nb in lits if m == n} >= set(range(cs.minimal_length_bytes(n) + 1, 5))
    copies = {(e.kind, e.length, e.offset) for e in el if isinstance(e, cs.Cpy)}
    assert copies >= {(1, ln, off) for ln in range(4, 12) for off in cs.KIND1_OFFSETS}
    assert copies >= {(k, ln, off) for k in (2, 3) for ln in cs.FAR_LENGTHS for off in cs.FAR_OFFSETS}
    # offset 32767: only a copy of one byte can have 32767 bytes in front of it and still end inside a chunk; the longer ones take
    # the whole chunk in front of them
    assert copies >= {(k, 1, 32767) for k in (2, 3)} | {(k, ln, cs.CHUNK_MAX - ln) for k in (2, 3) for ln in cs.FAR_LENGTHS}
    # the whole-chunk literal in every form that holds it (the GPU refuses these: they do not fit its LDS windows), and the largest that fits
    whole = [snappy_elements(c) for c in f["whole_chunk_literals"]]
    assert [(len(e[0].data), e[0].nb) for e in whole] == [(cs.CHUNK_MAX, nb) for nb in (2, 3, 4)]
    assert not any(cs.column_fits_lds(c) for c in f["whole_chunk_literals"])
    for c, nb in zip(f["largest_literals"], (2, 3, 4)):
        (e,) = snappy_elements(c)
        assert e.nb == nb and cs.column_fits_lds(c) and cs.snappy_lds_need(len(c.blocks[0].raw) + 1, len(e.data) + 1) > cs.SNAPPY_LDS_BUDGET
    assert cs.column_fits_lds(f["decodes"])


def test_overlap_matrix_is_complete(oracle):
    col = cs.snappy_overlap_matrix()
    el = snappy_elements(col)
    pairs = {k: {(e.offset, e.length) for e in el if isinstance(e, cs.Cpy) and e.kind == k} for k in (1, 2, 3)}
    every = {(off, ln) for off in range(1, 64) for ln in range(1, 65)}
    assert pairs[2] == every and len(every) == 63 * 64
    assert pairs[1] == {(off, ln) for off, ln in every if 4 <= ln <= 11}
    assert len(pairs[3]) >= len(every) // cs.KIND3_SAMPLE - 1 and any(off < ln for off, ln in pairs[3]) and any(off >= ln for off, ln in pairs[3])
    # every copy stands behind a literal of 1..7 bytes, and the window phase of the copies varies with them
    phases = set()
    for b in col.blocks:
        assert len(b.chunks) == 1 and len(b.expected) <= cs.CHUNK_MAX
        seq = cs.window_phases(b.chunks[0].elements)
        for (prev, _), (e, ph) in zip(seq, seq[1:]):
            if isinstance(e, cs.Cpy):
                assert isinstance(prev, cs.Lit) and (1 <= len(prev.data) <= 7 or len(prev.data) == 64)
                phases.add(ph)
    assert len(phases) >= 60
    assert len(col.blocks) > 1 and cs.column_fits_lds(col)


def test_every_header_form_at_every_window_phase(oracle):
    col = cs.snappy_window_phases()
    seen = {f: set() for f in cs.FORMS}
    ends = set()
    for b in col.blocks:
        for c in b.chunks:
            for e, ph in cs.window_phases(c.elements):
                seen[e.form].add(ph)
                if isinstance(e, cs.Lit):
                    ends.add(ph + len(e.encode()))
    # an element takes at least two bytes, so nothing ever starts at phase 1 of a window
    for f in cs.FORMS:
        assert seen[f] >= set(cs.PHASES), (f, sorted(set(cs.PHASES) - seen[f]))
        assert 1 not in seen[f]
    assert cs.PHASES == [0] + list(range(2, 64))
    assert {63, 64} <= ends                                   # literals that end exactly on the window edge, and one byte before
    assert cs.column_fits_lds(col)


def test_framing_cases_and_destination_phases(oracle):
    dst_phase, aligned_ulen, block_phase = set(), set(), set()
    for _, width in cs.FRAMING_WIDTHS:
        col = cs.snappy_framing(width)
        assert cs.column_fits_lds(col)
        rows = col.block_rows
        assert any(r == 0 and 0 < i < len(rows) - 1 and rows[i - 1] and rows[i + 1] for i, r in enumerate(rows))          # an empty block between full ones
        assert any(len(b.raw) == 7 for b in col.blocks)
        sizes = [[len(c.expected) for c in b.chunks] for b in col.blocks]
        assert any(s[1:] == [cs.CHUNK_MAX, 7] and s[0] in (100, 101) for s in sizes)
        three = [b for b in col.blocks if len(b.chunks) == 3 and len(b.chunks[1].expected) == cs.CHUNK_MAX][0]
        assert [c.kind for c in three.chunks] == ["stored", "snappy", "stored"]
        assert any(c.kind == "stored" and not c.expected for b in col.blocks for c in b.chunks)                              # zero-length chunks
        assert any(c.kind == "snappy" and not c.expected and c.raw == b"\0" for b in col.blocks for c in b.chunks)
        assert {c.preamble_len for b in col.blocks for c in b.chunks if c.kind == "snappy"} >= {1, 2, 3, 4, 5}             # padded preambles
        assert any(len(b.chunks) > 1 and len(b.chunks[0].expected) % 2 for b in col.blocks)                                 # second chunk at an odd `done`
        assert any(0 < len(c.expected) < cs.CHUNK_MAX for b in col.blocks for c in b.chunks[:-1])                           # short chunks that are not the last
        mine = {a % 4 for a, n in col.chunk_destinations() if n}
        if width == 1:
            assert mine == {0, 1, 2, 3}
        dst_phase |= mine
        aligned_ulen |= {n % 4 for a, n in col.chunk_destinations() if a % 4 == 0 and n}
        block_phase |= {int(o) % 4 for o in col.offsets[:-1]}
    assert dst_phase == {0, 1, 2, 3} and aligned_ulen == {0, 1, 2, 3} and block_phase == {0, 1, 2, 3}
    # across all snappy columns the GPU decodes: the same (the existing suite only ever had dword-aligned destinations)
    for name, col in cs.snappy_columns().items():
        if cs.column_fits_lds(col):
            block_phase |= {int(o) % 4 for o in col.offsets[:-1]}
    assert block_phase == {0, 1, 2, 3}


def test_lds_edge_sizes(oracle):
    # recomputed from snappy_index's formula, not taken on trust: in_cap = (stored + 3 + 8 + 15) & ~15, out_cap = (max(chunk, 16) + 15) & ~15
    n, b = cs.largest_stored_chunk(), cs.largest_block_beside_full_chunk()
    assert ((14 + n + 26) & ~15) + ((n + 15) & ~15) <= 63 * 1024 < ((14 + n + 1 + 26) & ~15) + ((n + 1 + 15) & ~15)
    assert ((b + 26) & ~15) + 32768 <= 63 * 1024 < ((b + 1 + 26) & ~15) + 32768
    assert (n, b) == (32240, 31733)
    e = cs.snappy_lds_edge()
    assert [len(e[k].blocks[0].raw) for k in ("stored_fits", "stored_over", "full_fits", "full_over")] == [14 + n, 15 + n, b, b + 1]
    assert [cs.column_fits_lds(e[k]) for k in ("stored_fits", "stored_over", "full_fits", "full_over")] == [True, False, True, False]
    assert all(len(e[k].blocks[0].expected) == cs.CHUNK_MAX and e[k].blocks[0].chunks[0].kind == "snappy" for k in ("full_fits", "full_over"))


def test_pfor_widths_at_every_header_position(oracle):
    col = cs.pfor_widths()
    assert all(r == 1024 for r in col.block_rows) and len(col.block_rows) <= 10
    exact = {(p, w) for p, w, bits in col.meta if w == bits}
    assert exact >= {(p, w) for p in range(4) for w in range(33)}
    wider = {(p, bits, w - bits) for p, w, bits in col.meta if w > bits}
    assert {(p, bits) for p, bits, _ in wider} >= {(p, bits) for p in range(4) for bits in range(31)}
    assert {x for _, _, x in wider} == {1, 2, 3, 4, 5} and all(w <= 31 for p, w, bits in col.meta if w > bits)
    for g in range(0, 4 * 33, 4):                             # neighbours at other widths
        assert len({w for _, w, _ in col.meta[g:g + 4]}) == 4
    left = cs.pfor_leftover_widths()
    assert {ws[0] for ws in left.meta} == set(range(33)) and {len(ws) for ws in left.meta} == {1, 2, 3}
    assert all(r % 128 in (32, 64, 96) for r in left.block_rows)
    assert {w for ws in left.meta for w in ws[1:]} == {0, 1, 31, 32}


def test_pfor_raw_positions(oracle):
    col = cs.pfor_raw_positions()
    assert all(r == 1024 for r in col.block_rows)
    assert col.meta[:32] == [(p,) for p in range(32)]
    assert (7, 8) in col.meta and (15, 16) in col.meta and tuple(range(32)) in col.meta
    v = col.values.view(np.uint32)
    assert (v == cs.INT_MIN).any() and (v == cs.INT_MAX).any()
    # deltas that wrap: a packed value below its predecessor
    packed_after_raw = col.values[32 * 1:32 * 2].astype(np.int64)           # block 0: raw at 0, packed behind it
    assert (np.diff(np.concatenate([[int(col.values[31])], packed_after_raw])) < 0).any()
    zero = col.block_rows.index(1024) + 35                                   # raw, then every other mini-block of width 0: one value repeated
    blk = col.values[1024 * zero:1024 * (zero + 1)]
    assert (blk[32:] == blk[31]).all() and col.meta[zero] == (0,)


def test_pfor_tails_and_leftovers(oracle):
    col = cs.pfor_leftovers_and_tails()
    assert {(k, t) for k, t, _, _ in col.meta} == {(k, t) for k in cs.LEFTOVER_K for t in range(32)}
    assert {len(left) for _, _, left, _ in col.meta} == {0, 1, 2, 3}
    assert {w for _, _, left, _ in col.meta for w in left} == {0, 1, 31, 32}
    for t in range(1, 32):
        assert {nb for _, tt, _, tail in col.meta if tt == t for _, nb in tail} == set(range(1, min(t, 5) + 1)) or t < 5
    assert {nb for _, _, _, tail in col.meta for _, nb in tail} == {1, 2, 3, 4, 5}
    assert any(d >> 31 for _, _, _, tail in col.meta for d, nb in tail)                                          # wrapping (negative) deltas
    assert any(nb > 1 and d < 1 << (7 * (nb - 1)) for _, _, _, tail in col.meta for d, nb in tail)               # a padded value
    assert any(r > 1024 for r in col.block_rows) and 0 in col.block_rows
    tails = cs.pfor_tile_tails()
    assert [c.meta for c in tails] == cs.TILE_TAIL_ROWS and all(c.block_rows == [1024, r] and 1 <= r <= 1023 for c, r in zip(tails, cs.TILE_TAIL_ROWS))
    assert {r % 32 for r in cs.TILE_TAIL_ROWS} >= {1, 5, 31} and any(r % 32 >= 5 and r >= 32 for r in cs.TILE_TAIL_ROWS)
    carry = cs.pfor_chunk_carry()
    assert carry.block_rows == [2048, 2048, 4096 + 77, 4096 + 77] and [m[1] for m in carry.meta] == ["raw last", "raw first"] * 2


def test_fused_predicates_name_rows_15_16_1023_and_the_last(oracle):
    from conftest import EQ
    col = cs.pfor_tile_tails()[-1]
    sels = cs.pfor_fused_predicates(col)
    eqs = [s[0][2] for s in sels if s[0][1] == EQ]
    assert eqs == [float(col.values[r]) for r in (15, 16, 1023, col.values.size - 1)] and len(sels[-1]) == 2


def test_both_oracles_refuse_every_malformed_block(oracle):
    snappy = cs.snappy_malformed()
    assert {n for n, _, _, _ in snappy} >= {"copy offset 0", "copy offset = written + 1", "copy ends 1 past the preamble", "literal ends 1 past the payload",
                                             "literal ends 1 past the preamble", "kind-2 copy header cut off", "output 1 byte short of the preamble",
                                             "five continuation bytes in the preamble", "preamble 32769", "flag 2", "payload length 1 past the block"}
    for name, raw, where, why in snappy:
        assert raw[:7] == cs.STREAM_HEADER and where in ("create", "use")
        with pytest.raises(oracle.OracleError):
            oracle.snappy_block_decode(raw)
        with pytest.raises(AssertionError):
            oracle_np.snappy_block_decode(raw)
        if where == "use":                                    # the chunk headers and the preamble are sound: only an element check can refuse it
            n = int.from_bytes(raw[8:10], "big")
            assert raw[7] == 1 and 14 + n == len(raw) and oracle.lib().imm3o_snappy_block_length(np.frombuffer(raw, np.uint8).ctypes.data, len(raw)) % 16 != 0
    pfor = cs.pfor_malformed()
    names = [n for n, _, _, _ in pfor]
    assert sum(n.startswith("width 33 at group position") for n in names) == 4 and "width 33 in a leftover" in names
    assert {"group widths end one word past the block", "tail value of six bytes", "tail runs one byte past the block"} <= set(names)
    for name, raw, rows, why in pfor:
        assert int.from_bytes(raw[:4], "big") == rows and len(raw) % 4 == 0
        with pytest.raises(oracle.OracleError):
            oracle.pfor_decode_block(raw)
        with pytest.raises(AssertionError):
            oracle_np.pfor_decode_block(raw)
