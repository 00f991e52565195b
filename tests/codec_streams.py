"""Hand-assembled snappy and PFOR_INT blocks for the block decoders (csrc/imm3_snappy.hip, csrc/imm3_codec.hip), and the case lists
test_gpu_codec_streams.py drives them with (test_codec_streams_host.py walks the same lists and asserts that they are not hollow).
Pure Python / numpy and the CPU oracles: nothing here touches a device.

An encoder writes only the streams it likes; an assembler writes any stream the format allows -- every copy kind, every literal
length form, any declared PFOR width, any variable-byte length -- and a few it does not allow.  What a block must decode to is
the assembler's own reading of the element list it was given (interpret(), pfor_block()'s wrapping sums), never the code under
test; and every assembled block is decoded by BOTH CPU restatements (oracle_c, oracle_np) when its column is built, so a GPU test
can never compare against bytes the two references do not share."""
import functools

import numpy as np

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, PFOR_INT, SNAPPY_INT, SNAPPY_STRING, SNAPPY_TINYINT, RawColumn
from oracle import oracle_c, oracle_np

CHUNK_MAX = 32768                       # SnappyOutputStream never puts more input bytes into a chunk; k_snappy_sizes refuses more
STREAM_HEADER = b"snappy\x00"


def _rand(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


# =====================================================================================================================
# snappy: elements
# =====================================================================================================================
class Lit:
    """literal: `nb` length bytes behind the tag (0: the length sits in the tag)"""

    def __init__(self, data, nb):
        self.data, self.nb = data, nb

    form = property(lambda self: "lit%d" % self.nb)
    header = property(lambda self: 1 + self.nb)

    def encode(self):
        n = len(self.data) - 1
        head = bytes([n << 2]) if self.nb == 0 else bytes([(59 + self.nb) << 2]) + n.to_bytes(self.nb, "little")
        return head + self.data


class Cpy:
    def __init__(self, length, offset, kind):
        self.length, self.offset, self.kind = length, offset, kind

    form = property(lambda self: "copy%d" % self.kind)
    header = property(lambda self: {1: 2, 2: 3, 3: 5}[self.kind])

    def encode(self):
        if self.kind == 1:
            return bytes([1 | ((self.length - 4) << 2) | ((self.offset >> 8) << 5), self.offset & 255])
        return bytes([self.kind | ((self.length - 1) << 2)]) + self.offset.to_bytes(2 if self.kind == 2 else 4, "little")


class Raw:
    """bytes the format does not allow (malformed cases only), and what a decoder without the check under test would make of them"""

    def __init__(self, data, produces=b""):
        self.data, self.produces = bytes(data), bytes(produces)

    form = "raw"

    def encode(self):
        return self.data


FORMS = ["lit0", "lit1", "lit2", "lit3", "lit4", "copy1", "copy2", "copy3"]


def minimal_length_bytes(n):
    return 0 if n <= 60 else 1 if n <= 1 << 8 else 2 if n <= 1 << 16 else 3 if n <= 1 << 24 else 4


def literal(data, length_bytes=None):
    """minimal form, or a forced number of length bytes (0 only for lengths <= 60; never fewer than the length needs)"""
    data = bytes(data)
    assert 1 <= len(data) <= 1 << 32
    nb = minimal_length_bytes(len(data)) if length_bytes is None else length_bytes
    assert 0 <= nb <= 4 and (nb > 0 or len(data) <= 60) and (nb == 0 or len(data) - 1 < 1 << (8 * nb))
    return Lit(data, nb)


def copy(length, offset, kind):
    assert kind in (1, 2, 3) and offset >= 1
    if kind == 1:
        assert 4 <= length <= 11 and offset < 2048
    else:
        assert 1 <= length <= 64 and offset < (1 << 16 if kind == 2 else 1 << 32)
    return Cpy(length, offset, kind)


def interpret(elements):
    """what the element list says, byte by byte (an overlapping copy reads bytes it has just written)"""
    out = bytearray()
    for e in elements:
        if isinstance(e, Lit):
            out += e.data
        elif isinstance(e, Raw):
            out += e.produces
        else:
            assert 0 < e.offset <= len(out), (e.offset, len(out))
            for _ in range(e.length):
                out.append(out[-e.offset])
    return bytes(out)


def varint(n, n_bytes=None):
    """minimal, or padded with zero groups to n_bytes (<= 5)"""
    out = []
    while n >= 128:
        out.append((n & 127) | 128)
        n >>= 7
    out.append(n)
    if n_bytes is not None:
        assert len(out) <= n_bytes <= 5
        while len(out) < n_bytes:
            out[-1] |= 128
            out.append(0)
    return bytes(out)


def payload(elements, preamble_bytes=None, declared=None):
    """(raw Snappy payload, expected output); `declared` overrides the preamble's length (malformed cases)"""
    expected = interpret(elements)
    pre = varint(len(expected) if declared is None else declared, preamble_bytes)
    return pre + b"".join(e.encode() for e in elements), expected


# =====================================================================================================================
# snappy: framing
# =====================================================================================================================
class Chunk:
    """one chunk of an assembled block: kind "stored" | "snappy", its elements (snappy), where its payload lies in the block"""

    def __init__(self, kind, elements, payload_pos, preamble_len, raw, expected):
        self.kind, self.elements, self.payload_pos, self.preamble_len, self.raw, self.expected = kind, elements, payload_pos, preamble_len, raw, expected


class Block:
    def __init__(self, raw, expected, chunks):
        self.raw, self.expected, self.chunks = raw, expected, chunks


def block(chunks, flag=None, length_delta=0):
    """chunks: ("stored", bytes) | ("snappy", elements) | ("snappy", elements, preamble_bytes) | ("snappy", elements, preamble_bytes,
    declared).  Header: flag, payload length big-endian, masked CRC-32C (oracle_np's) of the chunk's expected bytes.
    flag / length_delta bend the LAST chunk's header (malformed cases)."""
    raw, expected, made = bytearray(STREAM_HEADER), bytearray(), []
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        if c[0] == "stored":
            body, exp, elements, pre = bytes(c[1]), bytes(c[1]), None, 0
        else:
            assert c[0] == "snappy"
            elements = list(c[1])
            nb = c[2] if len(c) > 2 else None
            body, exp = payload(elements, nb, c[3] if len(c) > 3 else None)
            pre = len(body) - sum(len(e.encode()) for e in elements)
        f = {"stored": 0, "snappy": 1}[c[0]] if flag is None or not last else flag
        raw += bytes([f]) + (len(body) + (length_delta if last else 0)).to_bytes(2, "big") + oracle_np.crc32c_masked(exp).to_bytes(4, "big")
        made.append(Chunk(c[0], elements, len(raw), pre, body, exp))
        raw += body
        expected += exp
    return Block(bytes(raw), bytes(expected), made)


def both_oracles_snappy(blk):
    oracle_c.build()
    a, b = oracle_c.snappy_block_decode(blk.raw), oracle_np.snappy_block_decode(blk.raw)
    assert a == blk.expected, "the C oracle reads the assembled block differently"
    assert b == blk.expected, "the numpy oracle reads the assembled block differently"


class AssembledSnappyColumn:
    """SnappyColumn's interface over a list of assembled blocks; the dense view is the concatenated expected bytes."""

    def __init__(self, dense_codec, width, blocks, verify=True):
        self.codec = {DENSE_INT: SNAPPY_INT, DENSE_TINYINT: SNAPPY_TINYINT, DENSE_STRING: SNAPPY_STRING}[dense_codec]
        self.width, self.blocks = width, list(blocks)
        for b in self.blocks:
            assert len(b.expected) % width == 0
            if verify:
                both_oracles_snappy(b)
        self.block_rows = [len(b.expected) // width for b in self.blocks]
        dense = np.frombuffer(b"".join(b.expected for b in self.blocks), dtype=np.uint8)
        self.values = dense.view(np.int8) if dense_codec == DENSE_TINYINT else dense.view("<i4") if dense_codec == DENSE_INT else dense.reshape(-1, width)
        self._dense = RawColumn(dense_codec, width, self.values, self.block_rows)
        self.dat = np.frombuffer(b"".join(b.raw for b in self.blocks), dtype=np.uint8).copy()
        self.offsets = np.concatenate([[0], np.cumsum([len(b.raw) for b in self.blocks])]).astype(np.int32)

    def ocol(self):
        return self._dense.ocol()

    def npcol(self):
        return self._dense.npcol()

    def native(self):
        return (self.codec, self.width, self.dat, self.dat.size, self.offsets)

    def chunk_destinations(self):
        """(byte address in the dense column, uncompressed length) of every chunk: where k_snappy_decode stores it"""
        out, base = [], 0
        for b in self.blocks:
            done = 0
            for c in b.chunks:
                out.append((base + done, len(c.expected)))
                done += len(c.expected)
            base += len(b.expected)
        return out


def tiny(blocks):
    return AssembledSnappyColumn(DENSE_TINYINT, 1, blocks)


# ---- the decoder's LDS windows (csrc/imm3_api.cpp: snappy_index) -------------------------------------------------------------------
SNAPPY_LDS_BUDGET = 63 * 1024           # kSnappyLdsBudget: 64 KiB less the 1 KiB CRC table


def snappy_lds_need(biggest_block, biggest_chunk):
    """in_cap + out_cap as snappy_index sizes them: the staged block (+ 3 bytes of skew, 8 of read slack) and one chunk, each
    rounded up to 16 bytes; a segment whose sum exceeds SNAPPY_LDS_BUDGET is refused with IMM3_ERR_LAYOUT"""
    in_cap = (biggest_block + 3 + 8 + 15) & ~15
    out_cap = (max(biggest_chunk, 16) + 15) & ~15
    return in_cap + out_cap


def column_fits_lds(col):
    return snappy_lds_need(max([len(b.raw) for b in col.blocks] or [0]), max([len(c.expected) for b in col.blocks for c in b.chunks] or [0])) <= SNAPPY_LDS_BUDGET


def largest_stored_chunk():
    """the largest n for which a block of one stored chunk of n bytes (7 + 7 + n stored bytes) fits"""
    n = 0
    while snappy_lds_need(14 + n + 1, n + 1) <= SNAPPY_LDS_BUDGET:
        n += 1
    return n


def largest_block_beside_full_chunk():
    """the largest stored block that fits beside a chunk of CHUNK_MAX output bytes (the largest out_cap)"""
    n = 0
    while snappy_lds_need(n + 1, CHUNK_MAX) <= SNAPPY_LDS_BUDGET:
        n += 1
    return n


def grow(rng, elements, op, target, kind=2):
    """non-overlapping copies of up to 64 bytes from random earlier positions until the chunk holds `target` bytes"""
    while op < target:
        ln = min(64, target - op)
        elements.append(copy(ln, int(rng.integers(ln, op + 1)), kind))
        op += ln
    return op


def fit_elements(rng, out_bytes, enc_bytes):
    """elements that decode to exactly out_bytes bytes from exactly enc_bytes encoded bytes (enc_bytes < out_bytes): one random
    literal, 64-byte copies, and literals whose length forms are as wide as the bytes left over need"""
    n_copies = -(-(out_bytes - enc_bytes + 3) // 61)                # a copy turns 3 bytes into 64
    lit_bytes = out_bytes - 64 * n_copies
    slack = enc_bytes - (3 + lit_bytes + 3 * n_copies)              # the first literal has 2 length bytes
    assert 0 <= slack and lit_bytes >= 300
    extra = [4] * (slack // 5) + ([slack % 5 - 1] if slack % 5 else [])   # a literal with nb length bytes costs 1 + nb
    first = lit_bytes - len(extra)
    elements = [literal(_rand(rng, first), 2)]
    grow(rng, elements, first, first + 64 * n_copies)
    elements += [literal(_rand(rng, 1), nb) for nb in extra]
    enc = sum(len(e.encode()) for e in elements)
    assert enc == enc_bytes and len(interpret(elements)) == out_bytes, (enc, enc_bytes)
    return elements


def window_phases(elements):
    """[(element, phase)]: the position of every element's first byte in k_snappy_decode's 64-byte parse window -- a window starts
    at an element start, and the next one starts at the first element start at or after 64 bytes"""
    out, pos, start = [], 0, 0
    for e in elements:
        if pos - start >= 64:
            start = pos
        out.append((e, pos - start))
        pos += len(e.encode())
    return out


# =====================================================================================================================
# snappy: the case lists
# =====================================================================================================================
FORM_LITERALS = [1, 59, 60, 61, 64, 65, 255, 256, 257, 4095]        # + CHUNK_MAX: a block of its own (see snappy_forms)
FORM_LONGER = [5, 61]                                                 # + CHUNK_MAX; each with every longer length form
KIND1_OFFSETS = [1, 255, 256, 2047]
FAR_LENGTHS = [1, 4, 63, 64]
FAR_OFFSETS = [1, 2047, 2048]                                         # + 32767 (far_copy_chunks)


def _far_offset(length):
    """an offset of 32767 needs 32767 bytes in front of the copy, and a chunk ends at 32768: only length 1 fits.  The longer
    copies take the largest offset the format allows them, the whole chunk in front of them."""
    return CHUNK_MAX - length


@functools.lru_cache(maxsize=None)
def snappy_forms():
    """{"decodes": column, "whole_chunk_literals": [column per length form], "largest_literals": column}"""
    rng = np.random.default_rng(20261019)
    el = [literal(_rand(rng, n)) for n in FORM_LITERALS]
    for n in FORM_LONGER:
        el += [literal(_rand(rng, n), nb) for nb in range(minimal_length_bytes(n) + 1, 5)]
    blocks = [block([("snappy", el)])]
    # kind 1: every length at four offsets, a random literal between the copies so that a wrong source position shows
    el = [literal(_rand(rng, 2047))]
    for off in KIND1_OFFSETS:
        for ln in range(4, 12):
            el += [copy(ln, off, 1), literal(_rand(rng, 3))]
    blocks.append(block([("snappy", el)]))
    el = [literal(_rand(rng, 2048))]
    for kind in (2, 3):
        for off in FAR_OFFSETS:
            for ln in FAR_LENGTHS:
                el += [copy(ln, off, kind), literal(_rand(rng, 3))]
    blocks.append(block([("snappy", el)]))
    for kind in (2, 3):                                               # the far copies: a chunk of CHUNK_MAX bytes each
        for ln in FAR_LENGTHS:
            el = [literal(_rand(rng, 2048))]
            op = grow(rng, el, 2048, CHUNK_MAX - ln)
            el.append(copy(ln, _far_offset(ln), kind))
            assert op == _far_offset(ln)
            blocks.append(block([("snappy", el)]))
    # a literal of a whole chunk, in every length form that holds it: the oracles read it; the GPU decoder's LDS windows cannot hold a
    # chunk of 32768 bytes beside 32768 + 20 stored ones (snappy_lds_need), so there the segment is refused
    whole = [tiny([block([("snappy", [literal(_rand(rng, CHUNK_MAX), nb)])])]) for nb in (2, 3, 4)]
    # ... and the largest literal that does fit, in the same forms
    fits = []
    for nb in (2, 3, 4):
        n = CHUNK_MAX
        while snappy_lds_need(14 + 3 + 1 + nb + n, n) > SNAPPY_LDS_BUDGET:
            n -= 1
        fits.append(block([("snappy", [literal(_rand(rng, n), nb)])]))
    return {"decodes": tiny(blocks), "whole_chunk_literals": whole, "largest_literals": [tiny([b]) for b in fits]}


KIND3_SAMPLE = 5                                                      # every 5th (offset, length) pair also as a kind-3 copy


@functools.lru_cache(maxsize=None)
def snappy_overlap_matrix():
    """every offset 1..63 x length 1..64 as a kind-2 copy (kind 1 too where it can say the length, kind 3 on a sample), random
    literals of 1..7 bytes in between; one chunk per block"""
    rng = np.random.default_rng(6364)
    blocks, el, op = [], [literal(_rand(rng, 64))], 64
    for off in range(1, 64):
        for ln in range(1, 65):
            kinds = [2] + ([1] if 4 <= ln <= 11 else []) + ([3] if (off * 64 + ln) % KIND3_SAMPLE == 0 else [])
            if op + len(kinds) * (7 + ln) > CHUNK_MAX:
                blocks.append(block([("snappy", el)]))
                el, op = [literal(_rand(rng, 64))], 64
            for kind in kinds:
                n = int(rng.integers(1, 8))
                el += [literal(_rand(rng, n)), copy(ln, off, kind)]
                op += n + ln
    blocks.append(block([("snappy", el)]))
    return tiny(blocks)


def _prefix_to(rng, phase):
    """minimal literals that take exactly `phase` bytes of the window (an element takes at least 2 bytes: phase 1 does not exist);
    phase 0: one literal that fills the window, so that the element under test opens the next one"""
    assert phase != 1
    if phase == 0:
        return [literal(_rand(rng, 70))]
    if phase <= 61:
        return [literal(_rand(rng, phase - 1))]
    if phase == 62:
        return [literal(_rand(rng, 30)), literal(_rand(rng, 30))]
    return [literal(_rand(rng, 61))]


PHASES = [p for p in range(64) if p != 1]


@functools.lru_cache(maxsize=None)
def snappy_window_phases():
    """every element header form with its first byte at every phase of the parse window; one block per form, one chunk per phase"""
    rng = np.random.default_rng(64)
    blocks = []
    for form in FORMS:
        chunks = []
        for phase in PHASES:
            el = _prefix_to(rng, phase)
            have = len(interpret(el))
            if form.startswith("lit"):
                el.append(literal(_rand(rng, 9), int(form[3])))
            else:
                el.append(copy(11, have if form == "copy1" or phase % 2 else min(have, 7), int(form[4])))
            el.append(literal(_rand(rng, 2)))
            chunks.append(("snappy", el))
        blocks.append(block(chunks))
    # literals that end exactly on the window edge: at byte 63 (the next element starts at phase 63) and at byte 64 (it opens a window)
    blocks.append(block([("snappy", [literal(_rand(rng, 61)), literal(_rand(rng, 3)), copy(5, 2, 2)]),
                         ("snappy", [literal(_rand(rng, 62)), literal(_rand(rng, 3)), copy(5, 2, 2)])]))
    return tiny(blocks)


FRAMING_WIDTHS = [(DENSE_TINYINT, 1), (DENSE_STRING, 2), (DENSE_STRING, 5)]


@functools.lru_cache(maxsize=None)
def snappy_framing(width):
    """one segment: an empty block between full ones, stored and compressed chunks mixed, short chunks that are not the last, zero-length
    chunks, padded preambles, destinations on every byte phase"""
    rng = np.random.default_rng(700 + width)
    dense = {w: c for c, w in FRAMING_WIDTHS}[width]
    blocks = [block([("snappy", [literal(_rand(rng, 3 * width - 1)), copy(1, 1, 2)])]),         # 3 rows: the next block starts off a dword
              block([])]                                                                         # the empty block
    big = [literal(_rand(rng, 1024))]
    grow(rng, big, 1024, CHUNK_MAX, kind=3)
    first = 101 if width == 2 else 100                                                           # (100 + 32768 + 7 is odd)
    blocks.append(block([("stored", _rand(rng, first)), ("snappy", big), ("stored", _rand(rng, 7))]))
    blocks.append(block([("snappy", [literal(_rand(rng, 2 * width)), copy(width, 2 * width, 1 if 4 <= width <= 11 else 2)]), ("stored", b""), ("snappy", []),
                         ("stored", _rand(rng, width)), ("stored", b"")]))
    blocks.append(block([("snappy", [literal(_rand(rng, width * nb)), copy(width * nb, width * nb, 3)], nb) for nb in (2, 3, 4, 5)]))
    blocks.append(block([("stored", _rand(rng, 33)), ("snappy", [literal(_rand(rng, 20)), copy(32 - 20 - (width != 5), 9, 2)])]))   # 33 + 31 | 33 + 32
    # dword-aligned destinations with every ulen % 4: a filler block first, so that this one starts on a dword
    rows = sum(len(b.expected) for b in blocks) // width
    filler = [f for f in range(4) if ((rows + f) * width) % 4 == 0][0]
    if filler:
        blocks.append(block([("stored", _rand(rng, filler * width))]))
    sizes = [8, 9, 3, 6, 2, 7, 1]                                                                # done = 0, 8, 17, 20, 26, 28, 35
    sizes += [(-sum(sizes)) % width] if sum(sizes) % width else []
    blocks.append(block([("stored", _rand(rng, n)) if i % 2 else ("snappy", [literal(_rand(rng, n))]) for i, n in enumerate(sizes)]))
    return AssembledSnappyColumn(dense, width, blocks)


@functools.lru_cache(maxsize=None)
def snappy_lds_edge():
    """{"stored_fits" / "stored_over": one stored chunk of the largest size that fits / one byte more;
        "full_fits" / "full_over": a compressed chunk of CHUNK_MAX output bytes in the largest stored block that fits / one byte more}"""
    rng = np.random.default_rng(63)
    n, b = largest_stored_chunk(), largest_block_beside_full_chunk()
    out = {"stored_fits": tiny([block([("stored", _rand(rng, n))])]), "stored_over": tiny([block([("stored", _rand(rng, n + 1))])])}
    for name, size in (("full_fits", b), ("full_over", b + 1)):
        blk = block([("snappy", fit_elements(rng, CHUNK_MAX, size - 14 - 3))])
        assert len(blk.raw) == size
        out[name] = tiny([blk])
    return out


def snappy_columns():
    """every snappy column the GPU file decodes or expects refused, by name (the census walks them)"""
    f = snappy_forms()
    out = {"forms": f["decodes"], "overlap": snappy_overlap_matrix(), "phases": snappy_window_phases()}
    out.update({"framing%d" % w: snappy_framing(w) for _, w in FRAMING_WIDTHS})
    out.update({"whole_chunk_literal%d" % i: c for i, c in enumerate(f["whole_chunk_literals"])})
    out.update({"largest_literal%d" % i: c for i, c in enumerate(f["largest_literals"])})
    out.update(snappy_lds_edge())
    return out


# =====================================================================================================================
# PFOR_INT
# =====================================================================================================================
def vbyte(delta, n_bytes):
    """7 bits per byte, low group first, 0x80 on the value's LAST byte; zero groups pad a value to n_bytes"""
    assert 1 <= n_bytes <= 5 and 0 <= delta < min(1 << 32, 1 << (7 * n_bytes))
    out = [(delta >> (7 * i)) & 127 for i in range(n_bytes)]
    out[-1] |= 128
    return bytes(out)


def pfor_block(minis, tail, declared_count=None):
    """(block bytes, expected int32 values).  minis: [(width, 32 deltas)] -- width 32: the 32 values themselves; tail: [(delta, n_bytes)].
    Layout (csrc/imm3_codec.hip's header comment): the count word; one header (b1<<24)|(b2<<16)|(b3<<8)|b4 per four mini-blocks, one
    header word per leftover one; a mini-block's value i in bits [i*b, (i+1)*b) of its little-endian bit stream; the tail's bytes packed
    little-endian into words (byte 0 of a tail word is the LOW byte of the big-endian word); every word big-endian; eight zero bytes."""
    words, values, prev = [], [], 0
    n = 32 * len(minis) + len(tail)
    words.append(n if declared_count is None else declared_count)

    def pack(width, vals):
        nonlocal prev
        vals = [int(v) & 0xFFFFFFFF for v in vals]
        assert len(vals) == 32 and 0 <= width <= 32
        if width == 32:
            values.extend(vals)
            prev = vals[-1]
            return vals
        stream = 0
        for i, d in enumerate(vals):
            assert d < 1 << width, (d, width)
            stream |= d << (i * width)
            prev = (prev + d) & 0xFFFFFFFF
            values.append(prev)
        return [(stream >> (32 * k)) & 0xFFFFFFFF for k in range(width)]

    g = 0
    while g + 4 <= len(minis):
        ws = [w for w, _ in minis[g:g + 4]]
        words.append((ws[0] << 24) | (ws[1] << 16) | (ws[2] << 8) | ws[3])
        for w, vals in minis[g:g + 4]:
            words += pack(w, vals)
        g += 4
    for w, vals in minis[g:]:
        words.append(w)
        words += pack(w, vals)
    by = bytearray()
    for delta, n_bytes in tail:
        by += vbyte(delta, n_bytes)
        prev = (prev + delta) & 0xFFFFFFFF
        values.append(prev)
    by += bytes(-len(by) % 4)
    words += [int.from_bytes(by[i:i + 4], "little") for i in range(0, len(by), 4)]
    raw = b"".join(w.to_bytes(4, "big") for w in words) + bytes(8)
    return raw, np.array(values, dtype=np.uint32).view(np.int32)


def both_oracles_pfor(raw, expected):
    oracle_c.build()
    assert oracle_c.pfor_decode_block(raw).tolist() == expected.tolist(), "the C oracle reads the assembled block differently"
    assert oracle_np.pfor_decode_block(raw).tolist() == expected.tolist(), "the numpy oracle reads the assembled block differently"


class AssembledPforColumn:
    """PforColumn's interface over assembled blocks [(bytes, expected values)]; `meta` is whatever the case list wants the census to see"""

    def __init__(self, blocks, meta=None):
        self.codec, self.width, self.meta = PFOR_INT, 4, meta
        for raw, exp in blocks:
            both_oracles_pfor(raw, exp)
        self.block_rows = [int(exp.size) for _, exp in blocks]
        self.values = np.concatenate([exp for _, exp in blocks]) if blocks else np.zeros(0, np.int32)
        self._dense = RawColumn(DENSE_INT, 4, self.values, self.block_rows)
        self.dat = np.frombuffer(b"".join(raw for raw, _ in blocks), dtype=np.uint8).copy()
        self.offsets = np.concatenate([[0], np.cumsum([len(raw) for raw, _ in blocks])]).astype(np.int32)

    def ocol(self):
        return self._dense.ocol()

    def npcol(self):
        return self._dense.npcol()

    def native(self):
        return (self.codec, self.width, self.dat, self.dat.size, self.offsets)


INT_MIN, INT_MAX = 0x80000000, 0x7FFFFFFF


def deltas_of(rng, bits):
    """32 random deltas of exactly `bits` bits (the top one set); bits == 32: raw values"""
    if bits == 0:
        return [0] * 32
    return [int(x) | (1 << (bits - 1)) for x in rng.integers(0, 1 << (bits - 1), 32)]


def raw_values(rng):
    v = [int(x) for x in rng.integers(0, 1 << 32, 32)]
    v[3], v[17], v[31] = INT_MIN, INT_MAX, INT_MAX - int(rng.integers(0, 3))      # the packed deltas behind it wrap
    return v


def mini(rng, width, bits=None):
    return (width, raw_values(rng) if width == 32 else deltas_of(rng, width if bits is None else bits))


def _pack_groups(groups, rng):
    """groups of four mini-blocks -> blocks of 1024 rows; the last block is filled up with width-9 mini-blocks"""
    minis = [m for g in groups for m in g]
    while len(minis) % 32:
        minis.append(mini(rng, 9))
    return [pfor_block(minis[i:i + 32], []) for i in range(0, len(minis), 32)]


@functools.lru_cache(maxsize=None)
def pfor_widths():
    """every width 0..32 at each position of a group, the neighbours at other widths; then declared 1..5 bits wider than the deltas
    need (never 32: that width means values, not deltas).  meta: [(position, declared, bits of the deltas)]"""
    rng = np.random.default_rng(33)
    groups, meta = [], []
    for j in range(33):
        ws = [(j + 8 * p) % 33 for p in range(4)]
        groups.append([mini(rng, w) for w in ws])
        meta += [(p, w, w) for p, w in enumerate(ws)]
    for j in range(33):
        g = []
        for p in range(4):
            bits = (j + 8 * p) % 33
            declared = min(31, bits + 1 + (j + p) % 5) if bits < 31 else bits
            g.append(mini(rng, declared, bits))
            meta.append((p, declared, bits))
        groups.append(g)
    return AssembledPforColumn(_pack_groups(groups, rng), meta)


@functools.lru_cache(maxsize=None)
def pfor_leftover_widths():
    """ragged blocks (decode path): every width 0..32 in a leftover mini-block, one to three leftovers behind zero or one group.
    meta: [leftover widths per block]"""
    rng = np.random.default_rng(34)
    blocks, meta = [], []
    for w in range(33):
        left = [w] + [(0, 1, 31, 32)[(w + i) % 4] for i in range(w % 3)]
        minis = [mini(rng, int(x)) for x in rng.integers(0, 33, 4 * (w % 2))] + [mini(rng, x) for x in left]
        blocks.append(pfor_block(minis, []))
        meta.append(left)
    return AssembledPforColumn(blocks, meta)


RAW_EXTRA = [(7, 8), (15, 16), tuple(range(32)), (0,), (13,)]           # raw at both sides of a DPP row / bcast boundary, all raw, raw + all width 0


@functools.lru_cache(maxsize=None)
def pfor_raw_positions():
    """block p < 32: a raw mini-block at position p among packed ones; then RAW_EXTRA (the last two: every other mini-block has width 0).
    meta: [raw positions per block]"""
    rng = np.random.default_rng(35)
    blocks, meta = [], []
    for k, raws in enumerate([(p,) for p in range(32)] + RAW_EXTRA):
        zero = k >= 32 + 3
        minis = [mini(rng, 32) if p in raws else mini(rng, 0 if zero else int(rng.choice([1, 2, 5, 13, 20, 31]))) for p in range(32)]
        blocks.append(pfor_block(minis, []))
        meta.append(raws)
    return AssembledPforColumn(blocks, meta)


LEFTOVER_K = [0, 1, 2, 3, 5, 6, 7, 35]


def tail_of(rng, t, salt=0):
    """t tail values whose deltas take 1..5 bytes in turn (the minimal form of a delta of that size; every fifth value one byte longer
    than it needs), 5-byte ones with the top bit set: a negative delta"""
    out = []
    for j in range(t):
        nb = 1 + (j + salt) % 5
        lo = 0 if nb == 1 else 1 << (7 * (nb - 1))
        hi = min(1 << 32, 1 << (7 * nb))
        d = int(rng.integers(lo, hi))
        if nb == 5:
            d |= 1 << 31
        if (j + salt) % 7 == 3 and nb > 1:
            d = int(rng.integers(0, lo))                                  # padded: a zero top group
        out.append((d, nb))
    return out


@functools.lru_cache(maxsize=None)
def pfor_leftovers_and_tails():
    """blocks of 32 k + t values, k in LEFTOVER_K, t in 0..31 (decode path).  meta: [(k, t, leftover widths, tail)]"""
    rng = np.random.default_rng(36)
    blocks, meta = [], []
    for k in LEFTOVER_K:
        for t in range(32):
            n_left = k % 4
            minis = [mini(rng, int(x)) for x in rng.integers(0, 33, k - n_left)]
            left = [(0, 1, 31, 32)[(t + i + k) % 4] for i in range(n_left)]
            minis += [mini(rng, w) for w in left]
            tail = tail_of(rng, t, salt=k)
            blocks.append(pfor_block(minis, tail))
            meta.append((k, t, left, tail))
    return AssembledPforColumn(blocks, meta)


TILE_TAIL_ROWS = [1, 5, 31, 33, 64 + 7, 128 + 31, 512 + 3, 1000, 1023]


@functools.lru_cache(maxsize=None)
def pfor_tile_tails():
    """[column]: a full 1024-row block, then a last block of 1..1023 rows (leftover mini-blocks and a tail of every byte count)"""
    rng = np.random.default_rng(37)
    cols = []
    for i, r in enumerate(TILE_TAIL_ROWS):
        full = pfor_block([mini(rng, int(x)) for x in rng.integers(0, 33, 32)], [])
        last = pfor_block([mini(rng, int(x)) for x in rng.integers(0, 33, r // 32)], tail_of(rng, r % 32, salt=i))
        cols.append(AssembledPforColumn([full, last], r))
    return cols


@functools.lru_cache(maxsize=None)
def pfor_chunk_carry():
    """blocks of 2048 and 4096 + 77 rows: the last mini-block of every 1024-value chunk raw and the next chunk's first packed, then the
    other way round.  meta: [(rows, "raw last" | "raw first")]"""
    rng = np.random.default_rng(38)
    blocks, meta = [], []
    for rows in (2048, 4096 + 77):
        for raw_last in (True, False):
            minis = []
            for m in range(rows // 32):
                edge = m % 32 == 31 if raw_last else m % 32 == 0
                other = m % 32 == 0 if raw_last else m % 32 == 31
                minis.append(mini(rng, 32) if edge else mini(rng, int(rng.choice([3, 17, 31]))) if other else mini(rng, int(rng.integers(0, 32))))
            blocks.append(pfor_block(minis, tail_of(rng, rows % 32)))
            meta.append((rows, "raw last" if raw_last else "raw first"))
    return AssembledPforColumn(blocks, meta)


def pfor_fused_predicates(col):
    """EQ of the values at rows 15, 16, 1023 and the last row, and a range whose ends are values of the column (GT / LT are strict)"""
    from conftest import EQ, GT, LT
    v = col.values
    rows = sorted({r for r in (15, 16, 1023, v.size - 1) if 0 <= r < v.size})
    sels = [[(0, EQ, float(v[r]))] for r in rows]
    lo, hi = sorted((int(v[v.size // 3]), int(v[(2 * v.size) // 3])))
    sels.append([(0, GT, float(lo) - 1.0), (0, LT, float(hi) + 1.0)])
    return sels


# =====================================================================================================================
# malformed blocks: valid framing, valid CRC (over what a decoder WITHOUT the check under test would produce), one step over the line
# =====================================================================================================================
def snappy_malformed():
    """[(name, block bytes, "create" | "use", the comparison in csrc/imm3_snappy.hip that refuses it)].  Every violation stays within
    a byte or two of its bound and every preamble is no multiple of 16, so that even a missing check would leave the decoder inside
    its LDS windows (out_cap rounds the largest chunk up to 16) and inside the column."""
    rng = np.random.default_rng(404)
    p10, p9, p301 = _rand(rng, 10), _rand(rng, 9), _rand(rng, 301)
    cut = lambda k, tail: Raw(bytes([k | (3 << 2)]) + tail, produces=p10[:4])     # a copy of 4 bytes whose offset bytes are cut short
    cases = [
        # k_snappy_decode, copy arm: `eoff == 0`
        ("copy offset 0", block([("snappy", [literal(p10), Raw(bytes([2 | (3 << 2), 0, 0]), produces=bytes(4))])]), "use", "eoff == 0"),
        # ... `eoff > op` (op = 10, offset 11)
        ("copy offset = written + 1", block([("snappy", [literal(p10), Raw(bytes([2 | (3 << 2), 11, 0]), produces=bytes(4))])]), "use", "eoff > op"),
        # ... `eoff > op` with all four offset bytes in eoff (`off = le`): no chunk is long enough for a kind-3 offset above 65535, so
        # the high offset bytes can only be seen through the refusal; the CRC is that of the copy at offset 5, which dropping them gives
        ("kind-3 copy offset 2^24 + 5", block([("snappy", [literal(p10), Raw(bytes([3 | (3 << 2), 5, 0, 0, 1]), produces=p10[5:9])])]), "use", "eoff > op"),
        # ... `op + elen > want` (10 + 5 > 14)
        ("copy ends 1 past the preamble", block([("snappy", [literal(p10), copy(5, 10, 2)], None, 14)]), "use", "op + elen > want"),
        # literal arm: `src + elen > end` (the tag says 6 bytes, 5 are left); want = 15
        ("literal ends 1 past the payload", block([("snappy", [literal(p9), Raw(bytes([5 << 2]) + p10[:5], produces=p10[:5] + b"\0")])]), "use", "src + elen > end"),
        # ... `op + elen > want` (9 + 6 > 14)
        ("literal ends 1 past the preamble", block([("snappy", [literal(p9), literal(p10[:6])], None, 14)]), "use", "op + elen > want"),
        # copy arm: `src > end` (src = the element's start + its header size: one past the payload's end)
        # (kind 1: the missing low offset byte reads as 0, so the tag's high offset bits say 256 and 301 bytes stand in front)
        ("kind-1 copy header cut off", block([("snappy", [literal(p301), Raw(bytes([1 | (1 << 5)]), produces=p301[45:49])])]), "use", "src > end"),
        ("kind-2 copy header cut off", block([("snappy", [literal(p10), cut(2, bytes([10]))])]), "use", "src > end"),
        ("kind-3 copy header cut off", block([("snappy", [literal(p10), cut(3, bytes([10, 0, 0]))])]), "use", "src > end"),
        # after the element loop: `op != want` (10 != 11)
        ("output 1 byte short of the preamble", block([("snappy", [literal(p10)], None, 11)]), "use", "op != want"),
        # the literal length 0xFFFFFFFF + 1 must not wrap to a literal of no bytes: `src + elen > end` with elen clamped to 0x00FFFFFF
        ("literal of 2^32 bytes", block([("snappy", [literal(p10), Raw(bytes([63 << 2, 255, 255, 255, 255])), literal(p9[:4])])]), "use", "src + elen > end"),
        # k_snappy_sizes: `!done` after five preamble bytes that all carry the continuation bit
        ("five continuation bytes in the preamble", block([("snappy", [Raw(bytes([0x8A, 0x80, 0x80, 0x80, 0x80, 0x00])), literal(p10)], None, 0)]), "create", "bad |= !done"),
        # k_snappy_sizes: `u > 32768u`.  (The chunk holds 32768 bytes: the oracles, which know no such limit, refuse the length mismatch.)
        ("preamble 32769", block([("snappy", fit_elements(rng, CHUNK_MAX, 4000), None, CHUNK_MAX + 1)]), "create", "u > 32768u"),
        # k_snappy_sizes: `flag > 1`
        ("flag 2", block([("snappy", [literal(p10)])], flag=2), "create", "flag > 1"),
        # k_snappy_sizes: `ip + plen > n`
        ("payload length 1 past the block", block([("snappy", [literal(p10)])], length_delta=1), "create", "ip + plen > n"),
    ]
    out = []
    for name, blk, where, why in cases:
        raw = blk.raw
        if name.startswith("five"):     # block() put its own preamble (0) in front: the five bytes ARE the preamble
            body = blk.chunks[0].raw[1:]
            raw = STREAM_HEADER + bytes([1]) + len(body).to_bytes(2, "big") + oracle_np.crc32c_masked(p10).to_bytes(4, "big") + body
        out.append((name, raw, where, why))
    return out


def pfor_malformed():
    """[(name, block bytes, rows the count word declares, the comparison in csrc/imm3_codec.hip that refuses it)]; every block is
    the last (only) block of its segment, so both k_filter_pfor and k_pfor_decode read it."""
    rng = np.random.default_rng(405)
    be = lambda words: b"".join(int(w).to_bytes(4, "big") for w in words)
    rnd = lambda n: [int(x) for x in rng.integers(0, 1 << 32, n)]
    cases = []
    for p in range(4):          # pfor_chunk: `wide = b > 32u` -> `__ballot(wide) != 0`; the 33 words the width asks for are there
        ws = [5, 6, 7, 8]
        ws[p] = 33
        cases.append(("width 33 at group position %d" % p, be([128, (ws[0] << 24) | (ws[1] << 16) | (ws[2] << 8) | ws[3]] + rnd(sum(ws))) + bytes(8), 128, "b > 32u"))
    cases.append(("width 33 in a leftover", be([32, 33] + rnd(33)) + bytes(8), 32, "b > 32u"))
    # pfor_chunk: `pos > avail` -- the widths end one word past the block (its eight zero bytes included)
    cases.append(("group widths end one word past the block", be([128, 0x04040404] + rnd(16 - 3)) + bytes(8), 128, "pos > avail"))
    cases.append(("leftover width ends one word past the block", be([32, 9] + rnd(9 - 3)) + bytes(8), 32, "pos > avail"))
    # the tail loop: `shift > 28` at a value's sixth byte
    six = bytes([1, 1, 1, 1, 1, 0x81, 0x82, 0, 0, 0, 0, 0])
    cases.append(("tail value of six bytes", be([2]) + b"".join(six[i:i + 4][::-1] for i in range(0, 12, 4)) + bytes(8), 2, "shift > 28"))
    # the tail loop: `byte >= avail * 4` -- the second value's fourth byte would be the first byte past the block.  (No eight zero
    # bytes behind it: they carry no end mark, so with them the value would be refused as one of more than five bytes.)
    cases.append(("tail runs one byte past the block", be([2]) + bytes([0x85, 1, 1, 1][::-1]), 2, "byte >= avail * 4"))
    return cases
