"""The block decoders (csrc/imm3_snappy.hip: k_snappy_decode; csrc/imm3_codec.hip: pfor_chunk under k_filter_pfor and k_pfor_decode)
driven with hand-assembled blocks (codec_streams.py): the streams no encoder writes -- four-byte-offset copies, long literal length
forms, every overlap (offset, length) pair, element headers across the parse window's edge, mixed and empty chunks, byte-phased
destinations, the largest blocks the LDS windows hold; every PFOR width at every header position, wider than the deltas need, raw
mini-blocks at every position of the segmented scan, every tail length and byte count.  Bit-exact against bytes that both CPU oracles
read from the same block (asserted when the column is built); test_codec_streams_host.py asserts that the lists hold what they claim.

Every case: a projection with no predicate (the whole decoded column, byte for byte) and a predicate query (bitmap and count), through
test_gpu_parity.check, and each once more as ONE query run twice.  Malformed blocks must come back as IMM3_ERR_LAYOUT, never as a
fault: each stays one step over the line it crosses, and codec_streams.*_malformed names the comparison that refuses it."""
import numpy as np
import pytest

import codec_streams as cs
from conftest import DENSE_INT, GT, LT, MATCH, RawColumn, blocks_of
from test_gpu_parity import check, ctx  # noqa: F401  (ctx is a fixture)

pytestmark = pytest.mark.gpu

DECODE_LAUNCH, FILTER_LAUNCH = 5, 0                  # include/imm3_diag.h: kernel ids of the timing records


def run_twice(ctx, col, sels, proj, want, fused=False):
    """One query, run twice: both runs give what check() saw.  fused: the predicate must have run on the compressed blocks
    (k_filter_pfor).  imm3_query_plan has no word for that, so the launch records say it: a select launch and NO decode launch on a
    segment made for this query alone -- the column was never decoded, so nothing but k_filter_pfor can have read it."""
    from immutable3_amd import native
    seg = native.DeviceSegment(ctx, [col.native()])
    ctx.timing_enable(64)
    try:
        q = native.DeviceQuery(ctx, seg, [0], sels, proj)
        for _ in range(2):
            q.run()
            assert q.count() == want["count"] and q.bitmap().tolist() == want["words"].tolist()
            if proj:
                idx, vals = q.fetch_rows()
                assert idx.tolist() == want["row_index"].tolist() and vals[0].tobytes() == want["vals"][0].tobytes()
        decodes, filters = int(ctx.timing_collect(DECODE_LAUNCH).size), int(ctx.timing_collect(FILTER_LAUNCH).size)
        q.close()
    finally:
        ctx.timing_enable(0)
        seg.close()
    if fused:
        assert decodes == 0 and filters >= 2, (decodes, filters)
    else:
        assert decodes == 1, decodes                 # decoded once per segment, on first need


def whole_column(ctx, oracle, col):
    """the projection with no predicate IS the decoded column"""
    g = check(ctx, oracle, [col], [0], [], proj=[0])
    assert g["count"] == sum(col.block_rows) and g["vals"][0].tobytes() == col._dense.dat.tobytes()
    run_twice(ctx, col, [], [0], g)


def snappy_case(ctx, oracle, col):
    assert cs.column_fits_lds(col)
    whole_column(ctx, oracle, col)
    if col.width == 1:
        sels = [(0, GT, 0.0), (0, LT, 100.0)]
    else:
        v = col.values
        sels = [(0, MATCH, [bytes(v[0]), bytes(v[v.shape[0] // 2]), bytes(v[-1])])]
    g = check(ctx, oracle, [col], [0], sels)
    assert col.width != 1 or g["count"] == int(((col.values > 0) & (col.values < 100)).sum())
    run_twice(ctx, col, sels, [], g)


def refused_at_creation(ctx, col_native):
    from immutable3_amd import native
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceSegment(ctx, [col_native]).close()
    assert e.value.code == native.ERR_LAYOUT, e.value


# ---- snappy -------------------------------------------------------------------------------------------------------------------------
def test_snappy_forms(ctx, oracle):
    f = cs.snappy_forms()
    snappy_case(ctx, oracle, f["decodes"])
    # a literal of a whole chunk (32768 bytes) stands in 32768 + 20 stored bytes: beside its own output that is more than the LDS
    # windows hold (csrc/imm3_api.cpp: snappy_index; codec_streams.snappy_lds_need states the formula), so the segment is refused;
    # the largest literal that fits is decoded, in each of its length forms
    for col in f["whole_chunk_literals"]:
        assert not cs.column_fits_lds(col)
        refused_at_creation(ctx, col.native())
    for col in f["largest_literals"]:
        snappy_case(ctx, oracle, col)


def test_snappy_overlap_matrix(ctx, oracle):
    snappy_case(ctx, oracle, cs.snappy_overlap_matrix())


def test_snappy_window_phases(ctx, oracle):
    snappy_case(ctx, oracle, cs.snappy_window_phases())


@pytest.mark.parametrize("width", [w for _, w in cs.FRAMING_WIDTHS])
def test_snappy_framing(ctx, oracle, width):
    snappy_case(ctx, oracle, cs.snappy_framing(width))


def test_snappy_lds_window_edge(ctx, oracle):
    """snappy_index (csrc/imm3_api.cpp) gives k_snappy_decode in_cap = (stored block + 3 + 8 + 15) & ~15 bytes for the staged block and
    out_cap = (max(largest chunk, 16) + 15) & ~15 for one chunk, and refuses a segment whose sum exceeds 63 KiB.  At the largest sizes that
    pass, both windows are full to their last 16 bytes: they decode exactly; one byte more is IMM3_ERR_LAYOUT at segment creation."""
    e = cs.snappy_lds_edge()
    for name in ("stored_fits", "full_fits"):
        snappy_case(ctx, oracle, e[name])
    for name in ("stored_over", "full_over"):
        refused_at_creation(ctx, e[name].native())


# ---- PFOR_INT ------------------------------------------------------------------------------------------------------------------------
def pfor_both_paths(ctx, oracle, col):
    """k_pfor_decode: the projection; k_filter_pfor: predicates on a column that is not projected (1024-row blocks)"""
    assert all(r == 1024 for r in col.block_rows[:-1]) and col.block_rows[-1] <= 1024
    whole_column(ctx, oracle, col)
    for sels in cs.pfor_fused_predicates(col):
        g = check(ctx, oracle, [col], [0], sels)
        assert g["count"] >= 1
        run_twice(ctx, col, sels, [], g, fused=True)


def pfor_decode_path(ctx, oracle, col):
    whole_column(ctx, oracle, col)
    v = col.values
    sels = [(0, GT, float(np.sort(v)[v.size // 4])), (0, LT, float(np.sort(v)[(3 * v.size) // 4]))]
    g = check(ctx, oracle, [col], [0], sels, proj=[0])
    run_twice(ctx, col, sels, [0], g)


def test_pfor_widths(ctx, oracle):
    pfor_both_paths(ctx, oracle, cs.pfor_widths())
    pfor_decode_path(ctx, oracle, cs.pfor_leftover_widths())


def test_pfor_raw_positions(ctx, oracle):
    pfor_both_paths(ctx, oracle, cs.pfor_raw_positions())


def test_pfor_leftovers_and_tails(ctx, oracle):
    pfor_decode_path(ctx, oracle, cs.pfor_leftovers_and_tails())


def test_pfor_tile_tail(ctx, oracle):
    for col in cs.pfor_tile_tails():
        pfor_both_paths(ctx, oracle, col)


def test_pfor_chunk_carry(ctx, oracle):
    pfor_decode_path(ctx, oracle, cs.pfor_chunk_carry())


# ---- malformed blocks ----------------------------------------------------------------------------------------------------------------
def good_query(ctx, oracle):
    """the context is as good as before: a correct query right behind the refusal"""
    v = (np.arange(1500, dtype=np.int32) * 3) - 700
    check(ctx, oracle, [RawColumn(DENSE_INT, 4, v, blocks_of(v.size, 1024))], [0], [(0, GT, 10.0), (0, LT, 2000.0)], proj=[0])


def test_malformed_snappy_blocks_are_layout_errors(ctx, oracle):
    from immutable3_amd import native
    for name, raw, where, why in cs.snappy_malformed():
        dat = np.frombuffer(raw, dtype=np.uint8).copy()
        col = (cs.SNAPPY_TINYINT, 1, dat, dat.size, np.array([0, dat.size], dtype=np.int32))
        if where == "create":                        # k_snappy_sizes, behind imm3_segment_create
            refused_at_creation(ctx, col)
        else:                                        # k_snappy_decode, at first use: the query that needs the dense column
            seg = native.DeviceSegment(ctx, [col])
            for proj in ([], [0]):
                with pytest.raises(native.Imm3Error) as e:
                    native.DeviceQuery(ctx, seg, [0], [(0, GT, 0.0)], proj).close()
                assert e.value.code == native.ERR_LAYOUT, (name, why, e.value)
            seg.close()
        good_query(ctx, oracle)


def test_malformed_pfor_blocks_are_layout_errors(ctx, oracle):
    from immutable3_amd import native
    for name, raw, rows, why in cs.pfor_malformed():
        dat = np.frombuffer(raw, dtype=np.uint8).copy()
        seg = native.DeviceSegment(ctx, [(cs.PFOR_INT, 4, dat, dat.size, np.array([0, dat.size], dtype=np.int32))])   # the count word is sound
        q = native.DeviceQuery(ctx, seg, [0], [(0, GT, 5.0)])
        assert q.n_rows == rows
        q.run()                                      # k_filter_pfor: the status word comes back with the count
        with pytest.raises(native.Imm3Error) as e:
            q.count()
        assert e.value.code == native.ERR_LAYOUT, (name, why, e.value)
        q.close()
        with pytest.raises(native.Imm3Error) as e:   # k_pfor_decode: at the creation of the query that needs the dense column
            native.DeviceQuery(ctx, seg, [0], [(0, GT, 5.0)], [0]).close()
        assert e.value.code == native.ERR_LAYOUT, (name, why, e.value)
        seg.close()
        good_query(ctx, oracle)
