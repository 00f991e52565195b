"""GPU suite: Match on string columns whose width is a whole number of dwords (k_filter_str_rows, csrc/imm3_strmatch.hip) over ONE
segment.  Expected bitmaps, counts and rows are the C oracle's scan_select / project (tests/test_str_rows_host.py holds the oracle
against a plain numpy byte compare at width 256); groups are oracle_np's.  The same queries under the word-at-a-time kernel
(tuning variant 1) must give identical bitmaps."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, PforColumn, RawColumn, SnappyColumn, blocks_of
from immutable3_amd import native
from oracle import oracle_np
from str_rows_util import in_lists, make_strings, pool_for

pytestmark = pytest.mark.gpu
TV_GENERIC_ONLY = 1
WIDTHS = [4, 8, 12, 16, 20, 24, 40, 64, 256]      # every instance of the string pass
# rows and blocks: around a bitmap word and a tile, the loader quirk (a trailing 1-row block), blocks that are multiples of 64
SHAPES = [(0, []), (1, [1]), (63, [63]), (64, [64]), (65, [65]), (1023, [1023]), (1024, [1024]), (1025, blocks_of(1025, 1024)),
          (2 * 1024 + 1, [1024, 1024, 1]), (4 * 64 + 5, [64, 128, 64, 5])]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def select_both_ways(ctx, seg, used, sels):
    """(words, count) of run_select under the default plan and under the word-at-a-time kernel"""
    out = []
    for variant in (0, TV_GENERIC_ONLY):
        ctx.set_tuning(variant, 0)
        try:
            q = native.DeviceQuery(ctx, seg, used, sels)
            q.run_select()
            out.append((q.bitmap(), q.count()))
            q.close()
        finally:
            ctx.set_tuning(0, 0)
    return out


@pytest.mark.parametrize("width", WIDTHS)
def test_match_every_shape_and_in_list(ctx, oracle, width):
    rng = np.random.default_rng(1000 + width)
    pool, t0, t1 = pool_for(rng, width)
    for n, block_rows in SHAPES:
        col = RawColumn(DENSE_STRING, width, make_strings(rng, pool, n), block_rows)
        seg = native.DeviceSegment(ctx, [col.native()])
        for values in in_lists(rng, pool, t0, t1, width):
            sels = [(0, MATCH, values)]
            ow, oc = oracle.scan_select([col.ocol()], sels, 1024, 1)
            (w, c), (gw, gc) = select_both_ways(ctx, seg, [0], sels)
            assert c == oc and w.tolist() == ow.tolist(), (n, len(values))
            assert gc == oc and gw.tolist() == ow.tolist(), (n, len(values))
        seg.close()


@pytest.mark.parametrize("width", [20, 64, 256])
def test_prefix_candidates_run_and_reject(ctx, oracle, width):
    """rows that share their first 16 bytes with an IN-list value and differ in the last byte only: the second tile holds nothing but
    such rows (every row a candidate; one of them is the value itself)"""
    rng = np.random.default_rng(2000 + width)
    pool, t0, t1 = pool_for(rng, width)
    near = t0.copy()
    near[-1] ^= 0x20
    n = 2 * 1024 + 1
    v = make_strings(rng, pool, n)
    v[1024:2048] = near
    v[[5, 1500, 2048]] = t0
    col = RawColumn(DENSE_STRING, width, v, [1024, 1024, 1])
    seg = native.DeviceSegment(ctx, [col.native()])
    assert not (pool == near).all(1).any()
    for values, want in (([bytes(t0)], int((v == t0).all(1).sum())), ([bytes(near)], int((v == near).all(1).sum())), ([bytes(t0), bytes(near), bytes(t1)], None)):
        sels = [(0, MATCH, values)]
        ow, oc = oracle.scan_select([col.ocol()], sels, 1024, 1)
        (w, c), (gw, gc) = select_both_ways(ctx, seg, [0], sels)
        assert c == oc and w.tolist() == ow.tolist() and gw.tolist() == ow.tolist() and gc == oc
        if want is not None:
            assert c == want
    seg.close()


def make_mixed(rng, n, block_rows, w_a=16, w_b=8):
    pool_a, a0, a1 = pool_for(rng, w_a)
    pool_b, b0, b1 = pool_for(rng, w_b)
    ids = rng.integers(-50, 50, size=n).astype(np.int32)
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    cols = [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows),
            RawColumn(DENSE_STRING, w_a, make_strings(rng, pool_a, n), block_rows),
            SnappyColumn(DENSE_STRING, w_b, make_strings(rng, pool_b, n), block_rows),
            PforColumn(np.sort(rng.integers(0, 1000, size=n)).astype(np.int32), block_rows)]
    return cols, (pool_a, a0, a1), (pool_b, b0, b1)


@pytest.mark.parametrize("n,block_rows", [(3 * 1024 + 700, [1024] * 3 + [700]), (2 * 1024 + 1, [1024, 1024, 1]), (4 * 64 + 5, [64, 128, 64, 5])])
def test_combined_with_other_passes(ctx, oracle, n, block_rows):
    """the string pass first and as an and_existing pass: beside tile passes (both leaf orders), another string pass of another
    width, a snappy-coded 8-byte column and a PFOR_INT predicate"""
    rng = np.random.default_rng(n)
    cols, (pool_a, a0, a1), (pool_b, b0, b1) = make_mixed(rng, n, block_rows)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    la = [bytes(a0), bytes(a1)] + [bytes(p) for p in pool_a[:6]]
    lb = [bytes(b0), bytes(b1)] + [bytes(p) for p in pool_b[:10]]
    queries = [
        ([2, 0, 1], [(0, MATCH, la), (1, GT, -20.0), (1, LT, 40.0), (2, GT, -100.0), (2, LT, 90.0)]),
        ([0, 1, 2], [(0, GT, -20.0), (0, LT, 40.0), (1, GT, -100.0), (1, LT, 90.0), (2, MATCH, la)]),
        ([2, 3], [(0, MATCH, la), (1, MATCH, lb)]),
        ([3, 2], [(0, MATCH, lb), (1, MATCH, la)]),
        ([3], [(0, MATCH, [bytes(b0)])]),
        ([4, 2], [(0, GT, 100.0), (0, LT, 900.0), (1, MATCH, la)]),
        ([2, 4, 1, 3], [(0, MATCH, la), (1, GT, 100.0), (2, GT, -100.0), (3, MATCH, lb)]),
    ]
    for used, sels in queries:
        ow, oc = oracle.scan_select([cols[i].ocol() for i in used], sels, 1024, 1)
        (w, c), (gw, gc) = select_both_ways(ctx, seg, used, sels)
        assert c == oc and w.tolist() == ow.tolist(), (used, sels[0])
        assert gc == oc and gw.tolist() == ow.tolist(), (used, sels[0])
    seg.close()


@pytest.mark.parametrize("width", [16, 64])
def test_run_modes(ctx, oracle, width):
    """run_count (the bitmap stays readable), a projection with a limit, an unlimited one, a group-by with count / max"""
    rng = np.random.default_rng(3000 + width)
    n, block_rows = 5 * 1024 + 321, [1024] * 5 + [321]
    pool, t0, t1 = pool_for(rng, width)
    ids = rng.integers(-50, 50, size=n).astype(np.int32)
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    cols = [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows),
            RawColumn(DENSE_STRING, width, make_strings(rng, pool, n), block_rows)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    values = [bytes(t0), bytes(t1)] + [bytes(p) for p in pool[:5]]
    used, sels = [2, 0, 1], [(0, MATCH, values), (2, GT, -90.0)]
    ocols = [cols[i].ocol() for i in used]
    ow, oc = oracle.scan_select(ocols, sels, 1024, 1)
    assert 0 < oc < n
    q = native.DeviceQuery(ctx, seg, used, sels)
    q.run_count()
    assert q.count() == oc and q.bitmap().tolist() == ow.tolist()
    q.close()
    for limit in (0, 7, oc):
        proj = [1, 0, 2]
        q = native.DeviceQuery(ctx, seg, used, sels, proj, limit, 1024)
        q.run()
        idx, vals = q.fetch_rows()
        assert q.count() == oc and q.bitmap().tolist() == ow.tolist()
        q.close()
        rows, batch, pos, ovals, _ = oracle.project(ocols, proj, limit, 1024, ow)
        assert idx.tolist() == (batch.astype(np.int64) * 1024 + pos).tolist()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(vals, ovals))
    aggs = [("count", 1), ("max", 1)]
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=[2], aggs=[(native.AGG_COUNT, 1), (native.AGG_MAX, 1)])
    q.run()
    keys, first, counts, gvals = q.fetch_groups()
    q.close()
    _, _, masks = oracle_np.scan_select([cols[i].npcol() for i in used], sels, 1024)
    want = oracle_np.project_agg([cols[i].npcol() for i in used], [2], aggs, masks)
    got = [(str(int.from_bytes(bytes([int(k) & 0xFF]), "little", signed=True)), [int(c), float(int(v[1]))]) for k, c, v in zip(keys, counts, gvals)]
    assert got == [(k, [s[0], s[1]]) for k, s in want.items()]
    seg.close()


def test_device_wrapped_segment_with_a_partial_last_tile(ctx, oracle):
    """imm3_segment_wrap_device promises the kernels 16 KiB behind dat_bytes, a whole tile of a 256-byte column is 256 KiB: the
    buffer here ends 16 KiB behind the column, whose last tile holds 40 rows"""
    import torch
    width, n = 256, 1024 + 40
    rng = np.random.default_rng(77)
    pool, t0, t1 = pool_for(rng, width)
    v = make_strings(rng, pool, n)
    v[[0, 1023, 1024, n - 1]] = t0
    col = RawColumn(DENSE_STRING, width, v, [1024, 40])
    buf = torch.zeros(col.dat.size + 16384, dtype=torch.uint8, device="cuda")
    buf[: col.dat.size] = torch.from_numpy(col.dat).cuda()
    torch.cuda.synchronize()
    seg = native.DeviceSegment(ctx, [(DENSE_STRING, width, buf.data_ptr(), col.dat.size, col.offsets)], wrap_device=True)
    for values in ([bytes(t0)], [bytes(t0), bytes(t1)] + [bytes(p) for p in pool[:9]]):
        sels = [(0, MATCH, values)]
        ow, oc = oracle.scan_select([col.ocol()], sels, 1024, 1)
        q = native.DeviceQuery(ctx, seg, [0], sels)
        q.run_select()
        assert q.count() == oc and q.bitmap().tolist() == ow.tolist()
        q.close()
    seg.close()
    del buf
