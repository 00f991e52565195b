"""GPU suite: a launch census of the select run.  The other suites check what a run computes; this one also checks WHICH launches
computed it.  With the context's kernel timing on, every launch takes one timing record under its kernel id (include/imm3_diag.h:
0 select, 1 offsets scan, 2 gather, 3 count reduce), so the records of one run, counted per id, are the passes the run enqueued:
tile passes of up to kMaxTileCols = 3 columns with at most one 2-byte string column each, one launch per fused PFOR_INT predicate,
one per string column whose width is a multiple of 4, word-at-a-time passes of up to kMaxPredCols = 4 columns, and the count
reduce (k_total) whenever the chain is more than one tile launch (or tuning variant 7 asks for it).  A limit scan is one select
launch per chunk (the chunks end at tiles 1024, 8192, 32 768, ...: csrc/imm3_planner.cpp, limit_chunk_ends); what follows it is
run_project's business, which the split of run_select into launchers did not touch: for a limit of 10 no offsets scan, one fused
gather (k_limit_gather: limit_gather_applies, csrc/imm3_run.cpp), no count reduce (the chunks add to the running count).  Every case
also holds the count, and the bitmap where the run stored one, against numpy."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, GT, LT, MATCH, PforColumn, RawColumn, blocks_of
from immutable3_amd import native

pytestmark = pytest.mark.gpu

N = 3 * 1024 + 17                                                       # 3 tiles and a partial one


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    c.timing_enable(64)
    yield c
    c.close()


def census(ctx):
    return [int(ctx.timing_collect(k).size) for k in range(4)]


def strings(rng, n, width, pool=5):
    values = rng.integers(97, 123, size=(pool, width)).astype(np.uint8)
    return values[rng.integers(0, pool, size=n)].copy(), [bytes(v) for v in values]


def is_in(col, values):
    keep = np.zeros(col.shape[0], bool)
    for v in values:
        keep |= (col == np.frombuffer(v, np.uint8)).all(axis=1)
    return keep


SELECT_NAMES = ["one int32 range", "one int32 range, count by k_total", "no predicate", "four int32 columns", "two 2-byte strings and an int32",
                "one 8-byte string", "one 3-byte string", "five 3-byte strings", "a fused PFOR_INT column and an int32"]


@pytest.fixture(scope="module")
def select_cases(oracle):
    """name -> (columns, used, sels, keep, tuning variant, expected launches of kernel ids 0 and 3); built once (the PFOR_INT blocks
    come from the oracle's encoder)"""
    rng = np.random.default_rng(2024)
    br = blocks_of(N, 1024)
    i32 = [rng.integers(0, 1000, size=N).astype(np.int32) for _ in range(4)]
    icol = [RawColumn(DENSE_INT, 4, v, br) for v in i32]
    one_range = ([icol[0]], [0], [(0, GT, 100.0), (0, LT, 600.0)], (i32[0] > 100) & (i32[0] < 600))
    cases = {
        "one int32 range": one_range + (0, 1, 0),
        "one int32 range, count by k_total": one_range + (7, 1, 1),
        "no predicate": ([icol[0]], [0], [], np.ones(N, bool), 0, 1, 0),
        "four int32 columns": (icol, [0, 1, 2, 3], [(k, GT, 200.0) for k in range(4)],
                               (i32[0] > 200) & (i32[1] > 200) & (i32[2] > 200) & (i32[3] > 200), 0, 2, 1),
    }
    s2a, va = strings(rng, N, 2)
    s2b, vb = strings(rng, N, 2)
    cases["two 2-byte strings and an int32"] = (
        [RawColumn(DENSE_STRING, 2, s2a, br), RawColumn(DENSE_STRING, 2, s2b, br), icol[0]], [0, 1, 2],
        [(0, MATCH, va[:3]), (1, MATCH, vb[:2]), (2, GT, 100.0)], is_in(s2a, va[:3]) & is_in(s2b, vb[:2]) & (i32[0] > 100), 0, 2, 1)
    s8, v8 = strings(rng, N, 8)
    cases["one 8-byte string"] = ([RawColumn(DENSE_STRING, 8, s8, br)], [0], [(0, MATCH, v8[:2])], is_in(s8, v8[:2]), 0, 1, 1)
    s3 = [strings(rng, N, 3) for _ in range(5)]
    cases["one 3-byte string"] = ([RawColumn(DENSE_STRING, 3, s3[0][0], br)], [0], [(0, MATCH, s3[0][1][:2])], is_in(s3[0][0], s3[0][1][:2]), 0, 1, 1)
    keep = np.ones(N, bool)
    for col, vals in s3:
        keep &= is_in(col, vals[:4])
    cases["five 3-byte strings"] = ([RawColumn(DENSE_STRING, 3, col, br) for col, _ in s3], [0, 1, 2, 3, 4],
                                    [(k, MATCH, s3[k][1][:4]) for k in range(5)], keep, 0, 2, 1)
    ids = np.arange(N, dtype=np.int32) * 2
    cases["a fused PFOR_INT column and an int32"] = ([PforColumn(ids, br), icol[0]], [0, 1], [(0, GT, 1000.0), (0, LT, 5000.0), (1, GT, 100.0)],
                                                     (ids > 1000) & (ids < 5000) & (i32[0] > 100), 0, 2, 1)
    assert list(cases) == SELECT_NAMES
    return cases


def packed(keep, total_words):
    return np.packbits(keep, bitorder="little").tobytes()[: total_words * 8].ljust(total_words * 8, b"\0")


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_run_select_enqueues_one_launch_per_pass(ctx, select_cases, name):
    cols, used, sels, keep, variant, n_select, n_total = select_cases[name]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    ctx.set_tuning(variant)
    try:
        q = native.DeviceQuery(ctx, seg, used, sels)
        for rnd in range(2):
            ctx.timing_reset()
            q.run_select()
            got = census(ctx)
            print(name, rnd, "launches per kernel id 0..3:", got)
            assert got == [n_select, 0, 0, n_total], (name, rnd, got)
            assert q.count() == int(keep.sum()), (name, rnd)
            assert q.bitmap().tobytes() == packed(keep, q.total_words), (name, rnd)
        q.close()
    finally:
        ctx.set_tuning(0)
        seg.close()


def test_run_count_is_the_one_tile_launch(ctx, select_cases):
    cols, used, sels, keep, _, _, _ = select_cases["one int32 range"]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    q = native.DeviceQuery(ctx, seg, used, sels)
    for rnd in range(2):
        ctx.timing_reset()
        q.run_count()                                                    # (stores no bitmap)
        got = census(ctx)
        print("run_count", rnd, "launches per kernel id 0..3:", got)
        assert got == [1, 0, 0, 0], (rnd, got)
        assert q.count() == int(keep.sum()), rnd
    q.close()
    seg.close()


# tiles of the segment -> launches per kernel id 0..3 of one run().  Id 0: the chunks of the schedule (ends 1024 | 1025 and
# 1024 | 8192 | 8193).  Ids 1 - 3: what run_project does behind a limit scan, unchanged by the split of run_select (no offsets scan
# and one gather: k_limit_gather takes a limit of 10; no k_total: the chunks add to the running count themselves).
LIMIT_CENSUS = {1025: [2, 0, 1, 0], 8193: [3, 0, 1, 0]}


@pytest.mark.parametrize("n_tiles", list(LIMIT_CENSUS))
def test_limit_scan_is_one_select_launch_per_chunk(ctx, n_tiles):
    n = n_tiles * 1024 - 1000                                           # (a partial last tile)
    ids = np.arange(n, dtype=np.int32)
    val = (ids * 7 + 3).astype(np.int32)
    br = blocks_of(n, 1024)
    seg = native.DeviceSegment(ctx, [RawColumn(DENSE_INT, 4, ids, br).native(), RawColumn(DENSE_INT, 4, val, br).native()])
    # select val ... where id > 5 limit 10: a limit keeps the plan off survivor records and off the one launch (the bitmap path)
    q = native.DeviceQuery(ctx, seg, [0, 1], [(0, GT, 5.0)], [1], 10)
    plan = q.plan()
    assert not plan["single_pass"] and not plan["records"], plan
    want = np.flatnonzero(ids > 5)[:10]
    for rnd in range(2):
        ctx.timing_reset()
        q.run()
        got = census(ctx)
        print(n_tiles, rnd, "launches per kernel id 0..3:", got)
        assert got == LIMIT_CENSUS[n_tiles], (n_tiles, rnd, got)
        idx, vals = q.fetch_rows()
        assert idx.tolist() == want.tolist() and vals[0].tobytes() == val[want].tobytes(), (n_tiles, rnd)
    assert q.count() == n - 6                                           # (the whole select runs now)
    assert q.bitmap().tobytes() == packed(ids > 5, q.total_words)
    q.close()
    seg.close()
