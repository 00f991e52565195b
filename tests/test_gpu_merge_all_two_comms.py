"""GPU suite: the host combine of the single-process merges (imm3_comm_merge_groups_all, _merge_groups_wide_all, _merge_ordered_all)
with TWO communicators.  Those entry points run each communicator's local merge on its context and combine the results on the host;
every other test passes one communicator, so the combine never had anything to combine.  Here two contexts on device 0 carry a
world-of-one communicator each (the _all merges use a communicator's context only), four segments are dealt out s mod 2 -- the
global indices interleave -- most keys occur on both sides and a few on one side only, and in one case of each merge the second
communicator's predicate selects nothing.  Expected values: oracle_np.combine_agg, merge_wide_util.host_combine, merge_order_util."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, RawColumn, blocks_of
from immutable3_amd import native
from oracle import oracle_np
import merge_order_util as U
from merge_wide_util import AGGS, COMMON, GROUP, PAIR_FROM2, PAIR_ONLY1, assert_merged, host_combine

pytestmark = pytest.mark.gpu
SIZES = [3000, 1025, 1024, 2049]
N_SEG = len(SIZES)
OWNER = [s % 2 for s in range(N_SEG)]
NOTHING = [(2, GT, 2.0e6)]                                     # val < 10^6: no row selected
KIND = {"count": native.AGG_COUNT, "min": native.AGG_MIN, "max": native.AGG_MAX}


@pytest.fixture(scope="module")
def two():
    """(contexts, communicators): two contexts on device 0, each with a communicator of a world of one"""
    ctxs = [native.Context(0) for _ in range(2)]
    comms = [native.Comm(c, 1, 0, native.comm_unique_id()) for c in ctxs]
    yield ctxs, comms
    for c in comms:
        c.close()
    for c in ctxs:
        c.close()


def dealt(per_segment):
    """per-segment things -> [those of communicator 0, those of communicator 1], and the segments' indices likewise"""
    return [[per_segment[s] for s in range(N_SEG) if OWNER[s] == r] for r in range(2)], [[s for s in range(N_SEG) if OWNER[s] == r] for r in range(2)]


# ---- imm3_comm_merge_groups_all ------------------------------------------------------------------------------------------
def group_columns(rng, s):
    """0: int8 key, 1: int32 key, 2: int32 value.  Keys 0 .. 29 everywhere; 100 on communicator 1 only (segment 1), 101 on
    communicator 0 only (segment 2)."""
    n = SIZES[s]
    k = rng.integers(0, 30, size=n)
    if s in (1, 2):
        k[rng.integers(0, n, size=5)] = 99 + s
    br = blocks_of(n, 1024)
    return [RawColumn(DENSE_TINYINT, 1, k.astype(np.int8), br), RawColumn(DENSE_INT, 4, k.astype(np.int32) * 70_001, br),
            RawColumn(DENSE_INT, 4, rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int32), br)]


def decode_groups(cols, keys, counts, vals, group, aggs):
    got = []
    for g in range(keys.shape[0]):
        raw = int(keys[g]).to_bytes(8, "little")
        parts, off = [], 0
        for gi in group:
            w = cols[gi].width
            parts.append(str(int.from_bytes(raw[off: off + w], "little", signed=True)))
            off += w
        got.append(("_".join(parts), [int(counts[g]) if k == "count" else float(int(vals[g, j])) for j, (k, _) in enumerate(aggs)]))
    return got


@pytest.mark.parametrize("group", [[0], [1], [0, 1]], ids=["direct-table", "hash-list", "hash-list-5-bytes"])
def test_merge_groups_all_combines_two_communicators(two, group):
    ctxs, comms = two
    rng = np.random.default_rng(41)
    cols = [group_columns(rng, s) for s in range(N_SEG)]
    segs = [native.DeviceSegment(ctxs[OWNER[s]], [c.native() for c in cols[s]]) for s in range(N_SEG)]
    aggs = [("count", 2), ("max", 2), ("min", 2)]
    try:
        for what, sels_of in (("all rows", [[], []]), ("communicator 1 selects nothing", [[], NOTHING])):
            per_seg, queries = [], []
            for s in range(N_SEG):
                sels = sels_of[OWNER[s]]
                _, _, masks = oracle_np.scan_select([c.npcol() for c in cols[s]], sels, 1024)
                per_seg.append(oracle_np.project_agg([c.npcol() for c in cols[s]], group, aggs, masks))
                q = native.DeviceQuery(ctxs[OWNER[s]], segs[s], [0, 1, 2], sels, (), 0, 1024, group_cols=group, aggs=[(KIND[k], c) for k, c in aggs])
                q.run()
                queries.append(q)
            want = [(k, v) for k, v in oracle_np.combine_agg(per_seg, aggs).items()]
            qs, idx = dealt(queries)
            keys, first, counts, vals = native.Comm.merge_groups_all(comms, qs, idx)
            assert decode_groups(cols[0], keys, counts, vals, group, aggs) == want, what
            assert (np.diff(first.astype(np.int64)) > 0).all(), what
            if what == "all rows":                             # keys of one side only are there, and both sides contributed to the others
                seen = {int(k.split("_")[0]) // (70_001 if group == [1] else 1) for k, _ in want}
                assert {100, 101} <= seen and len(want) == 32, sorted(seen)
                assert {int(f) >> 32 for f in first} >= {0, 1, 2}, first
            for q in queries:
                q.close()
    finally:
        for s in segs:
            s.close()


# ---- imm3_comm_merge_groups_wide_all -------------------------------------------------------------------------------------
POOLS = [COMMON, COMMON + [PAIR_ONLY1], COMMON[:5] + [PAIR_FROM2], COMMON]      # PAIR_ONLY1: communicator 1 only; PAIR_FROM2: communicator 0 only


def wide_columns(rng, s):
    """merge_wide_util.breaker_columns over this module's sizes and pools: 0 name (16-byte string), 1 k8 (int8), 2 val (int32),
    3 sname (16-byte string)"""
    n, pool = SIZES[s], POOLS[s]
    pick = rng.permutation(np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), size=n)])[:n])
    names = np.stack([pool[i][0] for i in pick])
    k8 = np.array([pool[i][1] for i in pick], np.int8)
    sname = rng.integers(97, 123, size=(n, 16)).astype(np.uint8)
    sname[:, :8] = ord("p")
    br = blocks_of(n, 1024)
    return [RawColumn(DENSE_STRING, 16, names, br), RawColumn(DENSE_TINYINT, 1, k8, br),
            RawColumn(DENSE_INT, 4, rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int32), br), RawColumn(DENSE_STRING, 16, sname, br)]


def test_merge_groups_wide_all_combines_two_communicators(two):
    ctxs, comms = two
    rng = np.random.default_rng(42)
    segs = [native.DeviceSegment(ctxs[OWNER[s]], [c.native() for c in wide_columns(rng, s)]) for s in range(N_SEG)]
    try:
        for what, sels_of in (("all rows", [[], []]), ("communicator 1 selects nothing", [[], NOTHING])):
            queries = []
            for s in range(N_SEG):
                q = native.DeviceQuery(ctxs[OWNER[s]], segs[s], [0, 1, 2, 3], sels_of[OWNER[s]], (), 0, 1024, group_cols=GROUP, aggs=AGGS, wide_keys=True)
                q.run()
                queries.append(q)
            want = host_combine(queries, list(range(N_SEG)))
            qs, idx = dealt(queries)
            assert_merged(native.Comm.merge_groups_wide_all(comms, qs, idx), want, what)
            assert want[0].shape == ((10, 17) if what == "all rows" else (9, 17)), want[0].shape   # COMMON + the two one-sided keys / COMMON + PAIR_FROM2
            for q in queries:
                q.close()
    finally:
        for s in segs:
            s.close()


# ---- imm3_comm_merge_ordered_all -----------------------------------------------------------------------------------------
def test_merge_ordered_all_combines_two_communicators(two):
    ctxs, comms = two
    rng = np.random.default_rng(43)
    cols = [U.segment_columns(rng, n, 0, few_ids=3) for n in SIZES]              # ids below 3, three ages: (age, id) keys tie across the sides
    segs = [native.DeviceSegment(ctxs[OWNER[s]], [c.native() for c in cols[s]]) for s in range(N_SEG)]
    used, proj, order_by = [U.ID, U.AGE, U.TAG], [0, 1, 2], [(1, True), (0, False)]   # age desc, id
    nothing = [(0, GT, 100.0)]                                                   # id < 3: no row selected
    side = min(sum(SIZES[s] for s in range(N_SEG) if OWNER[s] == r) for r in range(2))
    try:
        for what, sels_of, limit in (("unlimited", [[], []], 0), ("a limit below one side's list", [[], []], side // 3),
                                     ("communicator 1 selects nothing", [[], nothing], 0)):
            queries = [U.ordered_query(native, ctxs[OWNER[s]], segs[s], used, sels_of[OWNER[s]], proj, order_by, limit) for s in range(N_SEG)]
            there = {s: cols[s] for s in range(N_SEG) if sels_of[OWNER[s]] == []}
            want = U.expected(there, used, [], proj, order_by, limit)
            qs, idx = dealt(queries)
            U.assert_rows(native.Comm.merge_ordered_all(comms, qs, idx, limit), want, what)
            assert want[0].size == (limit or sum(SIZES[s] for s in there)), what
            if what != "communicator 1 selects nothing":
                assert (np.diff(want[0]) < 0).any() and set(want[0].tolist()) >= {0, 1}, what   # interleaved: not one side's list after the other's
            for q in queries:
                q.close()
    finally:
        for s in segs:
            s.close()
