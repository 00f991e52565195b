"""GPU suite: views of merged groups on ONE rank, imm3_comm_merge_groups_view[_all] -- filter, then order, then limit over the merged
record list on the device ("Views of merged groups").  Every comparison is exact.  The reference is never the
library's own ordering: merge_groups_wide's output through merge_view_util.reference_view (a filter in Python integers, np.lexsort).

Segments of 3000, 1024, 1 and 0 rows under the global indices 7, 300, 2, 0 (out of order, one above 255: two segment bytes in the
tie).  A 12-byte order key leaves room for no segment byte, so the cases with one run over ONE query under index 0."""
import numpy as np
import pytest

from immutable3_amd import native
from merge_view_util import (AGG, AGGS_A, AGGS_B, AND, CNT, EQ, G_K8KID, G_KID, G_NAME, G_STATE, GCOL, GT, LT, NOT, OR, SEG_INDEX, SIZES, agg_query, assert_view,
                             columns, reference_view)

pytestmark = pytest.mark.gpu

SMALL, FULL, SELECT = native.GROUP_ORDER_SMALL, native.GROUP_ORDER_RADIX_FULL, native.GROUP_ORDER_RADIX_SELECT


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def comm(ctx):
    c = native.Comm(ctx, 1, 0, native.comm_unique_id())
    yield c
    c.close()


@pytest.fixture(scope="module")
def segs(ctx):
    rng = np.random.default_rng(2110)
    out = [native.DeviceSegment(ctx, [c.native() for c in columns(rng, n)]) for n in SIZES]
    yield out
    for s in out:
        s.close()


class Shape:
    """the queries of one (group columns, aggregates) over the four segments, and merge_groups_wide's answer, once"""

    def __init__(self, ctx, comm, segs, group, aggs, only=None):
        which = list(range(len(segs))) if only is None else only
        self.group, self.aggs = group, aggs
        self.queries = [agg_query(ctx, segs[s], [], group, aggs) for s in which]
        self.seg_index = [SEG_INDEX[s] for s in which] if only is None else [0]
        self.merged = comm.merge_groups_wide(self.queries, self.seg_index)

    def close(self):
        for q in self.queries:
            q.close()


@pytest.fixture(scope="module")
def shapes(ctx, comm, segs):
    out = {"state/A": Shape(ctx, comm, segs, G_STATE, AGGS_A), "kid/A": Shape(ctx, comm, segs, G_KID, AGGS_A), "name/B": Shape(ctx, comm, segs, G_NAME, AGGS_B),
           "k8kid/A": Shape(ctx, comm, segs, G_K8KID, AGGS_A), "kid/B": Shape(ctx, comm, segs, G_KID, AGGS_B),
           "name/B one query": Shape(ctx, comm, segs, G_NAME, AGGS_B, only=[0])}
    yield out
    for s in out.values():
        s.close()


def view(order=(), leaves=(), prog=(), limit=0):
    return dict(order=list(order), leaves=list(leaves), prog=list(prog), limit=limit)


def BOTH(key):
    """a key ascending and descending"""
    return [key + (0,), key + (1,)]


# leaves over AGGS_A: the count, MIN(val), MAX(k8), SUM(val), the average of val
L_COUNT, L_MIN, L_MAX, L_SUM, L_AVG = (CNT, 0, GT, 40), (1, 0, LT, -48), (2, 0, EQ, 100), (3, 0, GT, 0), (3, 1, GT, 0)
VIEWS = {
    "state/A": [view([k]) for k in BOTH((GCOL, 0)) + BOTH((AGG, 0)) + BOTH((AGG, 1)) + BOTH((AGG, 2)) + BOTH((AGG, 3))]
               + [view([(AGG, 0, 1)], [L_COUNT], [0], 10), view(leaves=[L_COUNT], prog=[0]), view(leaves=[(0, 0, GT, 10 ** 6)], prog=[0]),
                  view([(AGG, 3, 0)], [(0, 0, GT, 0)], [0]), view(limit=5), view()],
    "kid/A": [view([k]) for k in BOTH((GCOL, 0)) + BOTH((AGG, 2))]                 # MAX(k8) has 4 values: the ties span segments, `first` decides
             + [view([(AGG, 2, 1), (AGG, 0, 0)]), view([(AGG, 2, 0)], [L_MIN], [0])]
             + [view([(AGG, 0, 1)], [leaf], [0], 7) for leaf in (L_COUNT, L_MIN, L_MAX, L_SUM, L_AVG)]
             + [view([(AGG, 3, 1)], [L_SUM, L_MAX, L_MIN], [0, 1, OR, 2, NOT, AND]), view([(GCOL, 0, 1)], limit=1), view([(GCOL, 0, 1)], limit=10 ** 6),
                view()],
    "k8kid/A": [view([k]) for k in BOTH((GCOL, 0)) + BOTH((GCOL, 1))]
               + [view([(GCOL, 0, 1), (AGG, 2, 0), (AGG, 1, 1), (GCOL, 1, 0)]), view([(GCOL, 0, 0)], [L_AVG], [0], 3), view()],      # four keys: 1 + 1 + 4 + 4 bytes
    "kid/B": [view([k]) for k in BOTH((AGG, 2))] + [view([(AGG, 2, 1), (AGG, 0, 0)], [(1, 0, LT, 0)], [0], 20), view()],             # MAX over a 4-byte string (4 + 5 bytes)
    "name/B": [view([(AGG, 0, 1)]), view([(AGG, 2, 0), (AGG, 0, 1)], [(CNT, 0, GT, 45)], [0]), view(limit=3), view()],                 # a 12-byte group key: wide records
    "name/B one query": [view([k]) for k in BOTH((GCOL, 0)) + BOTH((AGG, 3))] + [view([(AGG, 3, 1)], [(CNT, 0, GT, 30)], [0], 4), view()],   # 12-byte keys, S = 0
}


def run_views(comm, shape, views, what):
    for v in views:
        want = reference_view(shape.merged, shape.group, shape.aggs, **v)
        got = comm.merge_groups_view(shape.queries, shape.seg_index, **v)
        assert_view(got, want, (what, v))


@pytest.mark.parametrize("radix", [False, True], ids=["small", "radix"])
@pytest.mark.parametrize("name", list(VIEWS))
def test_views_of_the_small_shapes_on_both_paths(ctx, comm, shapes, name, radix):
    """every key source ascending and descending, two- and four-key orders, ties across segments decided by `first`, each leaf kind, an
    average, a program with OR and NOT, limits of 1, = kept, > kept and none, a limit without an order, the empty view: the
    one-work-group launch and (TV_GROUP_ORDER_RADIX) the radix path give the reference's bytes"""
    shape = shapes[name]
    assert 0 < shape.merged[1].size <= native.GROUP_ORDER_SMALL_MAX
    ctx.set_tuning(native.TV_GROUP_ORDER_RADIX if radix else 0, 0)
    try:
        run_views(comm, shape, VIEWS[name], name)
        # limit = kept and kept + 1 under a filter: neither cuts, so the radix path sorts every kept group; the path as the device reports it
        kept = reference_view(shape.merged, shape.group, shape.aggs, leaves=[(CNT, 0, GT, 2)], prog=[0])[5]
        assert kept > 0
        for lim in (kept, kept + 1):
            v = view([(AGG, 0, 1)], [(CNT, 0, GT, 2)], [0], lim)
            assert_view(comm.merge_groups_view(shape.queries, shape.seg_index, **v), reference_view(shape.merged, shape.group, shape.aggs, **v), (name, v))
            assert comm.merge_view_path() == (FULL if radix else SMALL), (name, v, comm.merge_view_path())
    finally:
        ctx.set_tuning(0, 0)


def test_the_empty_view_equals_merge_groups_wide(comm, shapes):
    for name, shape in shapes.items():
        got = comm.merge_groups_view(shape.queries, shape.seg_index)
        for i in range(4):
            assert np.array_equal(got[i], shape.merged[i]) and got[i].dtype == shape.merged[i].dtype, (name, i)
        assert sorted(got[4]) == sorted(shape.merged[4]) and all(np.array_equal(got[4][j], shape.merged[4][j]) for j in got[4]), name
        assert got[5] == shape.merged[1].size
        assert np.all(np.diff(got[1].astype(np.int64)) > 0)                          # first-arrival order, from the device
    # ties across segments: MAX(k8) has 4 values over ~600 groups, and within each value `first` ascends over more than one segment
    s = shapes["kid/A"]
    got = comm.merge_groups_view(s.queries, s.seg_index, order=[(AGG, 2, 0)])
    spans = []
    for v in np.unique(got[3][:, 2]):
        f = got[1][got[3][:, 2] == v].astype(np.int64)
        assert np.all(np.diff(f) > 0), v
        spans.append(len(set((f >> 32).tolist())))
    assert max(spans) > 1, spans


def test_max_groups_below_the_view(comm, shapes):
    s = shapes["kid/A"]
    v = view([(AGG, 3, 1)], [L_SUM], [0])
    want = reference_view(s.merged, s.group, s.aggs, **v)
    assert want[5] > 3
    got = comm.merge_groups_view(s.queries, s.seg_index, max_groups=3, **v)
    assert_view(got, tuple(w[:3] for w in want[:4]) + ({j: b[:3] for j, b in want[4].items()}, want[5]), "max_groups = 3")


def test_a_table_query_mixed_with_a_segment_query(ctx, comm, segs):
    table = native.DeviceTable(ctx, segs[:2])
    queries = [agg_query(ctx, table, [], G_KID, AGGS_A), agg_query(ctx, segs[2], [], G_KID, AGGS_A)]
    seg_index = [5, 300]
    merged = comm.merge_groups_wide(queries, seg_index)
    for v in (view([(AGG, 0, 1), (GCOL, 0, 0)], limit=12), view([(AGG, 2, 0)], [L_SUM], [0]), view()):
        assert_view(comm.merge_groups_view(queries, seg_index, **v), reference_view(merged, G_KID, AGGS_A, **v), ("table + segment", v))
    for q in queries:
        q.close()
    table.close()


@pytest.fixture(scope="module")
def dense(ctx, comm):
    """segments whose kid values are distinct: 2048 in one; 2049 with the second; 5000 over two of 3000 that share 1000"""
    rng = np.random.default_rng(2111)
    kids = [np.arange(2048), np.arange(1000, 2049), rng.permutation(3000) * 3 - 4000, (rng.permutation(3000) + 2000) * 3 - 4000]
    out_segs = [native.DeviceSegment(ctx, [c.native() for c in columns(rng, k.size, k)]) for k in kids]
    queries = [agg_query(ctx, s, [], G_KID, AGGS_A) for s in out_segs]
    yield queries
    for q in queries:
        q.close()
    for s in out_segs:
        s.close()


def test_2048_and_2049_merged_groups_take_the_two_paths(comm, dense):
    views = [view([(AGG, 3, 1)], limit=10), view([(AGG, 1, 0)], [L_SUM], [0]), view()]
    for queries, seg_index, n, path in ((dense[:1], [3], 2048, SMALL), (dense[:2], [3, 260], 2049, None)):
        merged = comm.merge_groups_wide(queries, seg_index)
        assert merged[1].size == n
        for v in views:
            assert_view(comm.merge_groups_view(queries, seg_index, **v), reference_view(merged, G_KID, AGGS_A, **v), (n, v))
            assert comm.merge_view_path() == (path if path is not None else (SELECT if v["limit"] else FULL)), (n, v, comm.merge_view_path())


def test_5000_groups_over_two_segments_select_full_sort_and_filter(comm, dense):
    queries, seg_index = dense[2:], [1, 0]
    merged = comm.merge_groups_wide(queries, seg_index)
    assert merged[1].size == 5000
    half = reference_view(merged, G_KID, AGGS_A, leaves=[L_SUM], prog=[0])[5]
    assert 1500 < half < 3500                                                          # the filter keeps about half
    for v, path in ((view([(AGG, 1, 1), (GCOL, 0, 0)], limit=10), SELECT), (view([(AGG, 3, 1)], limit=4000), FULL), (view([(GCOL, 0, 1)], [L_SUM], [0]), FULL),
                    (view([(AGG, 1, 0)], [L_SUM], [0], 10), SELECT), (view(leaves=[L_SUM], prog=[0], limit=3000), FULL)):
        assert_view(comm.merge_groups_view(queries, seg_index, **v), reference_view(merged, G_KID, AGGS_A, **v), v)
        assert comm.merge_view_path() == path, (v, comm.merge_view_path())


def test_refusals_and_argument_errors(ctx, comm, segs, shapes):
    s = shapes["name/B one query"]
    with pytest.raises(native.Imm3Error) as e:                    # a 12-byte key and one byte of segment: 12 + 1 + 4 > 16
        comm.merge_groups_view(s.queries, [1], order=[(GCOL, 0, 0)])
    assert e.value.code == native.ERR_ARG and e.value.msg.startswith(native.MERGE_VIEW_REFUSED), e.value.msg
    assert comm.merge_view_path() == native.GROUP_ORDER_NONE
    assert comm.merge_groups_view(s.queries, [0], order=[(GCOL, 0, 0)])[1].size == s.merged[1].size      # ... and none fits
    # plain argument errors: a key index out of range, an unknown key kind (the ABI has no way to name an average as a key: the engine
    # refuses that before any call), a leaf on a string MAX
    for kw in (dict(order=[(GCOL, 5, 0)]), dict(order=[(2, 0, 0)]), dict(leaves=[(3, 0, GT, 0)], prog=[0]), dict(leaves=[(0, 1, GT, 0)], prog=[0])):
        with pytest.raises(native.Imm3Error) as e:
            comm.merge_groups_view(s.queries, [0], **kw)
        assert e.value.code == native.ERR_ARG and not e.value.msg.startswith(native.MERGE_VIEW_REFUSED), (kw, e.value.msg)
    unrun = agg_query(ctx, segs[0], [], G_NAME, AGGS_B, run=False)
    with pytest.raises(native.Imm3Error) as e:
        comm.merge_groups_view([unrun], [0], order=[(AGG, 0, 0)])
    assert e.value.code == native.ERR_STATE
    unrun.close()
    assert_view(comm.merge_groups_view(s.queries, [0], limit=2), reference_view(s.merged, s.group, s.aggs, limit=2), "after the errors")


def test_the_all_flavour_over_two_contexts_on_one_device(ctx, comm, segs):
    """the single-process flavour finishes on the host under the same rule: three views against the reference"""
    ctx2 = native.Context(0)
    comm2 = native.Comm(ctx2, 1, 0, native.comm_unique_id())
    rng = np.random.default_rng(2110)
    segs2 = [native.DeviceSegment(ctx2, [c.native() for c in columns(rng, n)]) for n in SIZES][:2]
    q1 = [agg_query(ctx, segs[0], [], G_KID, AGGS_A), agg_query(ctx, segs[2], [], G_KID, AGGS_A)]
    q2 = [agg_query(ctx2, segs2[1], [], G_KID, AGGS_A)]
    idx = [[7, 2], [300]]
    merged = native.Comm.merge_groups_wide_all([comm, comm2], [q1, q2], idx)
    for v in (view([(AGG, 2, 1), (AGG, 0, 0)], limit=9), view([(AGG, 3, 0)], [L_SUM, L_MAX], [0, 1, OR]), view()):
        got = native.Comm.merge_groups_view_all([comm, comm2], [q1, q2], idx, **v)
        assert_view(got, reference_view(merged, G_KID, AGGS_A, **v), ("_all", v))
    for q in q1 + q2:
        q.close()
    for s in segs2:
        s.close()
    comm2.close()
    ctx2.close()
