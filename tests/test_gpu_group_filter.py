"""GPU suite: HAVING over groups (imm3_query_set_group_filter; DESIGN.md section 21, "Filtering groups").  The view of the groups is
filter, then order, then limit.  Expectations come from numpy over the raw columns: the group computation of
test_gpu_agg_wide_key.expect (first-seen order), a keep mask from the expected counts and values (Python-int arithmetic for the
average), np.lexsort over the normalised key bytes of the kept groups, the limit.  Every case checks all four getters, the path the
settle took and the device's own counts (group_filter_stats); for group counts the one-work-group launch takes, the radix path pinned
by tuning variant 25 must give the same bytes."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, LT, RawColumn, blocks_of
from immutable3_amd import native
from test_gpu_agg_wide_key import expect, name_pool
from test_gpu_group_order import assert_same, fetch_all, normal_keys

pytestmark = pytest.mark.gpu
C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
G, A = native.GROUP_ORDER_GROUP_COL, native.GROUP_ORDER_AGG
GT_, LT_, EQ_ = native.GT, native.LT, native.EQ
AND, OR, NOT = native.EXPR_AND, native.EXPR_OR, native.EXPR_NOT
CNT = native.GROUP_FILTER_COUNT
NONE, SMALL, FULL, SELECT = native.GROUP_ORDER_NONE, native.GROUP_ORDER_SMALL, native.GROUP_ORDER_RADIX_FULL, native.GROUP_ORDER_RADIX_SELECT
KMAX = native.GROUP_ORDER_SMALL_MAX
N = 40_000
MAXG = 5000
G_BASE = 1000           # the group column holds gid - G_BASE: negatives; `g < d - G_BASE` selects exactly the groups 0 .. d - 1
DISTINCT = [0, 1, 63, 64, 65, 1023, KMAX, KMAX + 1, MAXG]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def make_cols(rng, n, max_groups=MAXG, names=None):
    """0 g int32 (every value of -G_BASE .. max_groups - G_BASE - 1 at least once, 2 .. ~20 rows each), 1 a8 int8 (full range), 2 v
    int32 in -1000 .. 1000, 3 big int32 (full range), 4 id int32, 5 name 16-byte string, 6 t16 16-byte string (random letters)"""
    br = blocks_of(n, 1024)
    gid = np.concatenate([np.arange(n // 2) % max_groups, rng.integers(0, max_groups, size=n - n // 2)])
    gid = gid[rng.permutation(n)]
    names = names if names is not None else name_pool(rng, 300, 16, 8)
    return [RawColumn(DENSE_INT, 4, (gid - G_BASE).astype(np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(-128, 128, size=n).astype(np.int8), br),
            RawColumn(DENSE_INT, 4, rng.integers(-1000, 1001, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, rng.permutation(n).astype(np.int32), br),
            RawColumn(DENSE_STRING, 16, names[gid % names.shape[0]], br),
            RawColumn(DENSE_STRING, 16, rng.integers(97, 100, size=(n, 16)).astype(np.uint8), br)]


@pytest.fixture(scope="module")
def data(ctx):
    cols = make_cols(np.random.default_rng(77), N)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    yield cols, seg
    seg.close()


# ---- the numpy side ----------------------------------------------------------------------------------------------------------------
def leaf_mask(leaf, aggs, exp):
    """bool[g]: one leaf on every expected group, in Python ints"""
    agg, average, cond, value = leaf
    counts, vals = exp[2], exp[3]
    out = np.zeros(counts.size, bool)
    for i in range(counts.size):
        cnt = int(counts[i])
        if agg == CNT or aggs[agg][0] == C:
            lhs, rhs = cnt, int(value)
        elif average:
            lhs, rhs = int(vals[i, agg]), int(value) * cnt
        else:
            lhs, rhs = int(vals[i, agg]), int(value)
        out[i] = lhs > rhs if cond == GT_ else (lhs < rhs if cond == LT_ else lhs == rhs)
    return out


def keep_mask(leaves, prog, aggs, exp):
    if not prog:
        return np.ones(exp[2].size, bool)
    stack = []
    for op in prog:
        if op >= 0:
            stack.append(leaf_mask(leaves[op], aggs, exp))
        elif op == NOT:
            stack.append(~stack.pop())
        else:
            y, x = stack.pop(), stack.pop()
            stack.append(x & y if op == AND else x | y)
    assert len(stack) == 1
    return stack[0]


def view_expect(cols, group, aggs, exp, keep, order, limit):
    """filter, then order, then limit over the expected groups (exp: first-seen order)"""
    keys, first, counts, vals, strs, kb = exp
    idx = np.flatnonzero(keep)
    sub = (keys[idx], first[idx], counts[idx], vals[idx], {j: s[idx] for j, s in strs.items()}, kb[idx])
    if order and idx.size:
        nk = normal_keys(cols, group, aggs, sub, order)
        perm = np.lexsort(tuple(nk[:, b] for b in range(nk.shape[1] - 1, -1, -1)))
    else:
        perm = np.arange(idx.size)
    if order and limit > 0:                               # (the limit belongs to the order)
        perm = perm[:limit]
    return sub[0][perm], sub[1][perm], sub[2][perm], sub[3][perm], {j: s[perm] for j, s in sub[4].items()}, sub[5][perm]


def check_view(ctx, q, seg, used, cols, group, aggs, exp, leaves, prog, order, limit, paths=None, what=None):
    """set the filter and the order, fetch through all four getters, compare with numpy; -> (result, kept)"""
    keep = keep_mask(leaves, prog, aggs, exp)
    want = view_expect(cols, group, aggs, exp, keep, order, limit)
    q.set_group_filter(leaves, prog)
    q.set_group_order(order, limit)
    assert q.group_filter_stats() == (0, 0)               # the view is stale until a getter asks
    got = fetch_all(q, seg, used, aggs)
    assert_same(got, want, (what, leaves, prog, order, limit))
    n_in, kept = exp[2].size, int(keep.sum())
    assert q.group_filter_stats() == ((n_in, kept) if prog else (0, 0)), what
    path = q.group_order_path()
    if prog or order:
        assert path == SMALL if n_in <= KMAX else path in (FULL, SELECT), (what, path)
        if path != SMALL and limit > 0 and order:
            assert path == (SELECT if kept >= 4 * limit else FULL), (what, kept, limit)
    else:
        assert path == NONE
    if paths is not None:
        paths.add(path)
    if path == SMALL:                                      # the same groups through the radix path: the same bytes
        ctx.set_tuning(native.TV_GROUP_ORDER_RADIX, 0)
        try:
            q.set_group_filter(leaves, prog)
            radix = fetch_all(q, seg, used, aggs)
            assert q.group_order_path() in (FULL, SELECT)
            assert q.group_filter_stats() == ((n_in, kept) if prog else (0, 0))
        finally:
            ctx.set_tuning(0, 0)
        assert_same(radix, got, (what, "radix against small"))
    return got, kept


def filters_for(aggs, exp, rng):
    """[(what, leaves, prog)] keeping none, one, about half and all of the expected groups; aggs = [(C, 4), (MN, 1), (MX, 3), (S, 2)]"""
    counts, vals = exp[2], exp[3]
    g = counts.size
    med = lambda x: int(np.sort(x)[x.size // 2]) if x.size else 0
    one_val = int(vals[int(rng.integers(0, g)), 2]) if g else 5
    return [
        ("none: count < 1", [(CNT, 0, LT_, 1)], [0]),
        ("all: not (count < 1)", [(CNT, 0, LT_, 1)], [0, NOT]),
        ("all: sum > -2^62 and count aggregate > 0", [(3, 0, GT_, -2 ** 62), (0, 0, GT_, 0)], [0, 1, AND]),
        ("one: max(big) == a value", [(2, 0, EQ_, one_val)], [0]),
        ("half: sum > median", [(3, 0, GT_, med(vals[:, 3]))], [0]),
        ("half: count aggregate > median count", [(0, 0, GT_, med(counts))], [0]),
        ("half: avg(v) < 0", [(3, 1, LT_, 0)], [0]),
        ("part: avg(v) > -30 and avg(v) < 40", [(3, 1, GT_, -30), (3, 1, LT_, 40)], [0, 1, AND]),
        ("half: min(a8) < median", [(1, 0, LT_, med(vals[:, 1]))], [0]),
        ("half: max(big) > median (int32)", [(2, 0, GT_, med(vals[:, 2]))], [0]),
        ("or and not: min(a8) < -120 or not (count > median) and max(big) < 0",
         [(1, 0, LT_, -120), (CNT, 0, GT_, med(counts)), (2, 0, LT_, 0)], [0, 1, NOT, 2, AND, OR]),
    ]


# ---- 1. group counts x filters x orders x limits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DISTINCT)
def test_distinct_counts(ctx, data, d):
    cols, seg = data
    used = list(range(len(cols)))
    t = d - G_BASE
    sels, mask = [(0, LT, float(t))], cols[0].values < t
    group, aggs = [0], [(C, 4), (MN, 1), (MX, 3), (S, 2)]
    exp = expect(cols, group, aggs, mask)
    assert exp[2].size == d
    rng = np.random.default_rng(d)
    order = [(A, 0, True), (G, 0, False)]                 # count descending (a handful of distinct counts: many ties), then the group column
    paths, kepts = set(), []
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    try:
        q.run()
        for what, leaves, prog in filters_for(aggs, exp, rng):
            _, kept = check_view(ctx, q, seg, used, cols, group, aggs, exp, leaves, prog, [], 0, what=what)
            kepts.append(kept)
            for limit in sorted({0, max(1, kept // 8), max(1, kept - 1), max(1, kept), kept + 3}):
                check_view(ctx, q, seg, used, cols, group, aggs, exp, leaves, prog, order, limit, paths, what)
        assert kepts[0] == 0 and kepts[1] == kepts[2] == d and kepts[3] == min(d, 1)
        if d >= 63:
            assert all(d // 4 < k < 3 * d // 4 for k in (kepts[4], kepts[5], kepts[6], kepts[8], kepts[9])), kepts
        assert paths == ({SMALL} if d <= KMAX else {FULL, SELECT}), paths
    finally:
        q.close()


def test_min_max_on_int8_and_no_count_aggregate(ctx, data):
    """aggregates (max(a8), min(big), sum(v)): no COUNT among them -- IMM3_GROUP_FILTER_COUNT still answers; an int8 MAX with negatives"""
    cols, seg = data
    used = list(range(len(cols)))
    d = 700
    sels, mask = [(0, LT, float(d - G_BASE))], cols[0].values < d - G_BASE
    group, aggs = [0], [(MX, 1), (MN, 3), (S, 2)]
    exp = expect(cols, group, aggs, mask)
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    try:
        q.run()
        for leaves, prog in (([(0, 0, LT_, 100)], [0]), ([(0, 0, EQ_, 127)], [0]), ([(1, 0, LT_, -2 ** 31 + 2 ** 28), (CNT, 0, GT_, 8)], [0, 1, OR]),
                             ([(0, 0, GT_, -129)], [0]), ([(2, 1, EQ_, 0), (2, 0, EQ_, 0)], [0, 1, NOT, OR])):
            check_view(ctx, q, seg, used, cols, group, aggs, exp, leaves, prog, [], 0)
            check_view(ctx, q, seg, used, cols, group, aggs, exp, leaves, prog, [(A, 0, True), (G, 0, True)], 20)
    finally:
        q.close()


# ---- 2. keys and strings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [65, KMAX + 1])
def test_wide_group_key_and_string_max(ctx, d):
    """group by a 16-byte string (d distinct values; the _wide creators) with a numeric filter, and group by int32 with a 16-byte string
    MAX beside the filtered SUM: the packed keys and the exact strings come back filtered and ordered with the rest"""
    rng = np.random.default_rng(1000 + d)
    names = name_pool(rng, d, 16, 8)
    assert names.shape[0] == d
    cols = make_cols(rng, 20_000, max_groups=d, names=names)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    mask = np.ones(20_000, bool)
    try:
        for group, aggs, leaves, prog, order in (
                ([5], [(C, 4), (S, 2)], [(1, 0, GT_, 0)], [0], [(A, 0, True)]),
                ([5], [(C, 4), (S, 2)], [(1, 1, LT_, 5), (CNT, 0, GT_, 2)], [0, 1, AND], [(A, 1, False)]),
                ([0], [(MX, 6), (S, 2), (C, 4)], [(1, 0, LT_, 0)], [0], [(A, 2, True), (G, 0, False)]),
                ([0], [(MX, 6), (S, 2), (C, 4)], [(1, 0, LT_, 0), (2, 0, GT_, 20_000 // d + 2)], [0, 1, OR], [(A, 1, True)])):
            exp = expect(cols, group, aggs, mask)
            assert exp[2].size == d
            q = native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
            try:
                q.run()
                _, kept = check_view(ctx, q, seg, used, cols, group, aggs, exp, leaves, prog, [], 0)
                assert 0 < kept < d
                for limit in (0, 7, kept, kept + 1):
                    check_view(ctx, q, seg, used, cols, group, aggs, exp, leaves, prog, order, limit)
            finally:
                q.close()
    finally:
        seg.close()


# ---- 3. a table ------------------------------------------------------------------------------------------------------------------------
def test_table_of_three_unequal_segments(ctx):
    rng = np.random.default_rng(31)
    parts = [make_cols(rng, n, max_groups=300) for n in (3072, 2048, 1500)]     # every group has rows in every segment
    segs = [native.DeviceSegment(ctx, [c.native() for c in p]) for p in parts]
    table = native.DeviceTable(ctx, segs)
    n = sum(p[0].values.shape[0] for p in parts)
    cols = [RawColumn(p0.codec, p0.width, np.concatenate([p[i].values for p in parts]), blocks_of(n, 1024)) for i, p0 in enumerate(parts[0])]
    used = list(range(len(cols)))
    group, aggs = [0], [(C, 4), (MN, 1), (MX, 3), (S, 2)]
    exp = expect(cols, group, aggs, np.ones(n, bool))
    assert exp[2].size == 300
    q = native.DeviceQuery(ctx, table, used, [], (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    try:
        q.run()
        for what, leaves, prog in filters_for(aggs, exp, rng):
            check_view(ctx, q, table, used, cols, group, aggs, exp, leaves, prog, [], 0, what=what)
            check_view(ctx, q, table, used, cols, group, aggs, exp, leaves, prog, [(A, 0, True), (G, 0, False)], 10, what=what)
    finally:
        q.close()
        table.close()
        for s in segs:
            s.close()


# ---- 4. state --------------------------------------------------------------------------------------------------------------------------
def test_state(ctx, data):
    cols, seg = data
    used = list(range(len(cols)))
    d = 500
    sels, mask = [(0, LT, float(d - G_BASE))], cols[0].values < d - G_BASE
    group, aggs = [0], [(C, 4), (MN, 1), (MX, 3), (S, 2)]
    exp = expect(cols, group, aggs, mask)
    f1, f2 = ([(3, 0, GT_, 0)], [0]), ([(0, 0, GT_, 8), (1, 0, LT_, -100)], [0, 1, OR])
    o1 = [(A, 0, True), (G, 0, False)]

    def want(f, order, limit):
        return view_expect(cols, group, aggs, exp, keep_mask(f[0], f[1], aggs, exp), order, limit)

    plain = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    try:
        plain.run()
        never = fetch_all(plain, seg, used, aggs)
        assert_same(never, want(([], []), [], 0), "the unfiltered getters, the second witness")
        q.run()
        assert_same(fetch_all(q, seg, used, aggs), never, "before any filter")
        q.set_group_filter(*f1)                               # a filter set after the first run
        a = fetch_all(q, seg, used, aggs)
        assert_same(a, want(f1, [], 0), "set after the run")
        assert q.group_order_path() == SMALL and q.group_filter_stats() == (d, a[1].size)
        assert_same(fetch_all(q, seg, used, aggs), a, "second fetch")
        q.set_group_filter(*f2)                               # changed between getters
        assert q.group_filter_stats() == (0, 0) and q.group_order_path() == NONE
        assert_same(fetch_all(q, seg, used, aggs), want(f2, [], 0), "changed")
        q.run()                                               # a run between two getters: the view is built again
        assert q.group_filter_stats() == (0, 0)
        assert_same(fetch_all(q, seg, used, aggs), want(f2, [], 0), "after a run")
        q.set_group_order(o1, 9)                              # the order after the filter ...
        assert_same(fetch_all(q, seg, used, aggs), want(f2, o1, 9), "order after filter")
        q.set_group_filter(*f1)                               # ... and the filter after the order
        assert_same(fetch_all(q, seg, used, aggs), want(f1, o1, 9), "filter after order")
        q.set_group_filter([], [])                            # removed: the ordered view of every group
        assert_same(fetch_all(q, seg, used, aggs), want(([], []), o1, 9), "filter removed, order kept")
        assert q.group_filter_stats() == (0, 0)
        q.set_group_order([], 0)
        assert_same(fetch_all(q, seg, used, aggs), never, "both removed: as never filtered")
        assert q.group_order_path() == NONE
        q.set_group_filter(*f1)
        with ctx.capture() as cap:                            # a recorded graph of the aggregation run, replayed, then filtered getters
            q.run()
        for _ in range(2):
            cap.graph.launch()
            assert_same(fetch_all(q, seg, used, aggs), want(f1, [], 0), "after a graph replay")
            assert q.group_filter_stats() == (d, a[1].size)
        cap.graph.close()
    finally:
        q.close()
        plain.close()


def test_merge_ignores_the_filter(ctx, data):
    cols, seg = data
    used = list(range(len(cols)))
    group, aggs = [0], [(C, 4), (S, 2)]
    sels = [(0, LT, float(400 - G_BASE))]
    qs = [native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs) for _ in range(2)]
    comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
    try:
        for q in qs:
            q.run()
        qs[1].set_group_filter([(1, 0, GT_, 0)], [0])
        assert 0 < qs[1].fetch_groups()[1].size < 400
        plain = comm.merge_groups([qs[0]], [0])
        filtered = comm.merge_groups([qs[1]], [0])
        assert plain[0].size == 400
        for x, y in zip(plain[:4], filtered[:4]):
            assert np.array_equal(x, y)
    finally:
        comm.close()
        for q in qs:
            q.close()


# ---- 5. errors on a live handle --------------------------------------------------------------------------------------------------------
def test_errors(ctx, data):
    cols, seg = data
    used = list(range(len(cols)))
    proj = native.DeviceQuery(ctx, seg, used, [], [0], 0, 1024)
    q = native.DeviceQuery(ctx, seg, used, [(0, LT, float(50 - G_BASE))], (), 0, 1024, group_cols=[0], aggs=[(C, 4), (MX, 6), (S, 2)], wide_keys=True)

    def refused(query, leaves, prog, frag):
        with pytest.raises(native.Imm3Error) as e:
            query.set_group_filter(leaves, prog)
        assert e.value.code == native.ERR_ARG and frag in e.value.msg, e.value.msg

    try:
        refused(proj, [(CNT, 0, GT_, 1)], [0], "not an aggregation query")
        refused(q, [(CNT, 0, GT_, 1)] * 9, [0], "n_leaves must be 0 .. 8")
        refused(q, [(CNT, 0, GT_, 1)], [0] + [0, AND] * 16, "n_prog must be 0 .. 32")
        refused(q, [(CNT, 0, GT_, 1)], [], "empty, but leaves were given")
        refused(q, [(3, 0, GT_, 1)], [0], "names aggregate 3 of 3")
        refused(q, [(1, 0, GT_, 1)], [0], "MAX over a STRING column")
        refused(q, [(0, 1, GT_, 1)], [0], "average is for a SUM aggregate only")
        refused(q, [(2, 1, GT_, 2 ** 31)], [0], "[-2^31, 2^31 - 1]")
        refused(q, [(2, 0, native.MATCH, 1)], [0], "unknown cond")
        refused(q, [(2, 0, GT_, 1)], [0, 0], "more than one result")
        q.run()
        assert q.fetch_groups()[1].size == 50                  # a refused call left no filter behind
        assert q.group_filter_stats() == (0, 0) and q.group_order_path() == NONE
    finally:
        q.close()
        proj.close()
