"""GPU suite: ORDER BY over groups (imm3_query_set_group_order; DESIGN.md section 21, "Ordering groups").  Expectations come from numpy:
the group computation of test_gpu_agg_wide_key.expect (first-seen order), then np.lexsort over the normalised key bytes with first_row
last, cut to the limit.  Every case checks all four getters (count, groups, strings, packed keys) and the path the settle took, and --
for group counts the one-work-group launch takes -- that the radix path pinned by tuning variant 25 gives the same bytes."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, PforColumn, RawColumn, SnappyColumn, blocks_of
from immutable3_amd import native
from test_gpu_agg_wide_key import FORMS, STATES, expect, name_pool

pytestmark = pytest.mark.gpu
C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
G, A = native.GROUP_ORDER_GROUP_COL, native.GROUP_ORDER_AGG
SMALL, FULL, SELECT = native.GROUP_ORDER_SMALL, native.GROUP_ORDER_RADIX_FULL, native.GROUP_ORDER_RADIX_SELECT
KMAX = native.GROUP_ORDER_SMALL_MAX
N = 200_000
ID_BASE = 5000          # ids are a permutation of -ID_BASE .. N - ID_BASE - 1: `id < t` selects exactly t + ID_BASE rows, each its own group


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def make_cols(rng, n, br=None):
    """0 id int32 (distinct, negatives), 1 age int8, 2 state 2-byte, 3 name 12-byte string (300 values, 8 bytes shared), 4 k int32 in
    -3 .. 3, 5 v int32 (full range), 6 k8 int8 in -2 .. 1, 7 s4 4-byte string (40 values), 8 t12 12-byte string (random), 9 c int8 = 7"""
    br = br or blocks_of(n, 1024)
    names = name_pool(rng, 300, 12, 8)
    s4 = name_pool(rng, 40, 4)
    return [RawColumn(DENSE_INT, 4, (rng.permutation(n) - ID_BASE).astype(np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(-128, 128, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 2, STATES[rng.integers(0, 51, size=n)], br),
            RawColumn(DENSE_STRING, 12, names[rng.integers(0, names.shape[0], size=n)], br),
            RawColumn(DENSE_INT, 4, rng.integers(-3, 4, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(-2, 2, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 4, s4[rng.integers(0, 40, size=n)], br),
            RawColumn(DENSE_STRING, 12, rng.integers(97, 100, size=(n, 12)).astype(np.uint8), br),
            RawColumn(DENSE_TINYINT, 1, np.full(n, 7, np.int8), br)]


@pytest.fixture(scope="module")
def data(ctx):
    cols = make_cols(np.random.default_rng(20), N)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    yield cols, seg
    seg.close()


def be_bytes(v, nbytes):
    """uint8[g, nbytes]: the low nbytes of the uint64s v, big-endian"""
    v = np.asarray(v, np.uint64)
    return np.stack([(v >> np.uint64(8 * (nbytes - 1 - b))).astype(np.uint8) for b in range(nbytes)], axis=1) if v.size else np.zeros((0, nbytes), np.uint8)


def is_int32(col):
    return np.asarray(col.values).dtype == np.int32      # (DENSE_INT, PFOR_INT and snappy int columns alike)


def is_int8(col):
    return np.asarray(col.values).dtype == np.int8


def normal_keys(cols, group, aggs, exp, order):
    """uint8[g, key bytes]: the normalised key of every expected group (imm3.h's table), first_row behind the user's bytes"""
    _, first, counts, vals, strs, kb = exp
    parts = []
    for (kind, index, desc) in order:
        if kind == G:
            col = cols[group[index]]
            off = sum(cols[g].width for g in group[:index])
            raw = kb[:, off: off + col.width]
            if is_int32(col):
                b = be_bytes(np.ascontiguousarray(raw).view("<u4").reshape(-1).astype(np.uint64) ^ np.uint64(0x80000000), 4)
            elif is_int8(col):
                b = raw ^ np.uint8(0x80)
            else:
                b = raw
        else:
            akind, c = aggs[index]
            col = cols[c]
            if akind == C:
                b = be_bytes(counts, 5)
            elif akind == S:
                b = be_bytes(vals[:, index].astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63), 8)
            elif is_int32(col):
                b = be_bytes((vals[:, index].astype(np.int64).view(np.uint64) & np.uint64(0xFFFFFFFF)) ^ np.uint64(0x80000000), 4)
            elif is_int8(col):
                b = be_bytes((vals[:, index].astype(np.int64).view(np.uint64) & np.uint64(0xFF)) ^ np.uint64(0x80), 1)
            else:
                b = strs[index]
        parts.append(np.uint8(255) - b if desc else b)
    parts.append(be_bytes(first, 4))
    return np.concatenate([np.asarray(p, np.uint8).reshape(first.size, -1) for p in parts], axis=1)


def ordered_expect(cols, group, aggs, mask, order, limit):
    exp = expect(cols, group, aggs, mask)
    if order and exp[1].size:
        nk = normal_keys(cols, group, aggs, exp, order)
        perm = np.lexsort(tuple(nk[:, b] for b in range(nk.shape[1] - 1, -1, -1)))
    else:
        perm = np.arange(exp[1].size)
    if limit > 0:
        perm = perm[:limit]
    keys, first, counts, vals, strs, kb = exp
    return keys[perm], first[perm], counts[perm], vals[perm], {j: s[perm] for j, s in strs.items()}, kb[perm]


def fetch_all(q, seg, used, aggs):
    """(prefix keys, first, counts, vals, {j: strings}, key bytes) through all four getters"""
    keys, first, counts, vals = q.fetch_groups()
    strs = {j: q.fetch_group_strings(j) for j, (k, c) in enumerate(aggs) if k == MX and seg.codecs[used[c]] == DENSE_STRING}
    kb = q.fetch_group_keys()
    n = np.zeros(1, np.uint32)
    native._check(native.load().imm3_query_group_count(q._h, n.ctypes.data_as(native.C.POINTER(native.C.c_uint32))))
    assert int(n[0]) == first.size == kb.shape[0]
    return keys, first, counts, vals, strs, kb


def assert_same(got, want, what=None):
    keys, first, counts, vals, strs, kb = got
    wk, wf, wc, wv, ws, wkb = want
    assert first.tolist() == wf.tolist(), what
    assert kb.shape == wkb.shape and np.array_equal(kb, wkb), what
    assert keys.tolist() == wk.tolist(), what
    assert counts.tolist() == wc.tolist(), what
    assert vals.tolist() == wv.tolist(), what
    assert sorted(strs) == sorted(ws), what
    for j in ws:
        assert strs[j].shape == ws[j].shape and np.array_equal(strs[j], ws[j]), (what, j)


def ordered_both_paths(ctx, cols, seg, used, sels, mask, group, aggs, order, limit=0, wide=True, expr=None, want=None):
    """One query, ordered after its run: the default path against numpy, then -- when that was the small launch -- the radix path pinned
    on the same groups, byte for byte.  -> (path, result)"""
    want = want or ordered_expect(cols, group, aggs, mask, order, limit)
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=wide, expr=expr)
    try:
        q.run()
        assert q.group_order_path() == native.GROUP_ORDER_NONE
        q.set_group_order(order, limit)
        got = fetch_all(q, seg, used, aggs)
        path = q.group_order_path()
        assert_same(got, want, (group, aggs, order, limit, "default path"))
        if path == SMALL:
            ctx.set_tuning(native.TV_GROUP_ORDER_RADIX, 0)
            try:
                q.set_group_order(order, limit)          # (a change of order: the view is made again, now by the pinned path)
                radix = fetch_all(q, seg, used, aggs)
                assert q.group_order_path() in (FULL, SELECT)
            finally:
                ctx.set_tuning(0, 0)
            assert_same(radix, got, (group, aggs, order, limit, "radix against small"))
        return path, got
    finally:
        q.close()


# ---- 1. group counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [0, 1, 2, 51, 64, 65, 1500, KMAX, KMAX + 1, 70_000])
def test_group_counts(ctx, data, n_groups):
    """group by id under `id < t`: exactly n_groups groups of one row.  age_max descending has ~n / 256 ties per value, which must stay in
    first-seen order; v_min ascending is all but unique."""
    cols, seg = data
    used = list(range(len(cols)))
    t = n_groups - ID_BASE
    sels, mask = [(0, LT, float(t))], cols[0].values < t
    assert int(mask.sum()) == n_groups
    aggs = [(C, 0), (MX, 1), (MN, 5)]
    for order in ([(A, 1, True)], [(A, 2, False)], [(G, 0, True)]):
        path, _ = ordered_both_paths(ctx, cols, seg, used, sels, mask, [0], aggs, order)
        assert path == (SMALL if n_groups <= KMAX else FULL), (n_groups, order)


# ---- 2. key kinds ----------------------------------------------------------------------------------------------------------------
KINDS = [
    ("int32 group column, negatives", [4], [(C, 0)], [(G, 0, True)]),
    ("int32 group column ascending", [4], [(C, 0)], [(G, 0, False)]),
    ("int8 group column", [6], [(C, 0)], [(G, 0, False)]),
    ("int8 group column descending", [6], [(C, 0)], [(G, 0, True)]),
    ("string(2) group column", [2], [(C, 0)], [(G, 0, True)]),
    ("12-byte string group column (wide key)", [3], [(C, 0), (MX, 1)], [(G, 0, False)]),
    ("12-byte string group column descending", [3], [(C, 0), (MX, 1)], [(G, 0, True)]),
    ("count", [2], [(MX, 1), (C, 0)], [(A, 1, True)]),
    ("min on int32", [2], [(MN, 5), (MX, 5)], [(A, 0, False)]),
    ("max on int32 descending", [2], [(MN, 5), (MX, 5)], [(A, 1, True)]),
    ("max on int8", [4, 6], [(MX, 1), (MN, 1)], [(A, 0, True)]),
    ("min on int8", [4, 6], [(MX, 1), (MN, 1)], [(A, 1, False)]),
    ("sum with negative totals", [2], [(S, 5), (C, 0)], [(A, 0, False)]),
    ("sum descending", [2], [(S, 5), (C, 0)], [(A, 0, True)]),
    ("max on a 4-byte string", [2], [(C, 0), (MX, 7)], [(A, 1, True)]),
    ("max on a 12-byte string (chunked)", [2], [(MX, 8), (C, 0)], [(A, 0, False)]),
    ("max on a 12-byte string, wide key too", [3], [(MX, 8)], [(A, 0, True)]),
    ("two keys", [2, 6], [(C, 0)], [(G, 1, True), (A, 0, False)]),
    ("three keys of mixed direction", [2, 6], [(C, 0), (MX, 1)], [(G, 1, True), (A, 1, False), (G, 0, True)]),
    ("four keys, 12 bytes", [2, 6], [(C, 0), (MX, 5)], [(G, 1, False), (A, 1, True), (G, 0, False), (A, 0, True)]),
    ("a descending key with many ties", [2], [(MX, 6), (C, 0)], [(A, 0, True)]),
    ("every user key equal: first-seen order", [2], [(MX, 9), (C, 0)], [(A, 0, True)]),
]


@pytest.mark.parametrize("what,group,aggs,order", KINDS, ids=[k[0] for k in KINDS])
def test_key_kinds(ctx, data, what, group, aggs, order):
    cols, seg = data
    used = list(range(len(cols)))
    age = cols[1].values
    for sels, mask in (([], np.ones(N, bool)), ([(1, GT, 100.0), (1, LT, 104.0)], (age > 100) & (age < 104))):
        path, got = ordered_both_paths(ctx, cols, seg, used, sels, mask, group, aggs, order)
        assert path == SMALL
        if what.startswith("every user key equal"):
            assert np.all(np.diff(got[1].astype(np.int64)) > 0)


@pytest.mark.parametrize("codec", ["pfor", "snappy"])
def test_compressed_int_columns_order_as_dense_ones(ctx, codec):
    """a PFOR_INT / snappy int column as group column and under MIN / MAX / SUM: the keys are built from the decoded values"""
    rng = np.random.default_rng(6 if codec == "pfor" else 7)
    n = 20_000
    br = blocks_of(n, 1024)
    cols = make_cols(rng, n, br)
    k = np.sort(rng.integers(-20, 20, size=n)).astype(np.int32)     # sorted: PFOR blocks with few bits
    v = np.sort(rng.integers(-1000, 1000, size=n)).astype(np.int32)
    cols[4] = PforColumn(k, br) if codec == "pfor" else SnappyColumn(DENSE_INT, 4, k, br)
    cols[5] = PforColumn(v, br) if codec == "pfor" else SnappyColumn(DENSE_INT, 4, v, br)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used = list(range(len(cols)))
    try:
        for order in ([(G, 0, True)], [(A, 0, False), (G, 0, False)], [(A, 1, True)], [(A, 2, True)]):
            ordered_both_paths(ctx, cols, seg, used, [], np.ones(n, bool), [4], [(MN, 5), (MX, 5), (S, 5)], order)
    finally:
        seg.close()


# ---- 3. limits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 10, 50, 51, 52, 1000])
def test_limits_small(ctx, data, limit):
    cols, seg = data
    used = list(range(len(cols)))
    path, got = ordered_both_paths(ctx, cols, seg, used, [], np.ones(N, bool), [2], [(C, 0), (MX, 1)], [(A, 0, True), (G, 0, False)], limit)
    assert path == SMALL and got[1].size == min(51, limit)


def test_limit_takes_the_select_on_the_radix_path(ctx, data):
    """70 000 groups, limit 10: the device takes the radix select (groups >= 4 x limit); the pinned full sort's prefix is the same; a
    limit of half the groups sorts everything."""
    cols, seg = data
    used = list(range(len(cols)))
    n_groups = 70_000
    t = n_groups - ID_BASE
    sels, mask = [(0, LT, float(t))], cols[0].values < t
    aggs, order = [(MX, 1), (S, 5)], [(A, 0, True), (A, 1, False)]
    want = ordered_expect(cols, [0], aggs, mask, order, 10)
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=[0], aggs=aggs, wide_keys=True)
    try:
        q.run()
        q.set_group_order(order, 10)
        sel = fetch_all(q, seg, used, aggs)
        assert q.group_order_path() == SELECT
        assert_same(sel, want, "select")
        ctx.set_tuning(native.TV_ORDER_FULL_SORT, 0)
        try:
            q.set_group_order(order, 10)
            full = fetch_all(q, seg, used, aggs)
            assert q.group_order_path() == FULL
        finally:
            ctx.set_tuning(0, 0)
        assert_same(full, sel, "full sort's prefix")
        q.set_group_order(order, n_groups // 2)
        half = fetch_all(q, seg, used, aggs)
        assert q.group_order_path() == FULL
        assert_same(half, ordered_expect(cols, [0], aggs, mask, order, n_groups // 2), "half")
    finally:
        q.close()


# ---- 4. aggregation forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_every_aggregation_form_gives_the_same_order(ctx, data, form):
    cols, seg = data
    used = list(range(len(cols)))
    group, aggs, order = [2], [(C, 0), (MX, 1), (S, 5)], [(A, 1, True), (A, 0, True)]
    want = ordered_expect(cols, group, aggs, np.ones(N, bool), order, 0)
    q = native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=group, aggs=aggs)
    try:
        ctx.set_tuning(100 + form, 0)
        try:
            q.run()
        finally:
            ctx.set_tuning(0, 0)
        q.set_group_order(order, 0)
        assert_same(fetch_all(q, seg, used, aggs), want, form)
        assert q.group_order_path() == SMALL
    finally:
        q.close()


# ---- 5. creators -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table3(ctx):
    """three segments of 3072 / 2048 / 1500 rows (virtual row == row of the concatenation); few k / state values: ties across segments"""
    rng = np.random.default_rng(21)
    parts = [make_cols(rng, n) for n in (3072, 2048, 1500)]
    segs = [native.DeviceSegment(ctx, [c.native() for c in p]) for p in parts]
    table = native.DeviceTable(ctx, segs)
    n = sum(p[0].values.shape[0] for p in parts)
    whole = [RawColumn(p0.codec, p0.width, np.concatenate([p[i].values for p in parts]), blocks_of(n, 1024)) for i, p0 in enumerate(parts[0])]
    yield whole, table, n
    table.close()
    for s in segs:
        s.close()


def test_table_query_ties_across_segments(ctx, table3):
    cols, table, n = table3
    used = list(range(len(cols)))
    for group, aggs, order in (([4], [(C, 0), (MX, 6)], [(A, 1, True)]), ([2], [(MX, 6), (C, 0)], [(A, 0, False)]), ([3], [(MX, 6)], [(A, 0, True)])):
        path, got = ordered_both_paths(ctx, cols, table, used, [], np.ones(n, bool), group, aggs, order)
        assert path == SMALL
    path, _ = ordered_both_paths(ctx, cols, table, used, [], np.ones(n, bool), [2], [(C, 0)], [(A, 0, True)], limit=7)
    assert path == SMALL


def test_expr_queries_with_an_or(ctx, data, table3):
    cols, seg = data
    used = list(range(len(cols)))
    leaves, prog = [(1, LT, -100.0), (1, GT, 100.0)], [0, 1, native.EXPR_OR]
    age = cols[1].values
    ordered_both_paths(ctx, cols, seg, used, leaves, (age < -100) | (age > 100), [2], [(C, 0), (MN, 5)], [(A, 0, True), (A, 1, False)], expr=prog)
    tcols, table, n = table3
    age = tcols[1].values
    ordered_both_paths(ctx, tcols, table, used, leaves, (age < -100) | (age > 100), [2], [(C, 0), (MN, 5)], [(A, 1, True)], limit=20, expr=prog)


def test_narrow_creator(ctx, data):
    cols, seg = data
    used = list(range(len(cols)))
    ordered_both_paths(ctx, cols, seg, used, [], np.ones(N, bool), [2, 4], [(C, 0), (S, 1)], [(A, 1, True)], wide=False)


# ---- 6. lifecycle ----------------------------------------------------------------------------------------------------------------
def test_lifecycle(ctx, data):
    cols, seg = data
    used = list(range(len(cols)))
    group, aggs = [2], [(C, 0), (MX, 1), (MX, 7)]
    mask = np.ones(N, bool)
    o1, o2 = [(A, 0, True)], [(G, 0, True)]
    plain = native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    q = native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True)
    try:
        plain.run()
        never = fetch_all(plain, seg, used, aggs)
        q.set_group_order(o1, 5)                      # before the first run: the first settle sizes the dense arrays, then orders
        q.run()
        a = fetch_all(q, seg, used, aggs)
        assert q.group_order_path() == SMALL
        assert_same(a, ordered_expect(cols, group, aggs, mask, o1, 5), "set before the run")
        b = fetch_all(q, seg, used, aggs)             # fetch twice: identical bytes
        assert_same(b, a, "second fetch")
        q.run()                                       # run again: the view is made again, identical
        assert q.group_order_path() == native.GROUP_ORDER_NONE
        assert_same(fetch_all(q, seg, used, aggs), a, "second run")
        q.set_group_order(o2, 0)                      # change the order between fetches
        assert_same(fetch_all(q, seg, used, aggs), ordered_expect(cols, group, aggs, mask, o2, 0), "changed order")
        q.set_group_order([], 3)                      # no keys: first-seen order, as if never ordered (the limit goes with the order)
        assert q.group_order_path() == native.GROUP_ORDER_NONE
        back = fetch_all(q, seg, used, aggs)
        assert_same(back, never, "order removed")
        assert_same(back, ordered_expect(cols, group, aggs, mask, [], 0), "order removed, numpy")
    finally:
        q.close()
        plain.close()


def test_merge_ignores_the_order(ctx, data):
    cols, seg = data
    used = list(range(len(cols)))
    group, aggs = [3], [(C, 0), (MX, 8)]
    qs = [native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=True) for _ in range(2)]
    comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
    try:
        for q in qs:
            q.run()
        qs[1].set_group_order([(A, 0, True)], 4)
        assert qs[1].fetch_groups()[1].size == 4
        plain = comm.merge_groups_wide([qs[0]], [0])
        ordered = comm.merge_groups_wide([qs[1]], [0])
        for x, y in zip(plain[:4], ordered[:4]):
            assert np.array_equal(x, y)
        assert sorted(plain[4]) == sorted(ordered[4]) and all(np.array_equal(plain[4][j], ordered[4][j]) for j in plain[4])
        assert_same(fetch_all(qs[1], seg, used, aggs), ordered_expect(cols, group, aggs, np.ones(N, bool), [(A, 0, True)], 4), "after the merge")
    finally:
        comm.close()
        for q in qs:
            q.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, data):
    cols, seg = data
    used = list(range(len(cols)))
    proj = native.DeviceQuery(ctx, seg, used, [], [0], 0, 1024)
    q = native.DeviceQuery(ctx, seg, used, [], (), 0, 1024, group_cols=[2, 3], aggs=[(C, 0), (MX, 8), (S, 5)], wide_keys=True)

    def refused(query, keys, n_keys=None, frag=""):
        ks = np.array([[k, i, d] for (k, i, d) in keys] or [[0, 0, 0]], np.int32)
        rc = native.load().imm3_query_set_group_order(query._h, ks.ctypes.data, len(keys) if n_keys is None else n_keys, 0)
        msg = native.load().imm3_last_error().decode()
        assert rc == native.ERR_ARG and frag in msg, (rc, msg)

    try:
        refused(proj, [(G, 0, 0)], frag="not an aggregation query")
        refused(q, [(G, 0, 0)], n_keys=-1, frag="n_keys must be 0 .. 4")
        refused(q, [(G, 0, 0), (G, 1, 0), (A, 0, 0), (A, 1, 0), (A, 2, 0)], frag="n_keys must be 0 .. 4")
        refused(q, [(2, 0, 0)], frag="unknown kind 2")
        refused(q, [(G, 2, 0)], frag="names group column 2 of 2")
        refused(q, [(G, -1, 0)], frag="names group column -1 of 2")
        refused(q, [(A, 3, 0)], frag="names aggregate 3 of 3")
        refused(q, [(A, 0, 0), (G, 0, 1), (A, 0, 1)], frag="aggregate 0 is an order key twice")
        refused(q, [(G, 1, 0), (G, 1, 0)], frag="group column 1 is an order key twice")
        refused(q, [(A, 1, 0), (A, 0, 0)], frag="17 bytes wide together, more than 12")          # 12-byte string MAX + count
        refused(q, [(G, 1, 0), (G, 0, 0)], frag="14 bytes wide together, more than 12")          # 12-byte + 2-byte group columns
        q.run()
        assert q.fetch_groups()[1].size > 0                                                       # a refused call left no order behind
        assert q.group_order_path() == native.GROUP_ORDER_NONE
    finally:
        q.close()
        proj.close()


def test_a_16_byte_group_column_cannot_be_a_key(ctx):
    rng = np.random.default_rng(5)
    n = 2048
    br = blocks_of(n, 1024)
    cols = [RawColumn(DENSE_STRING, 16, name_pool(rng, 20, 16)[rng.integers(0, 20, size=n)], br), RawColumn(DENSE_INT, 4, rng.integers(0, 9, size=n).astype(np.int32), br)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    q = native.DeviceQuery(ctx, seg, [0, 1], [], (), 0, 1024, group_cols=[0], aggs=[(C, 1)], wide_keys=True)
    try:
        with pytest.raises(native.Imm3Error) as e:
            q.set_group_order([(G, 0, False)])
        assert e.value.code == native.ERR_ARG and "16 bytes wide, more than 12" in e.value.msg
        q.set_group_order([(A, 0, True)])            # the aggregate of the same query can be
        q.run()
        assert_same(fetch_all(q, seg, [0, 1], [(C, 1)]), ordered_expect(cols, [0], [(C, 1)], np.ones(n, bool), [(A, 0, True)], 0))
    finally:
        q.close()
        seg.close()
