"""GPU suite: the IMM3_INT_IN_SET leaf -- membership in a device-built integer set (imm3_int_set_create) -- in every probe form (I8,
ARGS, LDS, GLOBAL): bitmap and count bit-exact against numpy.isin AND against the same query created with IMM3_INT_IN over
set.values(), on a uniform segment with a partial tile, a ragged one (word-at-a-time) and an imm3_table; behind the bitmap (limit,
aggregation, a recorded graph); folding with GT / LT / EQ; the refusals; the set destroyed before the consumer runs; one set shared
by two threads."""
import threading

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_TINYINT, EQ, GT, LT, RawColumn, blocks_of
from immutable3_amd import native
import int_in_util as U

pytestmark = pytest.mark.gpu
INT_IN, INT_IN_SET = native.INT_IN, native.INT_IN_SET
TV_GENERIC_ONLY = 1


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def int_segment(ctx, ids, age, block_rows):
    cols = [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows)]
    return native.DeviceSegment(ctx, [c.native() for c in cols])


def set_of(ctx, values, rows):
    """an IntSet holding exactly `values`, built from a `rows`-row source that selects every row"""
    rng = np.random.default_rng(len(values))
    v = np.array(values, dtype=np.int32)
    ids = np.concatenate([v, rng.choice(v, size=rows - v.size)]) if rows > v.size else v
    ids = ids[rng.permutation(ids.size)]
    seg = int_segment(ctx, ids, np.zeros(ids.size, np.int8), blocks_of(ids.size, 1024))
    q = native.DeviceQuery(ctx, seg, [0], [])
    q.run_select()
    s = native.IntSet(ctx, [(q, 0)])
    q.close(), seg.close()
    return s


@pytest.fixture(scope="module")
def sets(ctx):
    """name -> (IntSet, its values, the form an int32 consumer takes): the forms' sizes come from imm3_plan_int_list_form"""
    rng = np.random.default_rng(41)
    a, l = U.args_largest_n(), U.lds_largest_n()
    assert (a, l) == (8, 4096)
    pool = np.arange(-20_000, 20_000)
    made = {}
    for name, values, rows, form in (
            ("args", [5, -7, 299, 12_345, -20_000], 100, native.INT_LIST_ARGS),
            ("lds 9", rng.choice(pool, size=a + 1, replace=False).tolist(), 1024 + 9, native.INT_LIST_LDS),
            ("lds 4096", rng.choice(pool, size=l, replace=False).tolist(), 5000, native.INT_LIST_LDS),
            ("global", rng.choice(pool, size=l + 1, replace=False).tolist(), 8192, native.INT_LIST_GLOBAL),
            ("i8 small", [-128, 127, 5, 300, -129], 64, native.INT_LIST_ARGS),
            ("i8", [-128, -5, 0, 7, 127, 128, 300, -129, 100_000, 33, 34], 200, native.INT_LIST_LDS)):
        s = set_of(ctx, values, rows)
        assert s.info()[0] == len(values) and s.info()[3] == form == native.plan_int_list_form(4, len(values)), name
        assert s.values().tolist() == sorted(values), name
        made[name] = (s, sorted(values), form)
    yield made
    for s, _, _ in made.values():
        s.close()


N = 3 * 1024 + 17
RAGGED = [64 + 40, 1024, 128 + 40, 5, N - (64 + 1024 + 128 + 2 * 40 + 5)]


def consumer_data():
    rng = np.random.default_rng(42)
    ids = rng.integers(-20_500, 20_500, size=N).astype(np.int32)
    ids[[0, 1023, 1024, N - 1]] = [5, -20_000, 299, 12_345]                    # members in the first rows and the last valid row
    age = rng.integers(-128, 128, size=N).astype(np.int8)
    age[N - 1] = -128
    return ids, age


def run_select(ctx, seg, used, sels, variant=0, expr=None):
    ctx.set_tuning(variant, 0)
    try:
        q = native.DeviceQuery(ctx, seg, used, sels, expr=expr)
        q.run_select()
        out = (q.bitmap(), q.count())
        q.close()
    finally:
        ctx.set_tuning(0, 0)
    return out


def check(ctx, seg, used, leaf_col, s, values, extra, mask, block_rows, what, variants=(0,)):
    """[set leaf + extra] against np.isin's mask and against [IMM3_INT_IN over set.values() + extra]"""
    want = U.bitmap_words(mask, block_rows).tolist()
    for variant in variants:
        w, c = run_select(ctx, seg, used, [(leaf_col, INT_IN_SET, s)] + extra, variant)
        assert c == int(mask.sum()) and w.tolist() == want, (what, variant, c, int(mask.sum()))
        w2, c2 = run_select(ctx, seg, used, [(leaf_col, INT_IN, values)] + extra, variant)
        assert (c2, w2.tolist()) == (c, w.tolist()), (what, variant)


@pytest.mark.parametrize("layout", ["partial tile", "ragged"])
def test_every_form_on_a_segment(ctx, sets, layout):
    """(fails without the feature: cond 8 is an unsupported condition and the set cannot be built)"""
    ids, age = consumer_data()
    block_rows = blocks_of(N, 1024) if layout == "partial tile" else RAGGED
    assert sum(block_rows) == N
    seg = int_segment(ctx, ids, age, block_rows)
    variants = (0, TV_GENERIC_ONLY) if layout == "partial tile" else (0,)       # (a ragged layout IS the word-at-a-time kernel)
    for name, (s, values, form) in sets.items():
        check(ctx, seg, [0], 0, s, values, [], U.isin(ids, values), block_rows, (layout, name, "int32"), variants)
        check(ctx, seg, [1], 0, s, values, [], U.isin(age, values), block_rows, (layout, name, "int8"), variants)   # the I8 form: values outside -128 .. 127 match nothing
    assert U.isin(age, sets["i8"][1]).any() and U.isin(ids, sets["global"][1]).sum() > 100
    seg.close()


def test_every_form_on_a_table(ctx, sets):
    rng = np.random.default_rng(43)
    cols, dsegs = [], []
    for n in (1024 + 7, 40, 2048):
        ids = rng.integers(-20_500, 20_500, size=n).astype(np.int32)
        ids[-1] = 299
        age = rng.integers(-128, 128, size=n).astype(np.int8)
        cols.append((ids, age))
        dsegs.append(int_segment(ctx, ids, age, blocks_of(n, 1024)))
    table = native.DeviceTable(ctx, dsegs)
    for name, (s, values, form) in sets.items():
        for used, ci in (([0], 0), ([1], 1)):
            masks = [U.isin(c[ci], values) for c in cols]
            rows = [(si, int(r)) for si, m in enumerate(masks) for r in np.flatnonzero(m)]
            q = native.DeviceQuery(ctx, table, used, [(0, INT_IN_SET, s)], [0], 0, 1024)
            q.run()
            idx, vals = q.fetch_rows()
            seg_of, row_of = q.locate_rows(idx)
            assert q.count() == len(rows) and list(zip(seg_of.tolist(), row_of.tolist())) == rows, (name, used)
            got = vals[0].view("<i4" if ci == 0 else np.int8).reshape(-1).tolist()
            assert got == [int(cols[si][ci][r]) for si, r in rows], (name, used)
            w2, c2 = run_select(ctx, table, used, [(0, INT_IN, values)])
            assert (c2, w2.tolist()) == (q.count(), q.bitmap().tolist()), (name, used)
            q.close()
    table.close()
    for d in dsegs:
        d.close()


def test_behind_the_bitmap(ctx, sets):
    """projection with a limit, an aggregation, and a consumer's runs recorded in a graph and replayed"""
    ids, age = consumer_data()
    age = (age.astype(np.int32) % 5 - 2).astype(np.int8)
    block_rows = blocks_of(N, 1024)
    seg = int_segment(ctx, ids, age, block_rows)
    s, values, _ = sets["global"]
    used, sels = [0, 1], [(0, INT_IN_SET, s), (1, GT, -2.0)]
    mask = U.isin(ids, values) & (age > -2)
    keep = np.flatnonzero(mask)
    words = U.bitmap_words(mask, block_rows).tolist()
    assert 20 < keep.size < N
    for limit in (0, 7, keep.size):
        q = native.DeviceQuery(ctx, seg, used, sels, [1, 0], limit, 1024)
        q.run()
        idx, vals = q.fetch_rows()
        assert q.count() == keep.size and q.bitmap().tolist() == words
        want = keep[:limit] if limit else keep
        assert idx.tolist() == want.tolist()
        assert vals[0].view(np.int8).reshape(-1).tolist() == age[want].tolist() and vals[1].view("<i4").reshape(-1).tolist() == ids[want].tolist()
        q.close()
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=[1], aggs=[(native.AGG_COUNT, 0), (native.AGG_MAX, 0)])
    q.run()
    keys, first, counts, gvals = q.fetch_groups()
    q.close()
    want = {}
    for r in keep:
        c, m = want.get(int(age[r]), (0, -1 << 40))
        want[int(age[r])] = (c + 1, max(m, int(ids[r])))
    key_of = lambda k: int.from_bytes(bytes([int(k) & 0xFF]), "little", signed=True)
    assert {key_of(k): (int(c), int(v[1])) for k, c, v in zip(keys, counts, gvals)} == want
    q = native.DeviceQuery(ctx, seg, used, sels, [0], 0, 1024)
    q.run()
    q.fetch_rows()
    with ctx.capture() as cap:
        q.run()
    for _ in range(2):
        cap.graph.launch()
        idx, vals = q.fetch_rows()
        assert q.count() == keep.size and q.bitmap().tolist() == words and idx.tolist() == keep.tolist()
        assert vals[0].view("<i4").reshape(-1).tolist() == ids[keep].tolist()
    cap.graph.close()
    q.close()
    seg.close()


def test_folding_with_intervals(ctx, sets):
    ids, age = consumer_data()
    block_rows = blocks_of(N, 1024)
    seg = int_segment(ctx, ids, age, block_rows)
    for name in ("args", "lds 9", "global"):
        s, values, _ = sets[name]
        m = U.isin(ids, values)
        lo, hi, mid = values[0], values[-1], values[len(values) // 2]
        for extra, mask, what in (
                ([(0, GT, float(mid))], m & (ids > mid), "gt"),
                ([(0, LT, float(mid)), (0, GT, float(lo))], m & (ids < mid) & (ids > lo), "gt and lt"),
                ([(0, EQ, float(mid))], ids == mid, "eq a member"),
                ([(0, EQ, float(mid) + 0.0), (0, GT, float(mid))], np.zeros(N, bool), "an empty interval"),
                ([(0, GT, float(hi))], np.zeros(N, bool), "an interval above [min, max]"),
                ([(0, LT, float(lo))], np.zeros(N, bool), "an interval below [min, max]"),
                ([(1, GT, 0.0)], m & (age > 0), "another column")):
            check(ctx, seg, [0, 1], 0, s, values, extra, mask, block_rows, (name, what), (0, TV_GENERIC_ONLY))
    s, values, _ = sets["i8"]
    check(ctx, seg, [1], 0, s, values, [(0, GT, 0.0), (0, LT, 100.0)], U.isin(age, values) & (age > 0) & (age < 100), block_rows, "int8 interval", (0, TV_GENERIC_ONLY))
    check(ctx, seg, [1], 0, sets["lds 9"][0], sets["lds 9"][1], [], np.zeros(N, bool), block_rows, "no int8 value in the set")
    assert not any(-128 <= v <= 127 for v in sets["lds 9"][1])
    seg.close()


def test_refusals(ctx, sets):
    ids, age = consumer_data()
    seg = int_segment(ctx, ids, age, blocks_of(N, 1024))
    s, values, _ = sets["lds 9"]
    small = sets["args"][0]
    one_list = None
    for a_set in (s, small):                                                    # whatever the sizes: the refusal does not depend on data
        for sels in ([(0, INT_IN_SET, a_set), (0, INT_IN, [1, 2])], [(0, INT_IN, []), (0, INT_IN_SET, a_set)],
                     [(0, INT_IN_SET, a_set), (0, INT_IN_SET, s)], [(1, GT, 0.0), (0, INT_IN_SET, a_set), (0, INT_IN_SET, a_set)]):
            with pytest.raises(native.Imm3Error) as e:
                native.DeviceQuery(ctx, seg, [0, 1], sels)
            assert e.value.code == native.ERR_ARG and "takes no other" in e.value.msg, e.value.msg
            one_list = one_list or e.value.msg
            assert e.value.msg == one_list                                      # one fixed message
    q = native.DeviceQuery(ctx, seg, [0, 1], [(0, INT_IN_SET, s), (1, INT_IN, [1, 2, 3])])    # (lists on DIFFERENT columns are fine)
    q.run_select()
    assert q.count() == int((U.isin(ids, values) & U.isin(age, [1, 2, 3])).sum())
    q.close()
    tree = None
    table = native.DeviceTable(ctx, [seg])
    for prog in ([0, 1, native.EXPR_OR], [0, native.EXPR_NOT], [0, 1, native.EXPR_AND, native.EXPR_NOT]):
        for target in (seg, table):                                             # segment and table alike: the _expr and the _table_expr creators
            for aggs in (None, [(native.AGG_COUNT, 0)]):                        # ... and their aggregation forms
                with pytest.raises(native.Imm3Error) as e:
                    native.DeviceQuery(ctx, target, [0, 1], [(0, INT_IN_SET, s), (1, GT, 2.0)], expr=prog, group_cols=[1] if aggs else None, aggs=aggs)
                assert e.value.code == native.ERR_ARG and "IMM3_INT_IN_SET" in e.value.msg and not e.value.msg.startswith(native.TABLE_TREE_REFUSED)
                tree = tree or e.value.msg
                assert e.value.msg == tree
    q = native.DeviceQuery(ctx, table, [0, 1], [(0, INT_IN_SET, s), (1, GT, 1.0)], expr=[0, 1, native.EXPR_AND])   # a table's program of ANDs alone does
    q.run_select()
    assert q.count() == int((U.isin(ids, values) & (age > 1)).sum())
    q.close(), table.close()
    w, c = run_select(ctx, seg, [0, 1], [(0, INT_IN_SET, s), (1, GT, 1.0)], expr=[0, 1, native.EXPR_AND])   # a program of ANDs alone does
    assert c == int((U.isin(ids, values) & (age > 1)).sum())
    for operand, word in ((native.RawIntSet(1, None), "null"), (native.RawIntSet(0, s), "n_match"), (native.RawIntSet(2, s), "n_match")):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, [0], [(0, INT_IN_SET, operand)])
        assert e.value.code == native.ERR_ARG and word in e.value.msg, e.value.msg
    other = native.Context(0)
    oseg = int_segment(other, ids, age, blocks_of(N, 1024))
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(other, oseg, [0], [(0, INT_IN_SET, s)])
    assert e.value.code == native.ERR_ARG and "another context" in e.value.msg
    oseg.close(), other.close()
    seg.close()


def test_the_set_destroyed_before_the_consumer_runs(ctx):
    ids, age = consumer_data()
    block_rows = blocks_of(N, 1024)
    seg = int_segment(ctx, ids, age, block_rows)
    values = sorted(set(ids[::3].tolist()))
    s = set_of(ctx, values, len(values) + 500)
    assert s.info()[0] == len(values) > 8
    q = native.DeviceQuery(ctx, seg, [0], [(0, INT_IN_SET, s)], [0], 0, 1024)
    s.close()
    other = set_of(ctx, list(range(1000, 1000 + len(values))), len(values) + 500)   # (takes what the pool has to give)
    q.run()
    mask = U.isin(ids, values)
    assert q.count() == int(mask.sum()) and q.bitmap().tolist() == U.bitmap_words(mask, block_rows).tolist()
    q.run_select()
    assert q.count() == int(mask.sum())
    other.close(), q.close(), seg.close()


def test_one_set_shared_by_two_threads(ctx, sets):
    ids, age = consumer_data()
    block_rows = blocks_of(N, 1024)
    seg = int_segment(ctx, ids, age, block_rows)
    s, values, _ = sets["global"]
    wants = [U.isin(ids, values) & (ids > 0), U.isin(ids, values) & (age < 0)]
    sels = [[(0, INT_IN_SET, s), (0, GT, 0.0)], [(0, INT_IN_SET, s), (1, LT, 0.0)]]
    errors = []

    def work(k):
        try:
            for _ in range(5):
                q = native.DeviceQuery(ctx, seg, [0, 1], sels[k])
                q.run_select()
                if q.count() != int(wants[k].sum()) or q.bitmap().tolist() != U.bitmap_words(wants[k], block_rows).tolist():
                    errors.append((k, "mismatch"))
                q.close()
        except Exception as exc:                                                 # noqa: BLE001 (reported below, on the main thread)
            errors.append((k, repr(exc)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    seg.close()
