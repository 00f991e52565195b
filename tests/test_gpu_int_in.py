"""GPU suite: IMM3_INT_IN -- an IN-list on an int32 / int8 column -- through k_filter_int_list (csrc/imm3_intlist.hip: every form, segment
and table instances), the word-at-a-time kernel's probe (ragged layouts, tuning variant 1) and the decoded form of a PFOR_INT column.
Every bitmap, count and projected row is held bit-exact against np.isin over the same rows (tests/int_in_util.py); the thresholds
between the forms are read from imm3_plan_int_list_form."""
import ctypes as C

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, PforColumn, RawColumn, blocks_of
from immutable3_amd import native
import int_in_util as U

pytestmark = pytest.mark.gpu
INT_IN = native.INT_IN
TV_GENERIC_ONLY = 1


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def select(ctx, seg, used, sels, variant=0, expr=None):
    ctx.set_tuning(variant, 0)
    try:
        q = native.DeviceQuery(ctx, seg, used, sels, expr=expr)
        q.run_select()
        out = (q.bitmap(), q.count())
        q.close()
    finally:
        ctx.set_tuning(0, 0)
    return out


def check(ctx, seg, used, sels, mask, block_rows, what, expr=None, variants=(0, TV_GENERIC_ONLY)):
    want = U.bitmap_words(mask, block_rows)
    for variant in variants:
        w, c = select(ctx, seg, used, sels, variant, expr)
        assert c == int(mask.sum()), (what, variant, c, int(mask.sum()))
        assert w.tolist() == want.tolist(), (what, variant)


def int_segment(ctx, ids, age, block_rows):
    cols = [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows)]
    return native.DeviceSegment(ctx, [c.native() for c in cols])


def test_the_leaf_is_accepted_and_checked(ctx):
    """(fails without the feature: cond 7 was an unsupported condition)"""
    ids = np.arange(100, dtype=np.int32)
    seg = int_segment(ctx, ids, (ids % 7).astype(np.int8), [100])
    w, c = select(ctx, seg, [0], [(0, INT_IN, [3, 3, 50, 1000])])
    assert c == 2 and w.tolist() == U.bitmap_words(U.isin(ids, [3, 50]), [100]).tolist()
    assert select(ctx, seg, [0], [(0, INT_IN, [])])[1] == 0                      # an empty list: no row
    for operand, word in ((native.RawIntList(-1, [1]), "negative"), (native.RawIntList(3, None), "null"),
                          (native.RawIntList(native.INT_IN_MAX_VALUES + 1, [1]), "IMM3_INT_IN_MAX_VALUES")):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, [0], [(0, INT_IN, operand)])
        assert e.value.code == native.ERR_ARG and word in e.value.msg, e.value.msg
    for used in ([0], [1]):                                                     # Match on an int column keeps its error
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, used, [(0, MATCH, [b"abcd"])])
        assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    for prog in ([0, 1, native.EXPR_OR], [0, native.EXPR_NOT], [0, 1, native.EXPR_AND, native.EXPR_NOT]):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, [0, 1], [(0, INT_IN, [1, 2]), (1, GT, 2.0)], expr=prog)
        assert e.value.code == native.ERR_ARG and "IMM3_INT_IN" in e.value.msg and not e.value.msg.startswith(native.TABLE_TREE_REFUSED)
    check(ctx, seg, [0, 1], [(0, INT_IN, [1, 2, 9, 10]), (1, GT, 1.0)], U.isin(ids, [1, 2, 9, 10]) & (ids % 7 > 1), [100], "AND program",
          expr=[0, 1, native.EXPR_AND])
    seg.close()
    s = np.frombuffer(b"abcdwxyz" * 5, dtype=np.uint8).reshape(10, 4)
    sseg = native.DeviceSegment(ctx, [RawColumn(DENSE_STRING, 4, s, [10]).native()])
    with pytest.raises(native.Imm3Error) as e:
        native.DeviceQuery(ctx, sseg, [0], [(0, INT_IN, [1])])
    assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    sseg.close()
    empty = native.DeviceSegment(ctx, [RawColumn(DENSE_STRING, 4, np.zeros((0, 4), np.uint8), []).native()])
    native.DeviceQuery(ctx, empty, [0], [(0, INT_IN, [1])]).close()               # no batch: no vector to be of the wrong type
    empty.close()


def lists_for(rng, ids):
    """(values, what) on an int32 column: each form's sizes around its thresholds, present and absent values mixed"""
    a, big = U.args_largest_n(), 300
    out = []
    for n in (1, a, a + 1, big):
        present = rng.choice(ids, size=(n + 1) // 2).tolist()
        absent = rng.integers(-(1 << 31), 1 << 31, size=n - len(present)).tolist()
        out.append((present + absent, f"{n} values"))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17])
def test_segment_sizes(ctx, n):
    rng = np.random.default_rng(n)
    block_rows = blocks_of(n, 1024)
    ids = rng.integers(-40, 40, size=n).astype(np.int32)
    ids[-1] = 7                                                                 # the last valid row of the partial tile is a member
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    age[-1] = -128
    seg = int_segment(ctx, ids, age, block_rows)
    for values, what in lists_for(rng, ids):
        values = values + [7]
        check(ctx, seg, [0], [(0, INT_IN, values)], U.isin(ids, values), block_rows, (n, "int32", what))
    for values in ([-128], [0, 0, 5, 300], list(range(-128, 128, 4)) + [-129]):
        check(ctx, seg, [1], [(0, INT_IN, values)], U.isin(age, values), block_rows, (n, "int8", len(values)))
    seg.close()


N_FORMS = 40_000 + 123


@pytest.fixture(scope="module")
def forms_segment(ctx):
    rng = np.random.default_rng(77)
    block_rows = blocks_of(N_FORMS, 1024)
    ids = rng.integers(-100_000, 100_000, size=N_FORMS).astype(np.int32)
    same = U.same_home_values(12)
    ids[rng.integers(0, N_FORMS, size=400)] = rng.choice(same + [same[-1] + 1, same[0] - 1], size=400)
    ids[[0, 1023, 1024, N_FORMS - 1]] = [-(1 << 31), (1 << 31) - 1, -1, 0]
    age = rng.integers(-128, 128, size=N_FORMS).astype(np.int8)
    seg = int_segment(ctx, ids, age, block_rows)
    yield seg, ids, age, block_rows, same
    seg.close()


def test_int8_forms(ctx, forms_segment):
    seg, ids, age, block_rows, _ = forms_segment
    rng = np.random.default_rng(1)
    assert native.plan_int_list_form(1, 1) == native.plan_int_list_form(1, 256) == native.INT_LIST_I8
    for values, what in (([17], "1"), (rng.permutation(np.arange(-128, 128))[:64].tolist(), "64"), (list(range(-128, 128)), "all 256"),
                         ([-128, 127], "the ends"), ([-128, 127, 128, -129, 1000, -(1 << 31)], "the ends and values no int8 holds"),
                         ([300, -1000], "nothing an int8 holds")):
        mask = U.isin(age, values)
        check(ctx, seg, [1], [(0, INT_IN, values)], mask, block_rows, ("int8", what))
        if what == "all 256":
            assert mask.all()
        if what == "nothing an int8 holds":
            assert not mask.any()


def test_int32_forms(ctx, forms_segment):
    seg, ids, age, block_rows, same = forms_segment
    rng = np.random.default_rng(2)
    a, l = U.args_largest_n(), U.lds_largest_n()
    forms = {}
    cases = [(1, "1"), (a, "args largest"), (a + 1, "args largest + 1"), (l, "lds largest"), (l + 1, "lds largest + 1")]
    for n, what in cases:
        present = np.unique(rng.choice(ids, size=(n + 1) // 2))
        values = set(present.tolist())
        while len(values) < n:                                                  # exactly n distinct values: the form is the one asked for
            values.add(int(rng.integers(-(1 << 31), 1 << 31)))
        values = list(values)
        forms[what] = native.plan_int_list_form(4, len(values))
        mask = U.isin(ids, values)
        assert mask.any() and not mask.all()
        check(ctx, seg, [0], [(0, INT_IN, values)], mask, block_rows, ("int32", what), variants=(0,) if n > a + 1 else (0, TV_GENERIC_ONLY))
    assert forms["args largest"] == native.INT_LIST_ARGS and forms["args largest + 1"] == native.INT_LIST_LDS
    assert forms["lds largest"] == native.INT_LIST_LDS and forms["lds largest + 1"] == native.INT_LIST_GLOBAL
    # the ends of int32, -1 and 0
    ends = [-(1 << 31), (1 << 31) - 1, -1, 0]
    for extra in ([], list(range(5, 25))):
        check(ctx, seg, [0], [(0, INT_IN, ends + extra)], U.isin(ids, ends + extra), block_rows, ("ends", len(extra)))
    # every value shares one home slot: the longest probes the table can hold; neighbours of the values are rows, and no members
    mask = U.isin(ids, same)
    assert mask.any()
    check(ctx, seg, [0], [(0, INT_IN, same)], mask, block_rows, "one home slot")
    # no value occurs in the column (inside its span, so the probe runs); every row is a member
    absent = [v for v in range(-50_000, 50_000, 997) if v not in set(ids.tolist())][:40]
    check(ctx, seg, [0], [(0, INT_IN, absent)], np.zeros(N_FORMS, bool), block_rows, "no value occurs")
    few = np.unique(ids)
    check(ctx, seg, [0], [(0, INT_IN, few.tolist())], np.ones(N_FORMS, bool), block_rows, "every row a member", variants=(0,))


def test_every_row_a_member_small_lists(ctx):
    n, block_rows = 5000, blocks_of(5000, 1024)
    rng = np.random.default_rng(3)
    ids = rng.choice([5, -9, 1 << 20], size=n).astype(np.int32)
    age = rng.choice([-128, 3], size=n).astype(np.int8)
    seg = int_segment(ctx, ids, age, block_rows)
    for values in ([5, -9, 1 << 20], [5, -9, 1 << 20] + list(range(100, 120))):
        check(ctx, seg, [0], [(0, INT_IN, values)], np.ones(n, bool), block_rows, ("all", len(values)))
    check(ctx, seg, [1], [(0, INT_IN, [-128, 3])], np.ones(n, bool), block_rows, "all int8")
    seg.close()


def test_and_existing(ctx, forms_segment):
    seg, ids, age, block_rows, _ = forms_segment
    rng = np.random.default_rng(4)
    values = rng.choice(ids, size=600).tolist()
    ages = [-128, 127, 0, 1, 2, 3, 50]
    m_list, m_age = U.isin(ids, values), U.isin(age, ages)
    # a range on another column first (the tile pass), then the list
    check(ctx, seg, [1, 0], [(0, GT, -5.0), (0, LT, 60.0), (1, INT_IN, values)], (age > -5) & (age < 60) & m_list, block_rows, "range, then list")
    # two lists on two columns
    check(ctx, seg, [0, 1], [(0, INT_IN, values), (1, INT_IN, ages)], m_list & m_age, block_rows, "two lists")
    # list and range on the same column: the folded form; two lists on one column: their intersection
    check(ctx, seg, [0], [(0, INT_IN, values), (0, GT, 0.0), (0, LT, 50_000.0)], m_list & (ids > 0) & (ids < 50_000), block_rows, "list and range")
    half = values[::2] + [123456789]
    check(ctx, seg, [0], [(0, INT_IN, values), (0, INT_IN, half)], U.isin(ids, set(values) & set(half)), block_rows, "two lists, one column")
    check(ctx, seg, [0], [(0, INT_IN, values), (0, GT, 200_000.0)], np.zeros(N_FORMS, bool), block_rows, "list and range that do not meet")
    check(ctx, seg, [1], [(0, INT_IN, ages), (0, GT, 1.0)], m_age & (age > 1), block_rows, "int8 list and range")


def table_of(ctx, sizes, seed):
    rng = np.random.default_rng(seed)
    segs_cols, dsegs = [], []
    for n in sizes:
        br = blocks_of(n, 1024)
        ids = rng.integers(-300, 300, size=n).astype(np.int32)
        age = rng.integers(-128, 128, size=n).astype(np.int8)
        segs_cols.append((ids, age, br))
        dsegs.append(int_segment(ctx, ids, age, br))
    return segs_cols, dsegs, native.DeviceTable(ctx, dsegs)


def test_table_equals_per_segment(ctx):
    """three segments of 1500, 1024 and 7 rows: partial tiles inside the tile table"""
    segs_cols, dsegs, table = table_of(ctx, [1500, 1024, 7], 11)
    rng = np.random.default_rng(12)
    all_ids = np.concatenate([c[0] for c in segs_cols])
    a, l = U.args_largest_n(), U.lds_largest_n()
    cases = [([0], [(0, INT_IN, [5, -7, 299])], "args"), ([0], [(0, INT_IN, rng.choice(all_ids, size=40).tolist())], "lds"),
             ([0], [(0, INT_IN, list(range(-250, -250 + l + 1)))], "global"),
             ([1], [(0, INT_IN, [-128, 127, 5, 300])], "int8"),
             ([1, 0], [(0, GT, 0.0), (1, INT_IN, list(range(-300, 0, 3)))], "range, then list"),
             ([0, 1], [(0, INT_IN, list(range(0, 300, 2))), (1, INT_IN, list(range(-128, 128, 3)))], "two lists")]
    assert native.plan_int_list_form(4, l + 1) == native.INT_LIST_GLOBAL and a >= 3
    for used, sels, what in cases:
        q = native.DeviceQuery(ctx, table, used, sels, [0], 0, 1024)
        q.run()
        words, count = q.bitmap(), q.count()
        idx, vals = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        fb, fw = q.segment_starts()
        total, rows = 0, []
        for si, (ids, age, br) in enumerate(segs_cols):
            w, c = select(ctx, dsegs[si], used, sels)                           # the per-segment query ...
            cols = {0: ids.astype(np.int64), 1: age.astype(np.int64)}
            mask = np.ones(ids.size, bool)
            for (ci, cond, operand) in sels:
                col = cols[used[ci]]
                mask &= U.isin(col, operand) if cond == INT_IN else (col > operand)
            assert c == int(mask.sum()) and w.tolist() == U.bitmap_words(mask, br).tolist(), (what, si)   # ... is np.isin's
            assert words[int(fw[si]): int(fw[si]) + w.size].tolist() == w.tolist(), (what, si)
            assert not words[int(fw[si]) + w.size: int(fw[si + 1])].any(), (what, si)
            total += c
            rows += [(si, int(r)) for r in np.flatnonzero(mask)]
        assert count == total and list(zip(seg_of.tolist(), row_of.tolist())) == rows, what
        first = [segs_cols[s][0 if used[0] == 0 else 1][r] for s, r in rows]
        assert vals[0].view("<i4" if used[0] == 0 else np.int8).reshape(-1).tolist() == [int(x) for x in first], what
        q.close()
    table.close()
    for d in dsegs:
        d.close()


def test_behind_the_bitmap(ctx):
    """a count-only run, projection with a limit, group by with count + max, a recorded graph replayed twice, imm3_query_join_count"""
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(21)
    n, block_rows = 6 * 1024 + 321, blocks_of(6 * 1024 + 321, 1024)
    ids = rng.integers(-500, 500, size=n).astype(np.int32)
    age = rng.integers(-4, 4, size=n).astype(np.int8)
    seg = int_segment(ctx, ids, age, block_rows)
    values = rng.choice(np.arange(-500, 500), size=120, replace=False).tolist()
    used, sels = [0, 1], [(0, INT_IN, values), (1, GT, -3.0)]
    mask = U.isin(ids, values) & (age > -3)
    keep = np.flatnonzero(mask)
    words = U.bitmap_words(mask, block_rows).tolist()
    assert 0 < keep.size < n
    q = native.DeviceQuery(ctx, seg, used, sels)
    q.run_count()
    assert q.count() == keep.size
    q.join_count()
    ctx.sync()
    out = np.zeros(1, np.uint64)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(q.device_ptr(1)), C.c_size_t(8), C.c_int(2)) == 0
    assert int(out[0]) == keep.size
    assert q.bitmap().tolist() == words
    q.close()
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


def test_the_other_routes(ctx):
    """a ragged layout (the word-at-a-time kernel's probe under the default plan too) and a PFOR_INT predicate column (read decoded)"""
    rng = np.random.default_rng(31)
    block_rows = [64, 128, 64, 5, 1000, 3]
    n = sum(block_rows)
    ids = rng.integers(-60, 60, size=n).astype(np.int32)
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    seg = int_segment(ctx, ids, age, block_rows)
    for values in ([3], list(range(-60, 60, 7)), list(range(-60, 60, 2)) + [1 << 30]):
        check(ctx, seg, [0], [(0, INT_IN, values)], U.isin(ids, values), block_rows, ("ragged int32", len(values)))
    check(ctx, seg, [1, 0], [(0, INT_IN, [-128, 127, 9, 200]), (1, GT, -10.0)], U.isin(age, [-128, 127, 9]) & (ids > -10), block_rows, "ragged int8")
    seg.close()
    n, block_rows = 4 * 1024 + 100, blocks_of(4 * 1024 + 100, 1024)
    vals = rng.integers(0, 5000, size=n).astype(np.int32)
    other = rng.integers(-128, 128, size=n).astype(np.int8)
    pseg = native.DeviceSegment(ctx, [PforColumn(vals, block_rows).native(), RawColumn(DENSE_TINYINT, 1, other, block_rows).native()])
    for values in ([vals[5], vals[n - 1], 6000], rng.choice(vals, size=50).tolist()):
        values = [int(v) for v in values]
        mask = U.isin(vals, values)
        check(ctx, pseg, [0, 1], [(0, INT_IN, values)], mask, block_rows, ("pfor", len(values)))
        q = native.DeviceQuery(ctx, pseg, [0, 1], [(0, INT_IN, values), (0, GT, 10.0)], [1], 0, 1024)
        q.run()
        idx, pv = q.fetch_rows()
        q.close()
        keep = np.flatnonzero(mask & (vals > 10))
        assert idx.tolist() == keep.tolist() and pv[0].view(np.int8).reshape(-1).tolist() == other[keep].tolist()
    pseg.close()


def test_fuzz(ctx):
    """200 statements from a fixed seed (tests/int_in_util.py: 1 .. 4 segments of 1 .. 3000 rows, lists of 0 .. 40 values about half of
    them present, further range / Match leaves): per-segment queries under the default plan and the word-at-a-time kernel, and the
    table query, against plain numpy"""
    rng = np.random.default_rng(20260)
    ran = 0
    for k in range(200):
        st = U.draw_statement(rng)
        if U.refused(st):
            continue
        ran += 1
        used_names = list(dict.fromkeys(l[0] for l in st.leaves))
        used = [U.COLS.index(nm) for nm in used_names]
        sels = U.native_sels(st, used_names)
        dsegs, masks = [], []
        for si, (n, br) in enumerate(st.segments):
            ids, age, code = st.cols[si]
            cols = [RawColumn(DENSE_INT, 4, ids, br), RawColumn(DENSE_TINYINT, 1, age, br), RawColumn(DENSE_STRING, 4, code, br)]
            dsegs.append(native.DeviceSegment(ctx, [c.native() for c in cols]))
            masks.append(U.truth(st, si))
            check(ctx, dsegs[-1], used, sels, masks[-1], br, ("fuzz", k, si), variants=(0, TV_GENERIC_ONLY) if k % 4 == 0 else (0,))
        table = native.DeviceTable(ctx, dsegs)
        q = native.DeviceQuery(ctx, table, used, sels, [0], st.limit, 1024)
        q.run()
        idx, vals = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        rows = [(si, int(r)) for si, m in enumerate(masks) for r in np.flatnonzero(m)]
        assert q.count() == len(rows), ("fuzz", k)
        want = rows[:st.limit] if st.limit else rows
        assert list(zip(seg_of.tolist(), row_of.tolist())) == want, ("fuzz", k)
        got = [bytes(v) for v in vals[0]]
        assert got == [st.cols[s][used[0]][r].tobytes() for s, r in want], ("fuzz", k)
        q.close()
        table.close()
        for d in dsegs:
            d.close()
    assert ran >= 180
