"""GPU suite: imm3_int_set_create -- the set of the distinct values a column takes among the rows a query selects, built on the
device (csrc/imm3_intset.hip) -- against numpy.unique over the same rows: uniform, ragged and table sources, a select tree, two
sources, the sources whose bitmap is not current (count-only, a limit scan that stopped early, never run), the host route (both
int32 extremes present), values that all share one home slot, the overflow of a lowered cap, and every error of the call."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, PforColumn, RawColumn, blocks_of
from immutable3_amd import native
import int_in_util as U

pytestmark = pytest.mark.gpu
INT32_MIN, INT32_MAX = U.INT32_MIN, U.INT32_MAX


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def int_segment(ctx, ids, age, block_rows):
    cols = [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows)]
    return native.DeviceSegment(ctx, [c.native() for c in cols])


def check_set(s, selected_values, what):
    """values(), info() and the table itself against numpy.unique of the selected rows' values"""
    want = np.unique(np.asarray(selected_values).astype(np.int64))
    got = s.values()
    assert got.dtype == np.int32 and got.tolist() == want.tolist(), what
    n, lo, hi, form = s.info()
    assert n == want.size and form == native.plan_int_list_form(4, want.size), what
    assert (lo, hi) == ((int(want[0]), int(want[-1])) if want.size else (0, 0)), what
    slots, empty, max_probe, set256, _ = s.table()
    if want.size == 0:
        assert slots.size == 0 and not set256.any(), what
        return
    assert slots.size == U.slots_for(want.size) and max_probe >= 1 and empty not in set(want.tolist()), what
    assert sorted(int(x) for x in slots if x != empty) == want.tolist(), what          # each value once, nothing else
    for v in want.tolist():                                                          # max_probe bounds every member's distance
        assert native.plan_int_list_probe(slots, empty, max_probe, v) == 1, (what, v)
    for v in (empty, int(want[0]) - 1 if want[0] > INT32_MIN else 5, int(want[-1]) + 1 if want[-1] < INT32_MAX else 6):
        if v not in set(want.tolist()):
            assert native.plan_int_list_probe(slots, empty, max_probe, v) == 0, (what, v)
    bits = [v for v in range(-128, 128) if (int(set256[(v & 255) >> 5]) >> (v & 31)) & 1]
    assert bits == [v for v in want.tolist() if -128 <= v <= 127], what


N1 = 3 * 1024 + 40


def data1(seed=5):
    rng = np.random.default_rng(seed)
    ids = rng.integers(-50, 50, size=N1).astype(np.int32)                      # heavy duplicates, negatives
    ids[rng.integers(0, N1, size=30)] = rng.integers(-(1 << 30), 1 << 30, size=30)
    ids[[3, 1024, N1 - 1]] = [INT32_MIN, INT32_MAX - 1, INT32_MIN]
    age = rng.integers(-128, 128, size=N1).astype(np.int8)
    age[[3, 1024, N1 - 1]] = 100
    return ids, age


def test_one_uniform_segment(ctx):
    """(fails without the feature: the symbols do not exist)"""
    ids, age = data1()
    seg = int_segment(ctx, ids, age, blocks_of(N1, 1024))
    for t in (-129 + 128, 90, 127):                                            # about half the rows, a few, none
        q = native.DeviceQuery(ctx, seg, [1, 0], [(0, GT, float(t))])
        q.run_select()
        s = native.IntSet(ctx, [(q, 1)])
        check_set(s, ids[age > t], ("uniform", t))
        s8 = native.IntSet(ctx, [(q, 0)])                                      # the int8 column itself: sign-extended
        check_set(s8, age[age > t].astype(np.int64), ("uniform int8", t))
        s.close(), s8.close(), q.close()
    seg.close()


def test_ragged_layout(ctx):
    """the same data in batches that end in a word of 40 valid bits: the padding bits contribute nothing"""
    ids, age = data1()
    block_rows = [64 + 40, 1024 + 40, 128 + 40, 64 + 8]
    block_rows.append(N1 - sum(block_rows))
    assert sum(block_rows) == N1 and block_rows[-1] % 64 == 40
    seg = int_segment(ctx, ids, age, block_rows)
    for sels, mask in (([(0, GT, -1.0)], age > -1), ([], np.ones(N1, bool))):   # (no predicate: every bit of every valid row is set)
        q = native.DeviceQuery(ctx, seg, [1, 0], sels)
        q.run_select()
        s = native.IntSet(ctx, [(q, 1)])
        check_set(s, ids[mask], ("ragged", len(sels)))
        s.close(), q.close()
    seg.close()


def test_table_with_a_tree_source(ctx):
    """three segments with partial last tiles; the source is the tree `a or not b`"""
    rng = np.random.default_rng(9)
    cols, dsegs = [], []
    for n in (1024 + 7, 40, 2048):
        ids = rng.integers(-3000, 3000, size=n).astype(np.int32)
        age = rng.integers(-128, 128, size=n).astype(np.int8)
        cols.append((ids, age))
        dsegs.append(int_segment(ctx, ids, age, blocks_of(n, 1024)))
    table = native.DeviceTable(ctx, dsegs)
    ids, age = np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols])
    mask = (ids > 2500) | ~(age < 100)
    q = native.DeviceQuery(ctx, table, [0, 1], [(0, GT, 2500.0), (1, LT, 100.0)], expr=[0, 1, native.EXPR_NOT, native.EXPR_OR])
    q.run_select()
    assert q.count() == int(mask.sum())
    s = native.IntSet(ctx, [(q, 0)])
    check_set(s, ids[mask], "table tree")
    s.close()
    s = native.IntSet(ctx, [(q, 1)])
    check_set(s, age[mask].astype(np.int64), "table tree int8")
    s.close(), q.close(), table.close()
    for d in dsegs:
        d.close()


def test_two_sources_and_a_decoded_column(ctx):
    """the union over two segments and two columns, one int32 (PFOR_INT, filtered on its compressed blocks: read decoded) and one int8"""
    rng = np.random.default_rng(13)
    n1, n2 = 2 * 1024 + 5, 1500
    vals = rng.integers(0, 900, size=n1).astype(np.int32)
    other = rng.integers(-128, 128, size=n1).astype(np.int8)
    pseg = native.DeviceSegment(ctx, [PforColumn(vals, blocks_of(n1, 1024)).native(), RawColumn(DENSE_TINYINT, 1, other, blocks_of(n1, 1024)).native()])
    ids2 = rng.integers(-10, 10, size=n2).astype(np.int32)
    age2 = rng.integers(-128, 128, size=n2).astype(np.int8)
    seg2 = int_segment(ctx, ids2, age2, blocks_of(n2, 1024))
    q1 = native.DeviceQuery(ctx, pseg, [0], [(0, GT, 700.0)])
    q2 = native.DeviceQuery(ctx, seg2, [0, 1], [(0, LT, 0.0)])
    q1.run_select(), q2.run_select()
    s = native.IntSet(ctx, [(q1, 0), (q2, 1)])
    check_set(s, np.concatenate([vals[vals > 700].astype(np.int64), age2[ids2 < 0].astype(np.int64)]), "two sources")
    q1.close(), q2.close()                                                     # sources are not retained
    assert s.info()[0] > 8
    s.close(), pseg.close(), seg2.close()


def test_sources_whose_bitmap_is_not_current(ctx):
    """a source selecting nothing; one whose last run was count-only; one never run; a limit query whose scan stopped early"""
    ids, age = data1(6)
    seg = int_segment(ctx, ids, age, blocks_of(N1, 1024))
    q = native.DeviceQuery(ctx, seg, [0], [(0, GT, 5.0), (0, LT, 5.0)])
    q.run_select()
    s = native.IntSet(ctx, [(q, 0)])
    check_set(s, [], "nothing selected")
    c = native.DeviceQuery(ctx, seg, [0], [(0, native.INT_IN_SET, s)])
    c.run_select()
    assert c.count() == 0 and not c.bitmap().any()
    c.close(), s.close(), q.close()
    q = native.DeviceQuery(ctx, seg, [0, 1], [(1, GT, 0.0)])
    q.run_count()
    assert q.count() == int((age > 0).sum())
    s = native.IntSet(ctx, [(q, 0)])
    check_set(s, ids[age > 0], "count-only")
    s.close(), q.close()
    q = native.DeviceQuery(ctx, seg, [0, 1], [(1, GT, 0.0)])
    s = native.IntSet(ctx, [(q, 0)])
    check_set(s, ids[age > 0], "never run")
    s.close(), q.close(), seg.close()
    n = native.plan_limit_chunks(2048)[0] * 1024 + 1024 + 40                   # more tiles than a limit scan's first chunk
    assert len(native.plan_limit_chunks((n + 1023) // 1024)) >= 2
    rng = np.random.default_rng(8)
    big = rng.integers(0, 200, size=n).astype(np.int32)
    big[-5:] = [7000, 7001, 7002, 7000, -9]                                     # values only the last tile holds
    flag = np.ones(n, np.int8)
    seg = int_segment(ctx, big, flag, blocks_of(n, 1024))
    for limit in (5, 5000):                                                    # the fused limit gather, and the scan in chunks
        q = native.DeviceQuery(ctx, seg, [0, 1], [(1, GT, 0.0)], [0], limit, 1024)
        q.run()
        idx, _ = q.fetch_rows()
        assert idx.tolist() == list(range(limit))
        s = native.IntSet(ctx, [(q, 0)])
        check_set(s, big, ("limit scan", limit))
        assert q.count() == n                                                   # (the whole selection, as imm3_query_bitmap leaves it)
        s.close(), q.close()
    seg.close()


def test_both_extremes_take_the_host_route(ctx):
    ids, age = data1(7)
    ids[[10, 2000]] = [INT32_MAX, INT32_MAX]
    seg = int_segment(ctx, ids, age, blocks_of(N1, 1024))
    q = native.DeviceQuery(ctx, seg, [0], [])
    q.run_select()
    s = native.IntSet(ctx, [(q, 0)])
    assert s.table()[4] is True and s.info()[1:3] == (INT32_MIN, INT32_MAX)
    check_set(s, ids, "both extremes")
    c = native.DeviceQuery(ctx, seg, [0], [(0, native.INT_IN_SET, s), (0, GT, 40.0)])
    c.run_select()
    assert c.count() == int((ids > 40).sum()) and c.bitmap().tolist() == U.bitmap_words(ids > 40, blocks_of(N1, 1024)).tolist()
    c.close(), q.close()
    q = native.DeviceQuery(ctx, seg, [0], [(0, LT, float(INT32_MAX))])          # without INT32_MAX: max + 1 is free, the device route
    q.run_select()
    s2 = native.IntSet(ctx, [(q, 0)])
    assert s2.table()[4] is False
    check_set(s2, ids[ids < INT32_MAX], "one extreme")
    s.close(), s2.close(), q.close(), seg.close()


def test_values_that_share_one_home_slot(ctx):
    """64 values with one home slot in the final table (found by brute force on the CPU): max_probe >= 64 and bounds every member"""
    same = U.same_home_values(64)
    assert len({U.home(v, U.slots_for(64)) for v in same}) == 1
    rng = np.random.default_rng(3)
    n = 2 * 1024 + 9
    ids = rng.choice(np.array(same, dtype=np.int32), size=n)
    ids[:64] = same
    seg = int_segment(ctx, ids, np.zeros(n, np.int8), blocks_of(n, 1024))
    q = native.DeviceQuery(ctx, seg, [0], [])
    q.run_select()
    s = native.IntSet(ctx, [(q, 0)])
    check_set(s, same, "one home slot")
    slots, empty, max_probe, _, _ = s.table()
    assert slots.size == U.slots_for(64) and max_probe >= 64
    outsiders = [v for v in range(same[0], same[-1]) if v not in set(same)][:200]
    for v in outsiders:
        assert native.plan_int_list_probe(slots, empty, max_probe, v) == 0, v
    probe = np.array(same + outsiders, dtype=np.int32)
    pseg = int_segment(ctx, probe, np.zeros(probe.size, np.int8), [probe.size])
    c = native.DeviceQuery(ctx, pseg, [0], [(0, native.INT_IN_SET, s)])
    c.run_select()
    assert c.count() == 64 and c.bitmap().tolist() == U.bitmap_words(U.isin(probe, same), [probe.size]).tolist()
    c.close(), pseg.close(), s.close(), q.close(), seg.close()


def test_overflow_of_a_lowered_cap(ctx):
    """cap 16 against 40 distinct values: IMM3_ERR_ARG, no hang, and the context goes on working"""
    n = 1024 + 300
    ids = (np.arange(n) % 40).astype(np.int32) * 1000
    seg = int_segment(ctx, ids, np.zeros(n, np.int8), blocks_of(n, 1024))
    q = native.DeviceQuery(ctx, seg, [0], [])
    q.run_select()
    for cap in (16, 39):
        with pytest.raises(native.Imm3Error) as e:
            native.IntSet(ctx, [(q, 0)], max_values=cap)
        assert e.value.code == native.ERR_ARG and "too many distinct values" in e.value.msg, e.value.msg
    s = native.IntSet(ctx, [(q, 0)], max_values=40)
    check_set(s, ids, "cap met exactly")
    s.close()
    # thousands of distinct values over 100 k rows against small caps: the running count raises the flag and every walk leaves -- the
    # work is bounded by the cap, not by rows x slots (and a later build on the context is exact)
    big_n = 100 * 1024 + 77
    rng = np.random.default_rng(5)
    wide = rng.integers(-4000, 4000, size=big_n).astype(np.int32)
    bseg = int_segment(ctx, wide, np.zeros(big_n, np.int8), blocks_of(big_n, 1024))
    bq = native.DeviceQuery(ctx, bseg, [0], [])
    bq.run_select()
    distinct = int(np.unique(wide).size)
    assert distinct > 7000
    for cap in (16, 1000, distinct - 1):
        with pytest.raises(native.Imm3Error) as e:
            native.IntSet(ctx, [(bq, 0)], max_values=cap)
        assert e.value.code == native.ERR_ARG and "too many distinct values" in e.value.msg, (cap, e.value.msg)
    s = native.IntSet(ctx, [(bq, 0)], max_values=distinct)
    check_set(s, wide, "the cap met exactly, 100 k rows")
    bq.close(), bseg.close()
    s.close()
    s = native.IntSet(ctx, [(q, 0)])
    check_set(s, ids, "after an overflow")
    s.close(), q.close(), seg.close()


def test_every_error(ctx):
    ids = np.arange(100, dtype=np.int32)
    seg = int_segment(ctx, ids, (ids % 7).astype(np.int8), [100])
    q = native.DeviceQuery(ctx, seg, [0, 1], [(0, GT, 10.0)])
    q.run_select()

    def refused(sources, code, word, **kw):
        with pytest.raises(native.Imm3Error) as e:
            native.IntSet(ctx, sources, **kw)
        assert e.value.code == code and word in e.value.msg, e.value.msg

    refused([], native.ERR_ARG, "n_sources")
    refused([(None, 0)], native.ERR_ARG, "null")
    refused([(q, 0), (None, 0)], native.ERR_ARG, "source 1 is null")
    refused([(q, 2)], native.ERR_ARG, "out of range")
    refused([(q, -1)], native.ERR_ARG, "out of range")
    agg = native.DeviceQuery(ctx, seg, [0, 1], [], (), 0, 1024, group_cols=[1], aggs=[(native.AGG_COUNT, 0)])
    refused([(agg, 0)], native.ERR_ARG, "aggregation")
    agg.close()
    other = native.Context(0)
    oseg = int_segment(other, ids, (ids % 7).astype(np.int8), [100])
    oq = native.DeviceQuery(other, oseg, [0], [])
    refused([(q, 0), (oq, 0)], native.ERR_ARG, "another context")
    oset = native.IntSet(other, [(oq, 0)])
    with pytest.raises(native.Imm3Error) as e:                                  # ... and the leaf takes no set of another context
        native.DeviceQuery(ctx, seg, [0], [(0, native.INT_IN_SET, oset)])
    assert e.value.code == native.ERR_ARG and "another context" in e.value.msg
    oset.close(), oq.close(), oseg.close(), other.close()
    text = np.frombuffer(b"abcdwxyz" * 5, dtype=np.uint8).reshape(10, 4)
    sseg = native.DeviceSegment(ctx, [RawColumn(DENSE_STRING, 4, text, [10]).native()])
    sq = native.DeviceQuery(ctx, sseg, [0], [])
    with pytest.raises(native.Imm3Error) as e:
        native.IntSet(ctx, [(sq, 0)])
    assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    sq.close(), sseg.close()
    refused([(q, 0)], native.ERR_ARG, "cap", max_values=0)
    refused([(q, 0)], native.ERR_ARG, "cap", max_values=native.INT_IN_MAX_VALUES + 1)
    with ctx.capture() as cap:                                                  # no less strict than a creation that uploads a list
        q.run_select()
        with pytest.raises(native.Imm3Error) as e:
            native.IntSet(ctx, [(q, 0)])
        assert e.value.code == native.ERR_STATE and "capture" in e.value.msg
    cap.graph.close()
    s = native.IntSet(ctx, [(q, 0)])
    check_set(s, ids[ids > 10], "after the refusals")
    with pytest.raises(native.Imm3Error) as e:
        load_values = np.zeros(4, np.int32)
        native._check(native.load().imm3_int_set_values(s._h, load_values.ctypes.data, 4))
    assert e.value.code == native.ERR_ARG
    s.close(), q.close(), seg.close()
