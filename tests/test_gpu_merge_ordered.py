"""GPU suite: imm3_comm_merge_ordered on ONE rank (a real native.Comm(ctx, 1, 0, ...)): the ordered results of per-segment and table
queries merged on the device by (normalised key, global segment, row) -- csrc/imm3_merge_order.hip -- against
order_util.expected_table over the segments in global order, and against one ordered imm3_table query over the same segments.
Everything is bit-exact.

Four segments of 1025, 1024, 1 and 700 rows; `age` has three values (ties inside and across segments), `name` five, `tag` is a 5-byte
payload.  The ids of segment s are id_of(v) for a range of v of its own, so an id window leaves a chosen number of rows per segment."""
import numpy as np
import pytest

import merge_order_util as U
from merge_order_util import AGE, ID, NAME, TAG

pytestmark = pytest.mark.gpu
ROWS = [1025, 1024, 1, 700]
FIRST_V = [0, 2000, 5000, 6000]
ALL = U.between(None, 6700)
USED = [ID, AGE, TAG]          # SELECT id, age, tag
PROJ = [0, 1, 2]


class Data:
    def __init__(self):
        from immutable3_amd import native
        self.native = native
        self.ctx = native.Context(0)
        rng = np.random.default_rng(2110)
        self.cols = [U.segment_columns(rng, n, v) for n, v in zip(ROWS, FIRST_V)]
        self.segs = [native.DeviceSegment(self.ctx, [c.native() for c in cols]) for cols in self.cols]
        self.table = native.DeviceTable(self.ctx, self.segs)
        self.comm = native.Comm(self.ctx, 1, 0, native.comm_unique_id())

    def close(self):
        self.comm.close()
        self.table.close()
        for s in self.segs:
            s.close()
        self.ctx.close()

    def queries(self, order, used, sels, proj, order_by, own_limit=0, run=True):
        return [U.ordered_query(self.native, self.ctx, self.segs[s], used, sels, proj, order_by, own_limit, run) for s in order]

    def want(self, used, sels, proj, order_by, limit=0, segments=(0, 1, 2, 3)):
        return U.expected({g: self.cols[g] for g in segments}, used, sels, proj, order_by, limit)

    def merged(self, order, used, sels, proj, order_by, limit=0, own_limit=None, **kw):
        qs = self.queries(order, used, sels, proj, order_by, limit if own_limit is None else own_limit)
        try:
            return self.comm.merge_ordered(qs, list(order), limit, **kw)
        finally:
            for q in qs:
                q.close()

    def table_rows(self, used, sels, proj, order_by, limit=0):
        """one ordered table query over all four segments: (segment, row, columns)"""
        q = U.ordered_query(self.native, self.ctx, self.table, used, sels, proj, order_by, limit)
        idx, vals = q.fetch_rows()
        seg, row = q.locate_rows(idx)
        q.close()
        return seg, row, vals


@pytest.fixture(scope="module")
def d():
    x = Data()
    yield x
    x.close()


# ---- ties by global segment ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [False, True])
def test_ties_come_out_by_global_segment_whatever_the_query_order(d, desc):
    order_by = [(1, desc)]
    want = d.want(USED, ALL, PROJ, order_by)
    assert want[0].size == sum(ROWS)
    got = d.merged([2, 0, 3, 1], USED, ALL, PROJ, order_by)
    U.assert_rows(got, want, "queries in the order [2, 0, 3, 1]")
    U.assert_rows(d.merged([0, 1, 2, 3], USED, ALL, PROJ, order_by), want, "queries in global order")
    U.assert_rows(d.table_rows(USED, ALL, PROJ, order_by), want, "one ordered table query")
    seg, row = got[0].astype(np.int64), got[1].astype(np.int64)
    age = got[2][1].reshape(-1)
    same = age[1:] == age[:-1]                               # inside a tie group (segment, row) ascends
    assert (((seg[1:] > seg[:-1]) | ((seg[1:] == seg[:-1]) & (row[1:] > row[:-1]))) | ~same).all()


# ---- full-width keys ----------------------------------------------------------------------------------------------------
def test_sixteen_key_bytes(d):
    used, proj, order_by = [ID, NAME, TAG], [1, 0, 2], [(0, True), (1, False)]        # SELECT name, id, tag ORDER BY name DESC, id
    want = d.want(used, ALL, proj, order_by)
    U.assert_rows(d.merged([3, 1, 0, 2], used, ALL, proj, order_by), want)
    U.assert_rows(d.table_rows(used, ALL, proj, order_by), want, "table")


def test_every_key_byte_active(d):
    want = d.want(USED, ALL, PROJ, [(0, True)])                                       # ORDER BY id DESC: ids span the int32 range
    ids = want[2][0].view("<i4").reshape(-1)
    assert all(np.unique((ids >> (8 * b)) & 0xFF).size > 1 for b in range(4))
    U.assert_rows(d.merged([1, 3, 2, 0], USED, ALL, PROJ, [(0, True)]), want)


# ---- limits ---------------------------------------------------------------------------------------------------------------
def test_limits(d):
    order_by = [(1, False)]
    youngest = [int((c[AGE].values == U.AGES.min()).sum()) for c in d.cols]
    assert youngest[0] > 3 and youngest[1] > 3
    inside = youngest[0] + 3                                 # cuts the first tie group inside segment 1: the group spans segments 0 .. 3
    total = sum(ROWS)
    for k in (inside, 1, total, total + 5, 0):
        want = d.want(USED, ALL, PROJ, order_by, k)
        assert want[0].size == (min(k, total) if k else total)
        if k == inside:
            assert want[0][-1] == 1 and want[2][1].view(np.int8).max() == U.AGES.min()
        got = d.merged([2, 0, 3, 1], USED, ALL, PROJ, order_by, k)                   # the Engine's shape: every query ordered with k
        U.assert_rows(got, want, ("own limit k", k))
        U.assert_rows(d.merged([2, 0, 3, 1], USED, ALL, PROJ, order_by, k, own_limit=0), want, ("own limit 0", k))
        if k in (inside, 1):
            U.assert_rows(d.table_rows(USED, ALL, PROJ, order_by, k), want, ("table", k))


# ---- list lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,lengths", [((None, 2065), [1025, 65, 0, 0]), ((960, 6063), [64, 1024, 1, 63]), ((5500, 5501), [0, 0, 0, 0])])
@pytest.mark.parametrize("limit", [0, 70])
def test_list_lengths(d, window, lengths, limit):
    sels = U.between(*window)
    order_by = [(1, True), (0, False)]                       # age desc, id
    qs = d.queries([0, 1, 2, 3], USED, sels, PROJ, order_by, limit)
    try:
        assert [q.row_count() for q in qs] == [min(n, limit) if limit else n for n in lengths]
        got = d.comm.merge_ordered(qs, [0, 1, 2, 3], limit)
    finally:
        for q in qs:
            q.close()
    U.assert_rows(got, d.want(USED, sels, PROJ, order_by, limit), (window, limit))


def test_single_query(d):
    order_by = [(1, False)]
    for s in (0, 2):
        U.assert_rows(d.merged([s], USED, ALL, PROJ, order_by, 0), d.want(USED, ALL, PROJ, order_by, 0, segments=(s,)), s)
    U.assert_rows(d.merged([3], USED, ALL, PROJ, order_by, 10), d.want(USED, ALL, PROJ, order_by, 10, segments=(3,)))


# ---- table queries --------------------------------------------------------------------------------------------------------
def test_table_query_next_to_segment_queries(d):
    native = d.native
    order_by = [(1, True)]
    t02 = native.DeviceTable(d.ctx, [d.segs[0], d.segs[2]])
    for limit in (0, 40):
        qs = [U.ordered_query(native, d.ctx, t02, USED, ALL, PROJ, order_by, limit)] + d.queries([1, 3], USED, ALL, PROJ, order_by, limit)
        try:
            if limit == 0:
                idx, _ = qs[0].fetch_rows()
                assert 2048 in idx.tolist()                  # segment 0 has 1025 rows = two tiles: virtual row 2048 is row 0 of the table's second segment
            got = d.comm.merge_ordered(qs, [[0, 2], 1, 3], limit)
        finally:
            for q in qs:
                q.close()
        U.assert_rows(got, d.want(USED, ALL, PROJ, order_by, limit), limit)
        if limit == 0:
            at = np.flatnonzero(got[0] == 2)
            assert at.size == 1 and got[1][at[0]] == 0
    t02.close()


def test_table_indices_need_not_follow_the_table_order(d):
    native = d.native
    t31 = native.DeviceTable(d.ctx, [d.segs[3], d.segs[1]])  # the table's first segment is global segment 3
    for order_by in ([(1, False)], [(1, True), (0, True)]):
        q = U.ordered_query(native, d.ctx, t31, USED, ALL, PROJ, order_by)
        try:
            got = d.comm.merge_ordered([q], [[3, 1]])
        finally:
            q.close()
        U.assert_rows(got, d.want(USED, ALL, PROJ, order_by, 0, segments=(1, 3)), order_by)
    # ... next to segment queries, cut by the merge's limit
    qs = [U.ordered_query(native, d.ctx, t31, USED, ALL, PROJ, [(1, False)])] + d.queries([2, 0], USED, ALL, PROJ, [(1, False)])
    try:
        got = d.comm.merge_ordered(qs, [[3, 1], 2, 0], 1500)
        U.assert_rows(got, d.want(USED, ALL, PROJ, [(1, False)], 1500), "with segments 2 and 0")
        # a limit of its own would have cut the table's ties in table order
        qs[0].close()
        qs[0] = U.ordered_query(native, d.ctx, t31, USED, ALL, PROJ, [(1, False)], 1500)
        for q in qs[1:]:
            q.close()
        qs[1:] = d.queries([2, 0], USED, ALL, PROJ, [(1, False)], 1500)
        with pytest.raises(native.Imm3Error) as e:
            d.comm.merge_ordered(qs, [[3, 1], 2, 0], 1500)
        assert e.value.code == native.ERR_ARG
    finally:
        for q in qs:
            q.close()
    t31.close()


# ---- the single-process flavour ------------------------------------------------------------------------------------------
def test_single_process_flavour(d):
    native = d.native
    order_by = [(1, True), (0, False)]
    (c0,) = native.Comm.create_all([d.ctx])
    try:
        for limit in (0, 33):
            qs = d.queries([2, 0, 3, 1], USED, ALL, PROJ, order_by, limit)
            try:
                got = native.Comm.merge_ordered_all([c0], [qs], [[2, 0, 3, 1]], limit)
            finally:
                for q in qs:
                    q.close()
            U.assert_rows(got, d.want(USED, ALL, PROJ, order_by, limit), limit)
    finally:
        c0.close()


# ---- max_rows -------------------------------------------------------------------------------------------------------------
def test_max_rows_reports_the_total_and_writes_no_more(d):
    import ctypes as C
    native = d.native
    order_by = [(1, False)]
    want = d.want(USED, ALL, PROJ, order_by, 500)
    seg, row, cols, total = d.merged([2, 0, 3, 1], USED, ALL, PROJ, order_by, 500, max_rows=100)
    assert total == 500 and seg.size == 100
    U.assert_rows((seg, row, cols), (want[0][:100], want[1][:100], [v[:100] for v in want[2]]))
    # the C call itself, into buffers with a sentinel behind max_rows rows
    qs = d.queries([0, 1, 2, 3], USED, ALL, PROJ, order_by, 500)
    try:
        n, keep = C.c_uint64(0), 100
        segb, rowb = np.full(keep + 8, 0xA5A5A5A5, np.uint32), np.full(keep + 8, 0xA5A5A5A5, np.uint32)
        colb = [np.full((keep + 8) * w, 0xA5, np.uint8) for w in (4, 1, 5)]
        ptrs = (C.c_void_p * 3)(*[c.ctypes.data for c in colb])
        qarr = (C.c_void_p * 4)(*[q._h for q in qs])
        idx = np.arange(4, dtype=np.int32)
        native._check(native.load().imm3_comm_merge_ordered(d.comm._h, qarr, idx.ctypes.data, 4, 500, segb.ctypes.data, rowb.ctypes.data, ptrs, keep, C.byref(n)))
        assert n.value == 500
        assert segb[:keep].astype(np.int64).tolist() == want[0][:keep].tolist() and (segb[keep:] == 0xA5A5A5A5).all() and (rowb[keep:] == 0xA5A5A5A5).all()
        for c, w, v in zip(colb, (4, 1, 5), want[2]):
            assert c[: keep * w].tobytes() == v[:keep].tobytes() and (c[keep * w:] == 0xA5).all()
    finally:
        for q in qs:
            q.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_communicator_usable(d):
    native = d.native
    order_by = [(1, False)]
    good = d.queries([0, 1], USED, ALL, PROJ, order_by)
    made = list(good)

    def refused(queries, index, limit=0):
        with pytest.raises(native.Imm3Error) as e:
            d.comm.merge_ordered(queries, index, limit)
        return e.value

    try:
        plain = native.DeviceQuery(d.ctx, d.segs[1], USED, ALL, PROJ, 0, 1024)
        plain.run()
        made.append(plain)
        assert refused([good[0], plain], [0, 1]).code == native.ERR_ARG                   # an unordered projection
        agg = native.DeviceQuery(d.ctx, d.segs[1], [AGE], [], (), 0, 1024, group_cols=[0], aggs=[(native.AGG_COUNT, 0)])
        agg.run()
        made.append(agg)
        assert refused([good[0], agg], [0, 1]).code == native.ERR_ARG                     # an aggregation
        unrun = U.ordered_query(native, d.ctx, d.segs[1], USED, ALL, PROJ, order_by, run=False)
        made.append(unrun)
        assert refused([good[0], unrun], [0, 1]).code == native.ERR_STATE                 # ordered, never run
        other_key = U.ordered_query(native, d.ctx, d.segs[1], USED, ALL, PROJ, [(1, True)])
        made.append(other_key)
        e = refused([good[0], other_key], [0, 1])
        assert e.code == native.ERR_ARG and "differ" in str(e)
        other_list = U.ordered_query(native, d.ctx, d.segs[1], [ID, AGE, NAME], ALL, PROJ, order_by)
        made.append(other_list)
        e = refused([good[0], other_list], [0, 1])
        assert e.code == native.ERR_ARG and "differ" in str(e)
        five = U.ordered_query(native, d.ctx, d.segs[1], USED, ALL, PROJ, order_by, 5)
        made.append(five)
        assert refused([good[0], five], [0, 1], 10).code == native.ERR_ARG                # own limit 5 under merge limit 10
        assert refused([good[0], five], [0, 1], 0).code == native.ERR_ARG                 # ... and under no limit
        assert refused(good, [1, 1]).code == native.ERR_ARG                               # a repeated segment index
        assert refused(good, [0, -1]).code == native.ERR_ARG
        U.assert_rows(d.comm.merge_ordered(good, [0, 1]), d.want(USED, ALL, PROJ, order_by, 0, segments=(0, 1)), "after the errors")
    finally:
        for q in made:
            q.close()
