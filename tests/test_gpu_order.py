"""ORDER BY on the device (imm3_query_set_order; csrc/imm3_order.hip) against the oracle: tests/order_util.py takes oracle_np's
unordered projection and numpy.lexsort over the normalised keys with the row's place as the last key.  Everything is bit-exact, and
every case is run twice (the second run of the same query must give the same bytes: no atomic decides a position).

Shapes: the order cuts the rows into 1024 pieces, one per wave, of whole 64-row steps; up to 65 536 rows ("one sort block": one step
of every wave) a piece is one step, above it a wave walks several.  The row counts below sit around those edges."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, EQ, GT, LT, MATCH, PforColumn, RawColumn, blocks_of
import order_util

pytestmark = pytest.mark.gpu

SORT_BLOCK = 1024 * 64          # csrc/imm3_internal.h: kOrderSweepRows
SEG_ROWS = 5 * 1024 + 37        # a partial last tile
EXPR_AND, EXPR_OR, EXPR_NOT = -1, -2, -4
ERR_ARG, ERR_STATE = 5, 7
S8_POOL = [bytes([0x80 + i, 0xFF, 0x00, 0x41, 0x9C, i, 0xFE, 0x7F + (i & 1)]) for i in range(6)]
# columns of the standard segment, by index
ID, K32, AGE, ST2, S8, PICK, ST2B = range(7)
CODECS = [DENSE_INT, DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING, DENSE_TINYINT, DENSE_STRING]


@pytest.fixture(scope="module")
def ctx():
    from immutable3_amd import native
    c = native.Context(0)
    yield c
    c.set_tuning(0, 0)
    c.close()


def special_int32(rng, n):
    """INT_MIN, -1, 0, INT_MAX and every byte value in every byte position, then random values; shuffled."""
    base = [-2 ** 31, -1, 0, 2 ** 31 - 1] + [((b << (8 * p)) & 0xFFFFFFFF) for p in range(4) for b in range(256)]
    v = np.array([x - (1 << 32) if x >= (1 << 31) else x for x in base], dtype=np.int64).astype(np.int32)
    if n <= v.size:
        return rng.permutation(v)[:n]
    more = rng.integers(-2 ** 31, 2 ** 31, size=n - v.size, dtype=np.int64).astype(np.int32)
    return rng.permutation(np.concatenate([v, more]))


def make_data(rng, n, picked):
    """The standard columns over n rows; PICK is 1 on exactly `picked` random rows."""
    pick = np.zeros(n, np.int8)
    pick[rng.permutation(n)[:picked]] = 1
    return [
        rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32),                    # ID
        special_int32(rng, n),                                                                       # K32
        (np.arange(n) % 256 - 128).astype(np.int8)[rng.permutation(n)],                              # AGE: -128 .. 127
        rng.integers(0, 256, size=(n, 2)).astype(np.uint8) | np.uint8(0x80) * (rng.random((n, 2)) < 0.5),  # ST2: bytes >= 0x80 among them
        np.array([list(S8_POOL[i]) for i in rng.integers(0, len(S8_POOL), size=n)], dtype=np.uint8).reshape(n, 8),  # S8
        pick,
        rng.integers(0x7E, 0x82, size=(n, 2)).astype(np.uint8),                                      # ST2B: few values around 0x80
    ]


def raw_cols(data, block_rows):
    widths = [4, 4, 1, 2, 8, 1, 2]
    return [RawColumn(c, w, d, block_rows) for c, w, d in zip(CODECS, widths, data)]


class Case:
    """One segment on the device and what the oracle needs of it."""

    def __init__(self, ctx, cols):
        from immutable3_amd import native
        self.ctx, self.cols = ctx, cols
        self.seg = native.DeviceSegment(ctx, [c.native() for c in cols])

    def close(self):
        self.seg.close()

    def query(self, used, sels, proj, order_by, limit=0, expr=None, reserve=None):
        from immutable3_amd import native
        q = native.DeviceQuery(self.ctx, self.seg, used, sels, proj, 0, 1024, expr=expr)
        q.set_order(order_by, limit)
        if reserve is not None:
            q.reserve_rows(reserve)
        return q

    def expect(self, used, sels, proj, order_by, limit=0, expr=None):
        npcols = [self.cols[u].npcol() for u in used]
        codecs = [value_codec(self.cols[u]) for u in used]
        return order_util.expected(npcols, codecs, sels, proj, order_by, limit, 1024, expr)

    def check(self, used, sels, proj, order_by, limit=0, expr=None, reserve=None, runs=2, q=None):
        own = q is None
        q = q or self.query(used, sels, proj, order_by, limit, expr, reserve)
        want_idx, want_vals = self.expect(used, sels, proj, order_by, limit, expr)
        for r in range(runs):
            q.run()
            assert q.row_count() == want_idx.size, (r, q.row_count(), want_idx.size)
            idx, vals = q.fetch_rows()
            assert idx.astype(np.int64).tolist() == want_idx.tolist(), ("row order", r)
            for j, (g, w) in enumerate(zip(vals, want_vals)):
                assert g.tobytes() == w.tobytes(), ("column", j, r)
        plan = q.plan()
        if own:
            q.close()
        return plan


def value_codec(col):
    return {0: DENSE_INT, 16: DENSE_INT, 17: DENSE_TINYINT, 18: DENSE_STRING}.get(col.codec, col.codec)


@pytest.fixture(scope="module")
def std(ctx):
    """5157 rows, every 3rd-ish row picked: shared by the key, top-k and refusal tests."""
    rng = np.random.default_rng(77)
    data = make_data(rng, SEG_ROWS, 1000)
    c = Case(ctx, raw_cols(data, blocks_of(SEG_ROWS, 1024)))
    c.data = data
    yield c
    c.close()


# ---- row counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1, 2 * SORT_BLOCK + 17, 1 << 20])
def test_row_counts(ctx, k):
    """k survivors, ordered by (age desc, id): int8 ties everywhere, an int32 key behind them."""
    rng = np.random.default_rng(1000 + k % 9973)
    n = SEG_ROWS if k <= SEG_ROWS else k + k // 3 + 37
    data = make_data(rng, n, k)
    c = Case(ctx, raw_cols(data, blocks_of(n, 1024)))
    try:
        plan = c.check([PICK, AGE, ID], [(0, EQ, 1.0)], [2, 1], [(1, True), (0, False)])
        assert plan["order_full_runs"] == 2 and plan["order_select_runs"] == 0, plan
    finally:
        c.close()


# ---- keys ----------------------------------------------------------------------------------------------------------
KEY_CASES = {
    "int32 asc": ([K32], [0], [(0, False)]),
    "int32 desc": ([K32], [0], [(0, True)]),
    "int8 asc": ([AGE, ID], [1, 0], [(1, False)]),
    "int8 desc": ([AGE, ID], [1, 0], [(1, True)]),
    "2-byte string": ([ST2, ID], [1, 0], [(1, False)]),
    "2-byte string desc": ([ST2, ID], [1, 0], [(1, True)]),
    "8-byte string": ([S8, ID], [0, 1], [(0, False)]),
    "8-byte string desc": ([S8, ID], [0, 1], [(0, True)]),
    "state asc, age desc": ([ST2B, AGE, ID], [2, 0, 1], [(1, False), (2, True)]),
    "four keys, 16 bytes": ([S8, K32, ST2, ST2B, ID], [4, 0, 3, 1, 2], [(1, False), (2, True), (4, False), (3, True)]),
}


@pytest.mark.parametrize("name", list(KEY_CASES))
def test_keys(std, name):
    used, proj, order_by = KEY_CASES[name]
    std.check(used, [], proj, order_by)


@pytest.mark.parametrize("desc", [False, True])
def test_all_keys_equal_keeps_row_order(ctx, desc):
    rng = np.random.default_rng(5)
    data = make_data(rng, SEG_ROWS, 900)
    data[K32] = np.full(SEG_ROWS, -7, np.int32)
    c = Case(ctx, raw_cols(data, blocks_of(SEG_ROWS, 1024)))
    try:
        q = c.query([PICK, K32, ID], [(0, EQ, 1.0)], [1, 2], [(0, desc)])
        c.check([PICK, K32, ID], [(0, EQ, 1.0)], [1, 2], [(0, desc)], q=q)
        idx, _ = q.fetch_rows()
        assert (np.diff(idx.astype(np.int64)) > 0).all() and idx.size == 900
        q.close()
        c.check([PICK, K32, ID], [(0, EQ, 1.0)], [1, 2], [(0, desc)], limit=10)     # ... and through the select: the first ten rows
    finally:
        c.close()


@pytest.mark.parametrize("limit", [0, 5])
def test_pass_skip_one_row_differs_in_the_top_byte(ctx, limit):
    """The top three bytes of the key are the same in every row but one, which differs in the TOP byte only: that byte's pass must
    run (a skip decided on 'almost every row' would leave the odd row in place)."""
    rng = np.random.default_rng(6)
    data = make_data(rng, SEG_ROWS, SEG_ROWS)
    v = (0x12345600 | rng.integers(0, 256, size=SEG_ROWS)).astype(np.int64)
    v[3333] = 0x11345600 | int(v[3333] & 0xFF)
    data[K32] = v.astype(np.int32)
    c = Case(ctx, raw_cols(data, blocks_of(SEG_ROWS, 1024)))
    try:
        c.check([K32, ID], [], [0, 1], [(0, False)], limit=limit)
        c.check([K32, ID], [], [0, 1], [(0, True)], limit=limit)
    finally:
        c.close()


# ---- top-k ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 10, 999, 1000, 1005])
def test_limits(std, limit):
    """1000 survivors: limit 1, 10, n - 1, n, n + 5."""
    plan = std.check([PICK, AGE, ID], [(0, EQ, 1.0)], [2, 1], [(1, True)], limit=limit)
    select = 1000 >= 4 * limit
    assert (plan["order_select_runs"], plan["order_full_runs"]) == ((2, 0) if select else (0, 2)), plan


def test_select_full_sort_switch(std):
    """The select runs when survivors >= 4 x limit: 1000 survivors, limit 250 takes it, 251 sorts every row."""
    for limit, select in ((250, True), (251, False)):
        for order_by in ([(1, False)], [(0, True), (1, False)]):
            plan = std.check([PICK, K32, ID], [(0, EQ, 1.0)], [2, 1], order_by, limit=limit)
            assert (plan["order_select_runs"], plan["order_full_runs"]) == ((2, 0) if select else (0, 2)), (limit, plan)


def test_threshold_value_straddles_a_piece_boundary(ctx):
    """Three rows below the threshold value and eleven rows equal to it at places 59 .. 69 of the result -- across the boundary
    between the first two waves' pieces; limit 9 takes the first six of them, in row order."""
    rng = np.random.default_rng(8)
    data = make_data(rng, SEG_ROWS, SEG_ROWS)
    age = np.zeros(SEG_ROWS, np.int8)
    age[[200, 300, 4000]] = -9
    age[59:70] = -5
    data[AGE] = age
    c = Case(ctx, raw_cols(data, blocks_of(SEG_ROWS, 1024)))
    try:
        q = c.query([AGE, ID], [], [1, 0], [(1, False)], 9)
        plan = c.check([AGE, ID], [], [1, 0], [(1, False)], limit=9, q=q)
        idx, _ = q.fetch_rows()
        assert idx.tolist() == [200, 300, 4000, 59, 60, 61, 62, 63, 64] and plan["order_select_runs"] == 2
        q.close()
        for limit in (3, 4, 13, 14, 15):
            c.check([AGE, ID], [], [1, 0], [(1, False)], limit=limit)
    finally:
        c.close()


def test_select_over_many_steps(ctx):
    """200 000 survivors (every wave walks several steps), few distinct keys: the threshold's ties sit in every piece."""
    rng = np.random.default_rng(9)
    n = 200_000 + 37
    data = make_data(rng, n, 200_000)
    c = Case(ctx, raw_cols(data, blocks_of(n, 1024)))
    try:
        for order_by, limit in (([(1, True)], 1000), ([(1, False), (2, True)], 50_000), ([(2, False)], 10)):
            plan = c.check([PICK, AGE, K32, ID], [(0, EQ, 1.0)], [3, 1, 2], order_by, limit=limit)
            assert plan["order_select_runs"] == 2, plan
    finally:
        c.close()


# ---- every producer of rows ----------------------------------------------------------------------------------------
def pinned(ctx, variant, make):
    ctx.set_tuning(variant, 0)
    try:
        return make()
    finally:
        ctx.set_tuning(0, 0)


def test_one_launch_projection(ctx):
    rng = np.random.default_rng(10)
    n = 40 * 1024 + 37
    data = make_data(rng, n, 100)
    c = Case(ctx, raw_cols(data, blocks_of(n, 1024)))
    try:
        used, sels, proj, order_by = [AGE, K32], [(0, GT, -40.0), (1, GT, -1.5e9)], [1, 0], [(1, True), (0, False)]
        q = pinned(ctx, 12, lambda: c.query(used, sels, proj, order_by))
        assert q.plan()["single_pass"], q.plan()
        plan = c.check(used, sels, proj, order_by, q=q)
        assert plan["ran_single_pass"], plan
        q.close()
        q = pinned(ctx, 12, lambda: c.query(used, sels, proj, order_by, 25))
        assert c.check(used, sels, proj, order_by, limit=25, q=q)["ran_single_pass"]
        q.close()
    finally:
        c.close()


def test_records_projection(ctx):
    rng = np.random.default_rng(11)
    n = 20 * 1024 + 37
    data = make_data(rng, n, 100)
    c = Case(ctx, raw_cols(data, blocks_of(n, 1024)))
    try:
        used, sels, proj, order_by = [ST2B, ID], [(0, MATCH, [bytes([0x80, 0x7F]), bytes([0x7E, 0x81]), bytes([0x81, 0x81])])], [1, 0], [(1, True), (0, True)]
        q = pinned(ctx, 12, lambda: c.query(used, sels, proj, order_by))
        assert q.plan()["records"] and not q.plan()["single_pass"], q.plan()
        c.check(used, sels, proj, order_by, q=q)
        q.close()
    finally:
        c.close()


def test_bitmap_path_with_a_gathered_column(std):
    q = std.query([AGE, ID, S8], [(0, GT, 100.0)], [1, 2], [(1, True), (0, False)])
    assert not q.plan()["records"] and not q.plan()["single_pass"], q.plan()
    std.check([AGE, ID, S8], [(0, GT, 100.0)], [1, 2], [(1, True), (0, False)], q=q)
    q.close()


def test_tree_with_or_and_not(std):
    # (age < -100 or age > 100) and not pick = 1
    sels = [(0, LT, -100.0), (0, GT, 100.0), (1, EQ, 1.0)]
    expr = [0, 1, EXPR_OR, 2, EXPR_NOT, EXPR_AND]
    std.check([AGE, PICK, K32], sels, [0, 2], [(0, True), (1, False)], expr=expr)
    std.check([AGE, PICK, K32], sels, [0, 2], [(1, True)], limit=7, expr=expr)


def test_pfor_key_column(ctx):
    rng = np.random.default_rng(12)
    n = SEG_ROWS
    ids = (np.cumsum(rng.integers(0, 50, size=n)) - 60_000).astype(np.int32)
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    br = blocks_of(n, 1024)
    c = Case(ctx, [PforColumn(ids, br), RawColumn(DENSE_TINYINT, 1, age, br)])
    try:
        c.check([1, 0], [(0, GT, 0.0)], [1, 0], [(0, True)])
        c.check([1, 0], [(0, GT, 0.0)], [1, 0], [(1, False), (0, True)], limit=33)
    finally:
        c.close()


class TableCase:
    """Three segments (2049, 1024, 3000 rows) as one table; equal keys straddle the segment boundaries."""
    ROWS = (2049, 1024, 3000)

    def __init__(self, ctx):
        from immutable3_amd import native
        rng = np.random.default_rng(13)
        self.ctx, self.cols, self.dsegs = ctx, [], []
        for n in self.ROWS:
            age = rng.integers(-3, 4, size=n).astype(np.int8)
            age[:40] = 2
            age[-40:] = 2                                             # the same key on both sides of every boundary
            ids = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
            st = rng.integers(0x7E, 0x82, size=(n, 2)).astype(np.uint8)
            br = blocks_of(n, 1024)
            cols = [RawColumn(DENSE_TINYINT, 1, age, br), RawColumn(DENSE_INT, 4, ids, br), RawColumn(DENSE_STRING, 2, st, br)]
            self.cols.append(cols)
            self.dsegs.append(native.DeviceSegment(ctx, [x.native() for x in cols]))
        self.table = native.DeviceTable(ctx, self.dsegs)

    def close(self):
        self.table.close()
        for s in self.dsegs:
            s.close()

    def check(self, used, sels, proj, order_by, limit=0, expr=None):
        from immutable3_amd import native
        per_seg = [[cols[u].npcol() for u in used] for cols in self.cols]
        codecs = [self.cols[0][u].codec for u in used]
        wseg, wrow, wvals = order_util.expected_table(per_seg, codecs, sels, proj, order_by, limit, 1024, expr)
        plain = native.DeviceQuery(self.ctx, self.table, used, sels, proj, 0, 1024, expr=expr)
        plain.run()
        q = native.DeviceQuery(self.ctx, self.table, used, sels, proj, 0, 1024, expr=expr)
        q.set_order(order_by, limit)
        for r in range(2):
            q.run()
            idx, vals = q.fetch_rows()
            seg, row = q.locate_rows(idx)
            assert q.row_count() == wseg.size
            assert seg.astype(np.int64).tolist() == wseg.tolist() and row.astype(np.int64).tolist() == wrow.tolist(), r
            for g, w in zip(vals, wvals):
                assert g.tobytes() == w.tobytes()
            assert q.count() == plain.count() and q.bitmap().tolist() == plain.bitmap().tolist()
            assert [a.tolist() for a in q.segment_starts()] == [a.tolist() for a in plain.segment_starts()]
        q.close()
        plain.close()


@pytest.fixture(scope="module")
def table(ctx):
    t = TableCase(ctx)
    yield t
    t.close()


def test_table_flat(table):
    table.check([0, 1, 2], [(0, GT, -2.0)], [1, 0, 2], [(1, True)])
    table.check([0, 1, 2], [(0, GT, -2.0)], [1, 0, 2], [(1, False), (2, True)], limit=100)
    table.check([0, 1, 2], [], [0, 1], [(0, False)], limit=4000)


def test_table_tree(table):
    sels = [(0, LT, -1.0), (0, GT, 1.0), (1, GT, 0.0)]
    table.check([0, 1, 2], sels, [1, 0], [(1, True)], expr=[0, 1, EXPR_OR, 2, EXPR_NOT, EXPR_AND])
    table.check([0, 1, 2], sels, [1, 0], [(1, False)], limit=50, expr=[0, 1, EXPR_OR, 2, EXPR_NOT, EXPR_AND])


def test_reservation_smaller_than_the_result(std):
    """settle_rows emits the rows again into larger arrays -- and must order them again."""
    for limit in (0, 20):
        q = std.query([PICK, AGE, ID], [(0, EQ, 1.0)], [2, 1], [(1, True), (0, False)], limit, reserve=100)
        plan = std.check([PICK, AGE, ID], [(0, EQ, 1.0)], [2, 1], [(1, True), (0, False)], limit=limit, q=q)
        assert plan["order_launches"] >= 3, plan          # two runs and at least one re-order behind the re-emit
        q.close()


# ---- the getters that describe the select, not the order -------------------------------------------------------------
def test_count_and_bitmap_unchanged(std):
    from immutable3_amd import native
    used, sels, proj = [AGE, PICK, ID], [(0, GT, 0.0), (1, EQ, 1.0)], [2, 0]
    plain = native.DeviceQuery(std.ctx, std.seg, used, sels, proj, 0, 1024)
    plain.run()
    for limit in (0, 10):
        q = std.query(used, sels, proj, [(1, True)], limit)
        q.run()
        assert q.count() == plain.count() and q.bitmap().tolist() == plain.bitmap().tolist()
        # the unordered projection stays where it was: device pointers 2, 3, 16+j are not the ordered arrays
        from immutable3_amd.native import PTR_ORDER_COLUMN, PTR_ORDER_ROW_COUNT, PTR_ORDER_ROW_INDEX
        assert q.device_ptr(2) != q.device_ptr(PTR_ORDER_ROW_INDEX) and q.device_ptr(16) != q.device_ptr(PTR_ORDER_COLUMN)
        assert q.device_ptr(PTR_ORDER_ROW_COUNT) not in (0, q.device_ptr(3)) and q.device_ptr(PTR_ORDER_COLUMN + 1) not in (0, q.device_ptr(17))
        assert q.row_count() == (limit or plain.row_count())
        q.close()
    plain.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def refused(fn, code, text=None):
    from immutable3_amd import native
    with pytest.raises(native.Imm3Error) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    if text:
        assert text in str(e.value), str(e.value)


def test_refusals(std):
    from immutable3_amd import native
    ctx, seg = std.ctx, std.seg
    mk = lambda proj=(1, 0), limit=0, **kw: native.DeviceQuery(ctx, seg, [AGE, ID, S8, K32, ST2B], [(0, GT, 0.0)], list(proj), limit, 1024, **kw)  # noqa: E731
    q = mk()
    refused(lambda: q.set_order([]), ERR_ARG)                                              # n_keys outside 1 .. 4
    refused(lambda: q.set_order([(0, False)] * 5), ERR_ARG)
    refused(lambda: q.set_order([(2, False)]), ERR_ARG)                                    # proj out of range
    refused(lambda: q.set_order([(-1, False)]), ERR_ARG)
    refused(lambda: q.set_order([(0, False), (0, True)]), ERR_ARG)                         # ... repeated
    q.set_order([(0, False), (1, True)], 3)                                                # (a refused call leaves the query usable)
    q.run()
    assert q.row_count() == 3
    refused(lambda: q.set_order([(0, False)]), ERR_STATE)                                  # has already run
    q.close()
    q = mk(proj=(2, 3, 4, 1, 0))
    refused(lambda: q.set_order([(0, False), (1, False), (2, False), (3, False)]), ERR_ARG, "16")   # 8 + 4 + 2 + 4 = 18 bytes
    q.close()
    q = mk(proj=())
    refused(lambda: q.set_order([(0, False)]), ERR_ARG)                                    # non-projecting
    q.close()
    q = native.DeviceQuery(ctx, seg, [AGE, ID], [], [], 0, 1024, group_cols=[0], aggs=[(0, 1)])
    refused(lambda: q.set_order([(0, False)]), ERR_ARG)                                    # aggregation
    q.close()
    q = mk(limit=10)
    refused(lambda: q.set_order([(0, False)], 5), ERR_ARG, "limit")                        # a creation-time limit, with or without an order limit
    refused(lambda: q.set_order([(0, False)]), ERR_ARG, "limit")
    q.close()
    q = mk()                                                                               # an ordered run inside a capture
    q.set_order([(0, False)])
    q.run()
    plain = mk()
    plain.run()
    with pytest.raises(native.Imm3Error) as e:
        with ctx.capture():
            plain.run()
            q.run()
    plain.close()
    assert e.value.code == ERR_STATE and "capture" in str(e.value)
    q.run()
    assert q.row_count() == q.count()
    q.close()


# ---- seeded fuzz -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_fuzz(ctx, seed):
    """200 small cases (20 seeds x 10): key kinds, directions, limits, a segment or a table."""
    from immutable3_amd import native
    rng = np.random.default_rng(31000 + seed)
    for _ in range(10):
        as_table = rng.random() < 0.4
        rows = [int(rng.choice([1, 64, 700, 1024, 2049, 3000]))] * 1 if not as_table else [int(rng.choice([1024, 2049, 3000, 5157])) for _ in range(int(rng.integers(1, 4)))]
        few = rng.random() < 0.5
        per_seg = []
        for n in rows:
            data = make_data(rng, n, int(rng.integers(0, n + 1)))
            if few:                                                     # few distinct keys: ties decide
                data[K32] = rng.integers(-2, 3, size=n).astype(np.int32)
                data[AGE] = rng.integers(-1, 2, size=n).astype(np.int8)
            per_seg.append(raw_cols(data, blocks_of(n, 1024)))
        used = [PICK] + [int(x) for x in rng.permutation([ID, K32, AGE, ST2B, S8])[: int(rng.integers(1, 5))]]
        sels = [(0, EQ, 1.0)] if rng.random() < 0.7 else []
        proj = [int(x) for x in rng.permutation(np.arange(1, len(used)))]
        order_by, width = [], 0
        for j in rng.permutation(len(proj)):
            w = per_seg[0][used[proj[int(j)]]].width
            if len(order_by) < 4 and width + w <= 16 and (not order_by or rng.random() < 0.6):
                order_by.append((int(j), bool(rng.random() < 0.5)))
                width += w
        limit = int(rng.choice([0, 0, 1, 7, 100, 10_000]))
        codecs = [CODECS[u] for u in used]
        dsegs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in per_seg]
        target = native.DeviceTable(ctx, dsegs) if as_table else dsegs[0]
        q = native.DeviceQuery(ctx, target, used, sels, proj, 0, 1024)
        q.set_order(order_by, limit)
        wseg, wrow, wvals = order_util.expected_table([[cols[u].npcol() for u in used] for cols in per_seg], codecs, sels, proj, order_by, limit)
        for r in range(2):
            q.run()
            idx, vals = q.fetch_rows()
            seg, row = q.locate_rows(idx) if as_table else (np.zeros(idx.size, np.uint32), idx)
            what = (seed, rows, used, sels, proj, order_by, limit, r)
            assert seg.astype(np.int64).tolist() == wseg.tolist() and row.astype(np.int64).tolist() == wrow.tolist(), what
            assert all(g.tobytes() == w.tobytes() for g, w in zip(vals, wvals)), what
        q.close()
        if as_table:
            target.close()
        for s in dsegs:
            s.close()


# ---- no host wait beyond the projection's own; a long SELECT list's device pointers ----------------------------------------------
def test_an_ordered_run_waits_for_the_device_exactly_when_the_unordered_one_does(std):
    """imm3_query_plan's run_syncs (times imm3_query_run had to wait for the device) of an ordered query and of the same query without
    an order, over the first and three more runs, for every producer shape: unreserved (one wait, on the first run), reserved (none)."""
    from immutable3_amd import native
    for used, sels, proj in (([PICK, AGE, ID], [(0, EQ, 1.0)], [2, 1]), ([AGE, K32], [(0, GT, 0.0), (1, GT, 0.0)], [1, 0]), ([AGE, ID, S8], [], [1, 2])):
        for reserve in (None, SEG_ROWS):
            syncs = []
            for ordered in (False, True):
                q = native.DeviceQuery(std.ctx, std.seg, used, sels, proj, 0, 1024)
                if ordered:
                    q.set_order([(0, True)], 10)
                if reserve:
                    q.reserve_rows(reserve)
                for _ in range(4):
                    q.run()
                syncs.append(q.plan()["run_syncs"])
                q.row_count()
                q.close()
            assert syncs[0] == syncs[1] and syncs[0] <= 1, (used, reserve, syncs)


def test_device_pointers_of_a_long_select_list(std):
    """A SELECT list has no bound, so 16+j runs past 32, 33 and 48: those ids keep meaning unordered columns 16, 17 and 32 -- on a query
    without an order and on an ordered one alike; the ordered arrays sit at IMM3_PTR_ORDER_*."""
    from immutable3_amd import native
    proj = [0, 1] * 17                                            # 34 SELECT-list entries: more than two gather groups of 8
    got = {}
    for ordered in (False, True):
        q = native.DeviceQuery(std.ctx, std.seg, [AGE, ID], [(0, GT, 100.0)], proj, 0, 1024)
        if ordered:
            q.set_order([(33, True), (0, False)], 0)
        q.run()
        n = q.row_count()
        ptrs = [q.device_ptr(16 + j) for j in range(len(proj))]
        assert all(ptrs) and len(set(ptrs)) == len(proj)
        assert q.device_ptr(32) == ptrs[16] and q.device_ptr(33) == ptrs[17] and q.device_ptr(48) == ptrs[32]
        if ordered:
            own = [q.device_ptr(native.PTR_ORDER_COLUMN + j) for j in range(len(proj))] + [q.device_ptr(native.PTR_ORDER_ROW_INDEX), q.device_ptr(native.PTR_ORDER_ROW_COUNT)]
            assert all(own) and not set(own) & set(ptrs + [q.device_ptr(2), q.device_ptr(3)])
        else:
            for which in (native.PTR_ORDER_ROW_INDEX, native.PTR_ORDER_ROW_COUNT, native.PTR_ORDER_COLUMN):
                refused(lambda: q.device_ptr(which), ERR_ARG)
        got[ordered] = (n, q.fetch_rows())
        q.close()
    (n0, (idx0, vals0)), (n1, (idx1, vals1)) = got[False], got[True]
    age, ids = vals0[0].view(np.int8).reshape(-1).astype(np.int64), vals0[1].view("<i4").reshape(-1).astype(np.int64)
    perm = np.lexsort((np.arange(n0), age, -ids))                 # id desc (entry 33), then age (entry 0), then row order
    assert n0 == n1 and idx1.tolist() == idx0[perm].tolist()
    assert all(v1.tobytes() == v0[perm].tobytes() for v0, v1 in zip(vals0, vals1))
