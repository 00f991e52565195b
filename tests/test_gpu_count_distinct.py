"""GPU suite: COUNT(DISTINCT col) in the group-by aggregation (IMM3_AGG_COUNT_DISTINCT): an exact set of (group, value)
pairs per aggregate on the device, filled by k_distinct_mark behind the aggregation launch.  Every expectation is len(set(...)) per
group in plain Python / numpy over the rows."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, RawColumn, blocks_of
from immutable3_amd import native

pytestmark = pytest.mark.gpu
C, MN, MX, S, CD = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM, native.AGG_COUNT_DISTINCT
I32_POOL = np.array([-2 ** 31, -1, 2 ** 31 - 1, 0, 1, 7, 1 << 20, -(1 << 20), 255, 256, 65535, 65536], np.int32)
# columns of every segment made here
ID, AGE, S1, S2, S3, S4, K1, STATE, K32, KA, KB, W16, S5, UNIQ = range(14)
ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17]
LAYOUTS = {"b1024": 1024, "b64": 64, "ragged100": 100}


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def rand_strings(rng, n, w, alphabet):
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, a.size, size=(n, w))]


def make_cols(rng, n, block):
    """id int32 (a pool with INT_MIN, -1, INT_MAX), age int8 (all 256 values once n >= 256), s1 .. s4 strings, k1 a 1-byte key, state a
    2-byte key, k32 an int32 key, (ka, kb) an 8-byte key that is all ones in some rows, w16 a 16-byte string (key or MAX), s5 a 5-byte
    string, uniq int32 = the row number"""
    br = blocks_of(n, block)
    age = (np.arange(n) % 256 - 128).astype(np.int8)
    rng.shuffle(age)
    ka = rng.integers(-1, 2, size=n).astype(np.int32)
    kb = rng.integers(-1, 1, size=n).astype(np.int32)
    if n > 2:
        ka[n // 2] = kb[n // 2] = -1                       # the all-ones key: the table's reserved slot
    return [RawColumn(DENSE_INT, 4, I32_POOL[rng.integers(0, I32_POOL.size, size=n)], br),
            RawColumn(DENSE_TINYINT, 1, age, br),
            RawColumn(DENSE_STRING, 1, rand_strings(rng, n, 1, b"abcdefgh\x00\xff"), br),
            RawColumn(DENSE_STRING, 2, rand_strings(rng, n, 2, b"xyz\xff"), br),
            RawColumn(DENSE_STRING, 3, rand_strings(rng, n, 3, b"pq\x00"), br),
            RawColumn(DENSE_STRING, 4, rand_strings(rng, n, 4, b"01\xff"), br),
            RawColumn(DENSE_TINYINT, 1, rng.integers(-2, 3, size=n).astype(np.int8), br),
            RawColumn(DENSE_STRING, 2, rand_strings(rng, n, 2, b"ABCDEFG"), br),
            RawColumn(DENSE_INT, 4, rng.integers(-300, 300, size=n).astype(np.int32), br),
            RawColumn(DENSE_INT, 4, ka, br),
            RawColumn(DENSE_INT, 4, kb, br),
            RawColumn(DENSE_STRING, 16, rand_strings(rng, n, 16, b"ab"), br),
            RawColumn(DENSE_STRING, 5, rand_strings(rng, n, 5, b"ab"), br),
            RawColumn(DENSE_INT, 4, np.arange(n, dtype=np.int32), br)]


def row_bytes(col, r):
    """the raw bytes of row r of a column: what a key packs and what a distinct value is"""
    return col.dat[r * col.width:(r + 1) * col.width].tobytes()


def expect(cols, group, aggs, mask):
    """{first selected row of the group: (count, [value per aggregate])} in plain Python; a 16-byte string MAX: its bytes"""
    groups = {}
    for r in np.flatnonzero(mask).tolist():
        groups.setdefault(b"".join(row_bytes(cols[g], r) for g in group), []).append(r)
    out = {}
    for rows in groups.values():
        vals = []
        for (kind, c) in aggs:
            col = cols[c]
            if kind == C:
                vals.append(len(rows))
            elif kind == CD:
                vals.append(len(set(row_bytes(col, r) for r in rows)))
            elif col.codec == DENSE_STRING:
                vals.append(max(row_bytes(col, r) for r in rows))
            else:
                v = [int(col.values[r]) for r in rows]
                vals.append(sum(v) if kind == S else max(v) if kind == MX else min(v))
        out[rows[0]] = (len(rows), vals)
    return out


def fetched(q, cols, aggs):
    """the same dict from the query's getters (a string MAX through fetch_group_strings)"""
    keys, first, counts, vals = q.fetch_groups()
    strs = {j: q.fetch_group_strings(j) for j, (k, c) in enumerate(aggs) if k == MX and cols[c].codec == DENSE_STRING}
    out = {}
    for g in range(first.size):
        out[int(first[g])] = (int(counts[g]), [bytes(strs[j][g]) if j in strs else int(vals[g, j]) for j in range(len(aggs))])
    assert len(out) == first.size
    return out


def query(ctx, seg, cols, sels, group, aggs, expr=None):
    wide = sum(cols[g].width for g in group) > 8
    return native.DeviceQuery(ctx, seg, list(range(len(cols))), sels, (), 0, 1024, group_cols=group, aggs=aggs, wide_keys=wide, expr=expr)


def run_once(ctx, seg, cols, sels, group, aggs, expr=None):
    q = query(ctx, seg, cols, sels, group, aggs, expr)
    q.run()
    got, form = fetched(q, cols, aggs), q.agg_form()
    q.close()
    assert form == native.AGG_FORM_GENERAL
    return got


KEYS = {"none": [], "k1": [K1], "state": [STATE], "k32": [K32], "ka_kb": [KA, KB], "w16": [W16]}


# ---- the walk: every row count, layout, value column and key ---------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n", ROWS)
def test_against_python_sets(ctx, n, layout):
    rng = np.random.default_rng(n * 7 + LAYOUTS[layout])
    cols = make_cols(rng, n, LAYOUTS[layout])
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    everything = np.ones(n, bool)
    if n >= 256:
        assert len(set(cols[AGE].values.tolist())) == 256
    if n > 2:
        assert any(row_bytes(cols[KA], r) + row_bytes(cols[KB], r) == b"\xff" * 8 for r in range(n))
    for name, group in KEYS.items():
        for aggs in ([(CD, ID), (CD, AGE), (CD, S1), (CD, S2)], [(CD, S3), (C, ID), (CD, S4)]):
            assert run_once(ctx, seg, cols, [], group, aggs) == expect(cols, group, aggs, everything), (name, aggs)
    seg.close()


def test_extremes(ctx):
    n = 3 * 1024 + 17
    cols = make_cols(np.random.default_rng(3), n, 1024)
    same = np.zeros(n, np.int32) + 12345
    cols[K32] = RawColumn(DENSE_INT, 4, same, blocks_of(n, 1024))
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    everything = np.ones(n, bool)
    # every row distinct, in one group: no group column, and a key column that never changes
    for group in ([], [K32]):
        got = run_once(ctx, seg, cols, [], group, [(CD, UNIQ), (C, ID)])
        assert got == {0: (n, [n, n])} == expect(cols, group, [(CD, UNIQ), (C, ID)], everything)
    # every row the same
    assert run_once(ctx, seg, cols, [], [STATE], [(CD, K32)]) == expect(cols, [STATE], [(CD, K32)], everything)
    assert run_once(ctx, seg, cols, [], [], [(CD, K32), (C, ID)]) == {0: (n, [1, n])}
    # an always-false select: no group at all
    assert run_once(ctx, seg, cols, [(AGE, GT, 127.0)], [STATE], [(CD, ID)]) == {}
    assert run_once(ctx, seg, cols, [(AGE, GT, 127.0)], [], [(CD, ID), (C, ID)]) == {}
    seg.close()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_predicates(ctx, layout):
    n = 3 * 1024 + 17
    cols = make_cols(np.random.default_rng(5), n, LAYOUTS[layout])
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    age = cols[AGE].values.astype(np.int64)
    aggs = [(CD, ID), (CD, S3), (C, ID), (CD, AGE)]
    for group in ([STATE], [KA, KB], [W16]):
        got = run_once(ctx, seg, cols, [(AGE, GT, 18.0), (AGE, LT, 30.0)], group, aggs)
        assert got == expect(cols, group, aggs, (age > 18) & (age < 30)), group
        got = run_once(ctx, seg, cols, [(AGE, GT, 100.0), (AGE, LT, -100.0)], group, aggs, expr=[0, 1, native.EXPR_OR])
        assert got == expect(cols, group, aggs, (age > 100) | (age < -100)), group
    seg.close()


def test_beside_every_other_aggregate(ctx):
    n = 3 * 1024 + 17
    cols = make_cols(np.random.default_rng(7), n, 1024)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    age = cols[AGE].values.astype(np.int64)
    for sels, mask in (([], np.ones(n, bool)), ([(AGE, GT, -50.0), (AGE, LT, 90.0)], (age > -50) & (age < 90))):
        for group in ([STATE], [K32], [KA, KB], [W16], []):
            for aggs in ([(CD, AGE), (MX, W16), (C, ID), (CD, S2)], [(MN, ID), (CD, S4), (MX, AGE), (CD, ID)], [(S, AGE), (CD, S1), (S, ID), (CD, AGE)]):
                assert run_once(ctx, seg, cols, sels, group, aggs) == expect(cols, group, aggs, mask), (group, aggs)
    seg.close()


# ---- state across runs ---------------------------------------------------------------------------------------------------------
def test_runs_getters_and_a_recorded_run(ctx):
    n = 3 * 1024 + 17
    cols = make_cols(np.random.default_rng(9), n, 1024)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    age = cols[AGE].values.astype(np.int64)
    mask = (age > 18) & (age < 30)
    aggs = [(CD, ID), (C, ID), (CD, S2)]
    want = expect(cols, [STATE], aggs, mask)
    q = query(ctx, seg, cols, [(AGE, GT, 18.0), (AGE, LT, 30.0)], [STATE], aggs)
    for _ in range(3):                       # the same figures every time: the set really is cleared
        q.run()
        assert fetched(q, cols, aggs) == want
    q.run_select()
    assert q.count() == int(mask.sum())
    words = q.bitmap()
    assert sum(bin(int(w)).count("1") for w in words) == int(mask.sum())
    assert fetched(q, cols, aggs) == want    # (the groups of the last aggregation are still there)
    q.run()
    with ctx.capture() as cap:
        q.run()
    for _ in range(2):
        cap.graph.launch()
        assert fetched(q, cols, aggs) == want
    cap.graph.close()
    q.close()
    seg.close()


# ---- a table: one figure over all segments ---------------------------------------------------------------------------------------
def test_table_counts_over_all_segments(ctx):
    rng = np.random.default_rng(11)
    sizes = [1500, 64, 2049]
    per_seg = [make_cols(rng, n, 1024) for n in sizes]
    segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in per_seg]
    table = native.DeviceTable(ctx, segs)
    aggs = [(CD, ID), (C, ID), (CD, S3), (CD, AGE)]

    def by_key(cols, rows_of):
        out = {}
        for key, rows in rows_of.items():
            out[key] = (len(rows), [len(rows) if k == C else len(set(rows_v[c] for rows_v in rows)) for (k, c) in aggs])
        return out

    for group, sels, keep in (([STATE], [], lambda a: np.ones(a.size, bool)), ([K1], [(AGE, GT, 18.0), (AGE, LT, 90.0)], lambda a: (a > 18) & (a < 90)), ([], [], lambda a: np.ones(a.size, bool))):
        whole, parts = {}, []
        for cols in per_seg:
            part = {}
            age = cols[AGE].values.astype(np.int64)
            for r in np.flatnonzero(keep(age)).tolist():
                key = b"".join(row_bytes(cols[g], r) for g in group)
                vals = {c: row_bytes(cols[c], r) for (_, c) in aggs}
                whole.setdefault(key, []).append(vals)
                part.setdefault(key, []).append(vals)
            parts.append(by_key(None, part))
        want = by_key(None, whole)
        # the union is not the sum of the per-segment figures: otherwise this test would show nothing
        summed = {k: sum(p[k][1][0] for p in parts if k in p) for k in want}
        assert any(summed[k] != want[k][1][0] for k in want)
        q = native.DeviceQuery(ctx, table, list(range(14)), sels, (), 0, 1024, group_cols=group, aggs=aggs)
        q.run()
        keys, first, counts, vals = q.fetch_groups()
        kb = sum(per_seg[0][g].width for g in group)
        got = {int(keys[g]).to_bytes(8, "little")[:kb]: (int(counts[g]), vals[g].tolist()) for g in range(keys.size)}
        assert q.agg_form() == native.AGG_FORM_GENERAL
        q.close()
        assert got == want, group
    table.close()
    for s in segs:
        s.close()


# ---- views of the groups ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["small", "radix_forced", "above_2048_groups"])
def test_order_by_the_figure_and_having(ctx, path):
    n = 6 * 1024 + 5
    cols = make_cols(np.random.default_rng(13), n, 1024)
    if path == "above_2048_groups":
        cols[K32] = RawColumn(DENSE_INT, 4, np.random.default_rng(14).integers(0, 2500, size=n).astype(np.int32), blocks_of(n, 1024))
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    group = [K32] if path == "above_2048_groups" else [STATE]
    aggs = [(C, ID), (CD, AGE), (CD, S4)]
    want = expect(cols, group, aggs, np.ones(n, bool))
    if path == "above_2048_groups":
        assert len(want) > native.GROUP_ORDER_SMALL_MAX
    ctx.set_tuning(native.TV_GROUP_ORDER_RADIX if path == "radix_forced" else 0, 0)
    try:
        q = query(ctx, seg, cols, [], group, aggs)
        q.run()
        # ORDER BY the figure descending (ties: first-seen order), cut to a limit
        q.set_group_order([(native.GROUP_ORDER_AGG, 1, True)], 7)
        ordered = sorted(want.items(), key=lambda kv: (-kv[1][1][1], kv[0]))[:7]
        keys, first, counts, vals = q.fetch_groups()
        assert [(int(f), (int(c), v.tolist())) for f, c, v in zip(first, counts, vals)] == ordered
        assert (q.group_order_path() == native.GROUP_ORDER_SMALL) == (path == "small")
        # HAVING figure > t over the int8 column, then over the string column, the order still on
        for j, t in ((1, sorted(v[1][1] for v in want.values())[len(want) // 2]), (2, sorted(v[1][2] for v in want.values())[len(want) // 2])):
            q.set_group_filter([(j, 0, native.GT, t)], [0])
            kept = sorted(((f, v) for f, v in want.items() if v[1][j] > t), key=lambda kv: (-kv[1][1][1], kv[0]))
            assert 0 < len(kept) < len(want)
            keys, first, counts, vals = q.fetch_groups()
            assert [(int(f), (int(c), v.tolist())) for f, c, v in zip(first, counts, vals)] == kept[:7]
        # HAVING alone, first-seen order
        q.set_group_order([], 0)
        assert fetched(q, cols, aggs) == dict(kept)
        q.close()
    finally:
        ctx.set_tuning(0, 0)
    seg.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    n = 2000
    cols = make_cols(np.random.default_rng(17), n, 1024)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    with pytest.raises(native.Imm3Error) as e:
        query(ctx, seg, cols, [], [STATE], [(CD, S5)])
    assert e.value.code == native.ERR_ARG and "at most 4 bytes" in e.value.msg
    with pytest.raises(native.Imm3Error) as e:
        query(ctx, seg, cols, [], [STATE], [(C, ID), (CD, W16)])
    assert e.value.code == native.ERR_ARG and "at most 4 bytes" in e.value.msg
    for kind in (4, 9):
        with pytest.raises(native.Imm3Error) as e:
            query(ctx, seg, cols, [], [STATE], [(kind, AGE)])
        assert e.value.code == native.ERR_ARG and e.value.msg == "Unknown Aggregate type"
    # counts of distinct values do not add: every merge entry point refuses the query
    q = query(ctx, seg, cols, [], [STATE], [(C, ID), (CD, AGE)])
    q.run()
    comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
    calls = [lambda: comm.merge_groups([q], [0]), lambda: comm.merge_groups_wide([q], [0]),
             lambda: comm.merge_groups_view([q], [0], order=[(native.GROUP_ORDER_AGG, 1, True)], limit=3),
             lambda: native.Comm.merge_groups_all([comm], [[q]], [[0]]), lambda: native.Comm.merge_groups_wide_all([comm], [[q]], [[0]]),
             lambda: native.Comm.merge_groups_view_all([comm], [[q]], [[0]], order=[(native.GROUP_ORDER_AGG, 1, True)], limit=3)]
    for i, call in enumerate(calls):
        with pytest.raises(native.Imm3Error) as e:
            call()
        assert e.value.code == native.ERR_ARG and "COUNT_DISTINCT" in e.value.msg and "do not add" in e.value.msg, (i, e.value.msg)
    assert fetched(q, cols, [(C, ID), (CD, AGE)]) == expect(cols, [STATE], [(C, ID), (CD, AGE)], np.ones(n, bool))   # (the query is intact)
    comm.close()
    q.close()
    seg.close()


# ---- a query without the kind runs the forms it ran before --------------------------------------------------------------------
def test_forms_of_queries_without_the_kind(ctx):
    n = 8 * 1024
    cols = make_cols(np.random.default_rng(19), n, 1024)
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    aggs = [(C, ID), (MX, AGE)]
    for tuning, form in ((0, native.AGG_FORM_LANES), (100 + native.AGG_FORM_LANES_WIDE, native.AGG_FORM_LANES_WIDE), (100 + native.AGG_FORM_DIRECT, native.AGG_FORM_DIRECT),
                         (100 + native.AGG_FORM_TILE, native.AGG_FORM_TILE), (100 + native.AGG_FORM_GENERAL, native.AGG_FORM_GENERAL)):
        ctx.set_tuning(tuning, 0)
        try:
            q = query(ctx, seg, cols, [], [STATE], aggs)
            q.run()
            assert fetched(q, cols, aggs) == expect(cols, [STATE], aggs, np.ones(n, bool))
            assert q.agg_form() == form, (tuning, q.agg_form())
            q.close()
            q = query(ctx, seg, cols, [], [STATE], aggs + [(CD, AGE)])       # with the kind: the general form, whatever is asked for
            q.run()
            assert q.agg_form() == native.AGG_FORM_GENERAL
            q.close()
        finally:
            ctx.set_tuning(0, 0)
    seg.close()
