"""Seeded differential fuzzing of everything that orders (order_fuzz_util.py: the generator and the reference side): ORDER BY and top-k
over table projections (csrc/imm3_order.hip), the device merge of ordered results (csrc/imm3_merge_order.hip), ORDER BY and top-k over
groups (csrc/imm3_group_order.hip), with IMM3_STR_RANGE leaves among the predicates -- over table_fuzz_util's random tables: empty and
one-row segments in the middle, mixed block layouts, PFOR and snappy columns, a string column of 3 to 32 bytes in the SELECT list.

Bit-exact, no tolerance anywhere, and every ordered query is run twice: the second run must give the same bytes (no atomic decides a
place).  test_order_fuzz_host.py walks the same seeds on the CPU and asserts that none of this is hollow."""
import os

import numpy as np
import pytest

import order_fuzz_util as F
import order_util
import table_fuzz_util as U
from immutable3_amd import native
from merge_order_util import assert_rows
from test_gpu_fuzz_table import check_layout
from test_gpu_group_order import assert_same
from test_gpu_str_rows_table import check_select

pytestmark = pytest.mark.gpu
MORE = int(os.environ.get("IMM3_FUZZ_MORE", "0"))      # extra seeds per fuzzer for a long hunt (default: the bounded set)
KIND = {"count": native.AGG_COUNT, "min": native.AGG_MIN, "max": native.AGG_MAX, "sum": native.AGG_SUM}
SMALL, FULL, SELECT = native.GROUP_ORDER_SMALL, native.GROUP_ORDER_RADIX_FULL, native.GROUP_ORDER_RADIX_SELECT
MERGE_BASE = 103_000                                   # the generator of the merges' global indices and query orders


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.set_tuning(0, 0)
    c.close()


@pytest.fixture(scope="module")
def comm(ctx):
    c = native.Comm(ctx, 1, 0, native.comm_unique_id())
    yield c
    c.close()


class OnDevice:
    """a table's segments (six columns each) and its imm3_table"""

    def __init__(self, ctx, t):
        self.segs = [native.DeviceSegment(ctx, [c.native() for c in cols]) for cols in t.segs]
        self.table = native.DeviceTable(ctx, self.segs)

    def close(self):
        self.table.close()
        for s in self.segs:
            s.close()


def ordered_query(ctx, target, used, sels, proj, order_by, limit, reserve=None, expr=None):
    q = native.DeviceQuery(ctx, target, used, sels, proj, 0, 1024, expr=expr)
    q.set_order(order_by, limit)
    if reserve is not None:
        q.reserve_rows(reserve)
    return q


def rows_of(q):
    """(segment, row, columns) of an ordered query's rows"""
    idx, vals = q.fetch_rows()
    assert q.row_count() == idx.size
    seg, row = q.locate_rows(idx) if q.is_table else (np.zeros(idx.size, np.uint32), idx)
    return seg, row, vals


def run_twice(q, want, what):
    for rnd in range(2):
        q.run()
        assert q.row_count() == want[0].size, (what, rnd, q.row_count(), want[0].size)
        assert_rows(rows_of(q), want, (what, "run", rnd))


# ---- 1. ordered rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(F.ROW_SEEDS + MORE))
def test_fuzz_ordered_rows(ctx, oracle, seed):
    """Ordered flat queries over the table: the row count, the rows as (segment, row), the bytes of every SELECT-list column; count,
    bitmap, segment starts and the batch layout stay those of the unordered query; a single-segment table's query over the segment too."""
    for ti, (t, queries) in enumerate(F.row_cases(seed)):
        dev = OnDevice(ctx, t)
        for qi, fq in enumerate(queries):
            e = F.RowExpected(oracle, t, fq)
            limit = F.row_limit(fq.limit_kind, e.total)
            want = e.ordered(fq.order_by, limit)
            what = (seed, ti, qi, F.describe(t), fq.describe(), e.total, limit)
            q = ordered_query(ctx, dev.table, fq.used, fq.sels, fq.proj, fq.order_by, limit, fq.reserve)
            run_twice(q, want, what)
            check_select(q, e.per_seg)
            check_layout(q, e)
            q.run()                                                           # and behind the getters that describe the select
            assert_rows(rows_of(q), want, (what, "after the getters"))
            q.close()
            if len(t.seg_rows) == 1:
                q = ordered_query(ctx, dev.segs[0], fq.used, fq.sels, fq.proj, fq.order_by, limit, fq.reserve)
                run_twice(q, want, (what, "the segment"))
                assert q.count() == e.total and q.bitmap().tolist() == e.per_seg[0][0].tolist(), (what, "the segment")
                q.close()
        dev.close()


# ---- 2. ordered trees -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(F.ORDER_TREE_TABLES))
def test_fuzz_ordered_trees(ctx, comm, part):
    """Random AND / OR / NOT trees through imm3_query_create_table_expr with an order.  A tree the table refuses must be a predicted
    refusal, and is then answered the other way: one ordered query per segment, merged -- against the same expectation."""
    tables, cases = F.ordered_tree_cases()
    t = tables[part]
    dev = OnDevice(ctx, t)
    used = list(range(6))
    for case, (ti, leaves, tree, proj, order_by, limit_kind) in enumerate(cases):
        if ti != part:
            continue
        prog = U.postfix(tree)
        words, s = F.tree_survivors(t, leaves, tree, proj)
        limit = F.row_limit(limit_kind, s.total)
        want = s.ordered(order_by, limit)
        what = (case, F.describe(t), leaves, tree, proj, order_by, limit)
        predicted = F.tree_prediction(t, leaves, tree)
        try:
            q = ordered_query(ctx, dev.table, used, leaves, proj, order_by, limit, expr=prog)
        except native.Imm3Error as err:
            assert err.code == native.ERR_ARG and err.msg.startswith(native.TABLE_TREE_REFUSED) and predicted, (what, err.msg)
            qs = [ordered_query(ctx, seg, used, leaves, proj, order_by, limit, expr=prog) for seg in dev.segs]
            for si, qseg in enumerate(qs):
                qseg.run()
                assert qseg.bitmap().tolist() == words[si].tolist(), (what, si)
            for rnd in range(2):
                assert_rows(comm.merge_ordered(qs, list(range(len(qs))), limit), want, (what, "refused: merged", rnd))
            for qseg in qs:
                qseg.close()
            continue
        assert not predicted, what
        run_twice(q, want, what)
        got = q.bitmap()
        _, fw = q.segment_starts()
        for si, ws in enumerate(words):
            lo = int(fw[si])
            assert got[lo: lo + ws.size].tolist() == ws.tolist() and not got[lo + ws.size: int(fw[si + 1])].any(), (what, si)
        assert q.count() == s.total, what
        q.close()
    dev.close()


# ---- 3. the two top-k implementations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(F.ROW_SEEDS + MORE))
def test_fuzz_merge_equals_table(ctx, comm, oracle, seed):
    """Every ordered flat case again as one ordered query per segment (empty and one-row segments included), each with the case's limit,
    merged on a one-rank communicator: (a) identity global indices -- the table query's rows and bytes; (b) the global indices a random
    permutation and the queries passed in a random order -- order_util.merge_ordered, ties by global segment; (c) an ordered table
    query without a limit of its own, its global indices not ascending, next to one more segment query (k_merge_order_split)."""
    x = np.random.default_rng(MERGE_BASE + seed)
    for ti, (t, queries) in enumerate(F.row_cases(seed)):
        dev = OnDevice(ctx, t)
        n = len(t.seg_rows)
        for qi, fq in enumerate(queries):
            e = F.RowExpected(oracle, t, fq)
            limit = F.row_limit(fq.limit_kind, e.total)
            want = e.ordered(fq.order_by, limit)
            what = (seed, ti, qi, F.describe(t), fq.describe(), e.total, limit)
            qs = [ordered_query(ctx, seg, fq.used, fq.sels, fq.proj, fq.order_by, limit) for seg in dev.segs]
            for q in qs:
                q.run()
            # (a)
            tq = ordered_query(ctx, dev.table, fq.used, fq.sels, fq.proj, fq.order_by, limit)
            tq.run()
            from_table = rows_of(tq)
            tq.close()
            merged = comm.merge_ordered(qs, list(range(n)), limit)
            assert_rows(merged, want, (what, "a"))
            assert_rows(merged, tuple(np.asarray(a, np.int64) for a in from_table[:2]) + (from_table[2],), (what, "a: the table query"))
            # (b)
            global_of, passed = x.permutation(n), [int(i) for i in x.permutation(n)]
            want_b = order_util.merge_ordered(e.parts(global_of), e.codecs, fq.order_by, limit)
            for rnd in range(2):
                got = comm.merge_ordered([qs[i] for i in passed], [int(global_of[i]) for i in passed], limit)
                assert_rows(got, want_b, (what, "b", global_of.tolist(), passed, rnd))
            # (c)
            table_index = [int(g) + 1 for g in x.permutation(n)]
            if n >= 2 and table_index == sorted(table_index):
                table_index.reverse()
            extra, extra_index = int(x.integers(0, n)), int(x.choice([0, n + 1]))
            parts = e.parts(table_index) + [(extra_index,) + e.parts(np.arange(n))[extra][1:]]
            want_c = order_util.merge_ordered(parts, e.codecs, fq.order_by, limit)
            tq = ordered_query(ctx, dev.table, fq.used, fq.sels, fq.proj, fq.order_by, 0)
            tq.run()
            got = comm.merge_ordered([tq, qs[extra]], [table_index, extra_index], limit)
            assert_rows(got, want_c, (what, "c", table_index, extra, extra_index))
            tq.close()
            for q in qs:
                q.close()
        dev.close()


# ---- 4. ordered groups ------------------------------------------------------------------------------------------------------------
def fetch_all(q, t, aq):
    """(prefix keys, first rows of the whole table, counts, vals, {aggregate: strings}, key bytes) through all four getters"""
    keys, first, counts, vals = q.fetch_groups()
    strs = {j: q.fetch_group_strings(j) for j, (kind, c) in enumerate(aq.aggs) if kind != "count" and aq.used[c] in (U.STATE, U.NAME)}
    kb = q.fetch_group_keys()
    n = np.zeros(1, np.uint32)
    native._check(native.load().imm3_query_group_count(q._h, n.ctypes.data_as(native.C.POINTER(native.C.c_uint32))))
    assert int(n[0]) == first.size == kb.shape[0] == counts.size and all(s.shape[0] == first.size for s in strs.values())
    seg_of, row_of = q.locate_rows(first)
    assert all(int(r) < t.seg_rows[int(s)] for s, r in zip(seg_of, row_of))
    return keys, t.starts[seg_of.astype(np.int64)] + row_of.astype(np.int64), counts, vals, strs, kb


def agg_query(ctx, dev, aq):
    return native.DeviceQuery(ctx, dev.table, aq.used, aq.sels, (), 0, 1024, group_cols=aq.group, aggs=[(KIND[k], c) for k, c in aq.aggs],
                              wide_keys=aq.wide_keys)


@pytest.mark.parametrize("seed", range(F.GROUP_SEEDS + MORE))
def test_fuzz_ordered_groups(ctx, oracle, seed):
    """Random ordered aggregations over the table: the default path through all four getters, first rows through locate_rows; where that
    was the small launch, the pinned radix path byte for byte; an order set before the first run; no keys: first-seen order again."""
    for ti, (t, queries) in enumerate(F.group_cases(seed)):
        dev = OnDevice(ctx, t)
        for qi, oq in enumerate(queries):
            aq = oq.aq
            keep = U.Expected(oracle, t, aq.used, aq.sels, [0]).keep(t)
            groups = U.expected_groups(t, aq, keep)
            g = len(groups[2])
            limit = F.group_limit(oq.limit_kind, g)
            want = F.groups_result(t, aq, groups, F.lex_perm(F.group_key_bytes(t, aq, groups, oq.order), limit))
            first_seen = F.groups_result(t, aq, groups, np.arange(g))
            what = (seed, ti, qi, F.describe(t), oq.describe(), g, limit)
            q = agg_query(ctx, dev, aq)
            q.run()
            assert_same(fetch_all(q, t, aq), first_seen, (what, "before the order"))
            q.set_group_order(oq.order, limit)
            got = fetch_all(q, t, aq)
            path = q.group_order_path()
            assert_same(got, want, (what, "default path", path))
            if g > 1:
                assert path == (SMALL if g <= native.GROUP_ORDER_SMALL_MAX else (SELECT if limit > 0 and g >= 4 * limit else FULL)), (what, path)
            q.run()
            assert_same(fetch_all(q, t, aq), want, (what, "second run"))
            if path == SMALL:
                ctx.set_tuning(native.TV_GROUP_ORDER_RADIX, 0)
                try:
                    q.set_group_order(oq.order, limit)
                    radix = fetch_all(q, t, aq)
                    assert q.group_order_path() in (FULL, SELECT), what
                finally:
                    ctx.set_tuning(0, 0)
                assert_same(radix, got, (what, "radix against small"))
            q2 = agg_query(ctx, dev, aq)                                      # the same order, set before the first run
            q2.set_group_order(oq.order, limit)
            q2.run()
            assert_same(fetch_all(q2, t, aq), got, (what, "set before the run"))
            q2.close()
            q.set_group_order([])
            assert_same(fetch_all(q, t, aq), first_seen, (what, "order removed"))
            q.close()
        dev.close()
