"""CPU census of the order fuzz (order_fuzz_util.py, test_gpu_fuzz_order.py): the generator and the whole reference side run over every
seed the GPU tests use, without a device.  It asserts that the fuzz is not hollow -- every table shape, key kind, direction, limit
position, tie and path threshold the GPU tests are there for really occurs -- and holds the references against each other: the
group-key restatement against test_gpu_group_order.normal_keys, order_util.merge_ordered against order_util.expected_table."""
import numpy as np
import pytest

import order_fuzz_util as F
import order_util
import table_fuzz_util as U
from conftest import DENSE_INT, DENSE_TINYINT, EQ, GT, LT
from immutable3_amd import native
from test_gpu_group_order import normal_keys

# what the chosen seed bases give, pinned so that a later change to a generator or a default cannot hollow the fuzz out unnoticed
ROW_CASES, ROW_CASES_EMPTY, ROW_CASES_BIG = 144, 24, 3
TREE_REFUSED, TREE_ACCEPTED_WITH_NOT = 3, 18
GROUP_CASES, GROUP_CASES_TINY, GROUP_CASES_RADIX = 96, 18, 15
KMAX = native.GROUP_ORDER_SMALL_MAX
SORT_BLOCK = 65_536


def check_table(t):
    assert all(U.layout_ok(br) and sum(br) == n for br, n in zip(t.layouts, t.seg_rows)), F.describe(t)
    assert all(len(cols) == 6 for cols in t.segs) and all(d.shape[0] == t.n_rows for d in t.data) and t.n_rows <= 150_000
    assert t.note_width in F.NOTE_WIDTHS and t.widths[F.NOTE] == t.note_width and t.data[F.NOTE].shape == (t.n_rows, t.note_width)
    assert 24 <= 2 * t.note_pool.shape[0] and t.note_pool.shape[0] <= 48 and t.note_pool.min() < 0x80 <= t.note_pool.max()
    if t.codecs[F.NOTE] == U.SNAPPY:
        assert max([max(br) for br in t.layouts if br], default=0) * t.note_width <= U.SNAPPY_MAX_BLOCK_BYTES
    if t.few and t.n_rows:
        assert np.unique(t.data[U.V]).size <= 3 and np.unique(t.data[U.AGE]).size <= 3


def check_order(t, used, proj, order_by):
    """the rules of imm3_query_set_order"""
    assert 1 <= len(order_by) <= 4 and len({i for i, _ in order_by}) == len(order_by) and all(0 <= i < len(proj) for i, _ in order_by)
    assert sum(t.widths[used[proj[i]]] for i, _ in order_by) <= 16


@pytest.fixture(scope="module")
def row_census(oracle):
    cases = []
    for seed in range(F.ROW_SEEDS):
        for t, qs in F.row_cases(seed):
            check_table(t)
            for q in qs:
                cases.append((seed, t, q, F.RowExpected(oracle, t, q)))
    return cases


def test_ordered_rows_cover_tables_keys_limits_and_ties(row_census):
    seen, empty, big = set(), 0, 0
    assert len(row_census) == ROW_CASES == F.ROW_SEEDS * F.ROW_TABLES * F.ROW_QUERIES
    for seed, t, q, e in row_census:
        check_order(t, q.used, q.proj, q.order_by)
        assert q.proj and len(set(q.used)) == len(q.used) and len(q.ranges) <= 1
        for j, (lo, hi) in q.ranges:                                          # a table takes a range on these widths only (include/imm3.h)
            assert q.used[j] in (U.NAME, F.NOTE) and t.widths[q.used[j]] % 4 == 0 and max(len(lo), len(hi)) <= t.widths[q.used[j]]
        T = e.total
        assert T == sum(c for _, c in e.per_seg)
        limit = F.row_limit(q.limit_kind, T)
        key_cols = [q.used[q.proj[i]] for i, _ in q.order_by]
        key_width = sum(t.widths[c] for c in key_cols)
        seen.add("note width %d" % t.note_width)
        if F.NOTE in key_cols:
            seen.add("note a key, width %d" % t.note_width)
        elif F.NOTE in [q.used[j] for j in q.proj]:
            seen.add("note in the list only, width %d" % t.note_width)
        for (i, desc), c in zip(q.order_by, key_cols):
            kind = {DENSE_INT: "int32", DENSE_TINYINT: "int8"}.get(F.VALUE_CODECS[c], "string")
            seen.add("%s %s" % (kind, "descending" if desc else "ascending"))
            if T >= 2 and t.codecs[c] != U.DENSE:
                seen.add("a %s key column" % t.codecs[c])
        seen.add("%d keys" % len(q.order_by))
        if key_width == 16:
            seen.add("16 key bytes")
        empty += T == 0
        big += T > SORT_BLOCK
        seen.add("T = 0" if T == 0 else "T = 1" if T == 1 else "T in 65 .. 65536" if 65 <= T <= SORT_BLOCK else "T > 65536" if T > SORT_BLOCK else "T small")
        if T > SORT_BLOCK:
            assert any(n == 20_000 for n in t.seg_rows)
        seen.add("limit " + q.limit_kind)
        keys = e.keys(q.order_by)
        perm = order_util.order_permutation(keys)
        if T >= 65:
            active = [np.unique(keys[:, b]).size > 1 for b in range(keys.shape[1])]
            seen.add("every key byte active" if all(active) else "a pass skipped")
        if limit > 0 and T >= 2:
            seen.add("the select runs" if T >= 4 * limit else "limit >= T" if limit >= T else "the full sort runs")
            if limit < T and keys[perm[limit - 1]].tobytes() == keys[perm[limit]].tobytes():
                seen.add("ties cut at the threshold")
        sorted_keys, sorted_seg = keys[perm], e.seg[perm]
        if T >= 2 and ((sorted_keys[1:] == sorted_keys[:-1]).all(axis=1) & (sorted_seg[1:] != sorted_seg[:-1])).any():
            seen.add("ties across a segment boundary")
        if T >= 2:
            if 0 in t.seg_rows[1:-1]:
                seen.add("an empty segment in the middle")
            if 1 in t.seg_rows[1:-1]:
                seen.add("a one-row segment in the middle")
            if F.is_mixed(t):
                seen.add("a mixed layout")
            if len(t.seg_rows) == 1:
                seen.add("a single-segment table")
        if q.reserve is not None and q.reserve < T:
            seen.add("a reservation too small")
        if q.ranges and any(cond in (GT, LT, EQ) for _, cond, _ in q.base_sels):
            seen.add("a range beside a numeric predicate")
        if q.ranges and 0 < T < t.n_rows:
            seen.add("a range that cuts")
    want = {"note width %d" % w for w in F.NOTE_WIDTHS} | {"note a key, width 3", "note a key, width 5", "note in the list only, width 20",
                                                            "note in the list only, width 32"}
    want |= {"%s %s" % (k, d) for k in ("int32", "int8", "string") for d in ("ascending", "descending")}
    want |= {"1 keys", "4 keys", "16 key bytes", "a pass skipped", "every key byte active", "T = 0", "T = 1", "T in 65 .. 65536", "T > 65536"}
    want |= {"limit " + k for k in F.ROW_LIMIT_KINDS} | {"the select runs", "the full sort runs", "limit >= T", "ties cut at the threshold"}
    want |= {"ties across a segment boundary", "an empty segment in the middle", "a one-row segment in the middle", "a mixed layout",
             "a single-segment table", "a pfor key column", "a snappy key column", "a reservation too small",
             "a range beside a numeric predicate", "a range that cuts"}
    assert want <= seen, sorted(want - seen)
    assert (empty, big) == (ROW_CASES_EMPTY, ROW_CASES_BIG), (empty, big)
    assert 4 * empty <= len(row_census) and big >= 2


def test_merge_reference_agrees_with_the_table_reference(row_census):
    """order_util.merge_ordered over the per-segment survivors (in global order, and with the global indices reversed) against
    order_util.expected_table -- oracle_np's own projection -- on the cases that one knows (no range leaf) and can afford"""
    held = 0
    for seed, t, q, e in row_census:
        if q.ranges or t.n_rows > 30_000:
            continue
        held += 1
        n = len(t.seg_rows)
        limit = F.row_limit(q.limit_kind, e.total)
        codecs = [F.VALUE_CODECS[c] for c in q.used]
        per_seg = [[cols[c].npcol() for c in q.used] for cols in t.segs]
        want = order_util.expected_table(per_seg, codecs, q.sels, q.proj, q.order_by, limit)
        mine = e.ordered(q.order_by, limit)
        merged = order_util.merge_ordered(e.parts(np.arange(n)), e.codecs, q.order_by, limit)
        turned = (order_util.merge_ordered(e.parts(np.arange(n)[::-1]), e.codecs, q.order_by, limit),
                  order_util.expected_table(per_seg[::-1], codecs, q.sels, q.proj, q.order_by, limit))
        for got, ref in ((mine, want), (merged, want), turned):
            assert got[0].tolist() == ref[0].tolist() and got[1].tolist() == ref[1].tolist(), (seed, q.describe())
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[2], ref[2])), (seed, q.describe())
    assert held >= len(row_census) // 3


def test_ordered_trees_keep_the_refusals_within_bounds():
    tables, cases = F.ordered_tree_cases()
    assert len(cases) == F.ORDER_TREE_COUNT and len(tables) == F.ORDER_TREE_TABLES
    refused = accepted_with_not = 0
    for t in tables:
        check_table(t)
    for ti, leaves, tree, proj, order_by, limit_kind in cases:
        t = tables[ti]
        check_order(t, list(range(6)), proj, order_by)
        assert all(leaf[0] < 5 for leaf in leaves)
        words, s = F.tree_survivors(t, leaves, tree, proj)
        assert len(words) == len(t.seg_rows)
        s.ordered(order_by, F.row_limit(limit_kind, s.total))
        if F.tree_prediction(t, leaves, tree):
            refused += 1
        elif U.has_not(tree):
            accepted_with_not += 1
    assert (refused, accepted_with_not) == (TREE_REFUSED, TREE_ACCEPTED_WITH_NOT), (refused, accepted_with_not)
    assert 1 <= refused and 4 * refused <= F.ORDER_TREE_COUNT and accepted_with_not > 1
    assert any(n <= 1 for t in tables for n in t.seg_rows[:-1])


KIND = {"count": native.AGG_COUNT, "min": native.AGG_MIN, "max": native.AGG_MAX, "sum": native.AGG_SUM}


def other_restatement(t, oq, groups):
    """test_gpu_group_order.normal_keys over the same groups: numpy's uint64 arithmetic where group_key_bytes uses Python ints"""
    aq = oq.aq
    keys, first, counts, vals = groups
    g = len(counts)
    cols = [t.segs[0][c] for c in aq.used]
    strs, v = {}, np.zeros((g, len(aq.aggs)), np.int64)
    for j, (kind, cj) in enumerate(aq.aggs):
        if kind != "count" and aq.used[cj] in (U.STATE, U.NAME):
            strs[j] = np.frombuffer(b"".join(vals[i][j] for i in range(g)), np.uint8).reshape(g, t.widths[aq.used[cj]])
        else:
            v[:, j] = [int(vals[i][j]) for i in range(g)]
    exp = (None, np.arange(g, dtype=np.uint64), np.array(counts, np.uint64), v, strs, np.asarray(keys))
    return normal_keys(cols, aq.group, [(KIND[k], c) for k, c in aq.aggs], exp, oq.order)


def test_ordered_groups_cover_counts_and_key_kinds_and_the_restatements_agree(oracle):
    seen, tiny, radix, cases = set(), 0, 0, 0
    for seed in range(F.GROUP_SEEDS):
        for t, qs in F.group_cases(seed):
            check_table(t)
            for oq in qs:
                aq = oq.aq
                cases += 1
                assert 1 <= len(oq.order) <= 4 and len({(k, i) for k, i, _ in oq.order}) == len(oq.order)
                widths = {(k, i): w for k, i, w, _ in F.group_key_candidates(t, aq)}
                assert all(widths[(k, i)] <= F.KEY_MAX for k, i, _ in oq.order) and sum(widths[(k, i)] for k, i, _ in oq.order) + 4 <= 16
                keep = U.Expected(oracle, t, aq.used, aq.sels, [0]).keep(t)
                groups = U.expected_groups(t, aq, keep)
                g = len(groups[2])
                nk = F.group_key_bytes(t, aq, groups, oq.order)
                assert nk.shape == (g, sum(widths[(k, i)] for k, i, _ in oq.order) + 4)
                if g:
                    other = other_restatement(t, oq, groups)
                    assert other.shape == nk.shape and other.tobytes() == nk.tobytes(), (seed, oq.describe())
                limit = F.group_limit(oq.limit_kind, g)
                perm = F.lex_perm(nk, limit)
                F.groups_result(t, aq, groups, perm)
                tiny += g <= 1
                radix += g > KMAX
                seen.add("g = 0" if g == 0 else "g = 1" if g == 1 else "g up to 2048" if g <= KMAX else "g > 2048")
                seen.add("limit " + oq.limit_kind)
                if limit > 0 and g >= 2:
                    seen.add(("small" if g <= KMAX else "radix") + (", the select side" if g >= 4 * limit else ", the sort side"))
                seen.update(oq.kinds)
                for k, i, desc in oq.order:
                    seen.add("descending" if desc else "ascending")
                if aq.wide_keys:
                    seen.add("wide keys")
                if any(aq.used[j] == U.NAME for j in aq.group):
                    seen.add("name in the group key")
                if g >= 3:
                    user = nk[:, :-4]
                    _, n_same = np.unique(user, axis=0, return_counts=True) if user.shape[1] else (None, np.array([g]))
                    if n_same.max() >= 3:
                        seen.add("first-seen order decides")
                if g >= 2 and any(t.codecs[aq.used[aq.group[i]] if k == F.G_COL else aq.used[aq.aggs[i][1]]] != U.DENSE for k, i, _ in oq.order):
                    seen.add("a compressed key column")
    want = {"g = 0", "g = 1", "g up to 2048", "g > 2048", "small, the select side", "small, the sort side", "radix, the select side",
            "radix, the sort side", "group int32", "group int8", "group string", "count", "sum", "int min", "int max", "string max",
            "ascending", "descending", "wide keys", "name in the group key", "first-seen order decides", "a compressed key column"}
    want |= {"limit " + k for k in F.GROUP_LIMIT_KINDS}
    assert want <= seen, sorted(want - seen)
    assert (cases, tiny, radix) == (GROUP_CASES, GROUP_CASES_TINY, GROUP_CASES_RADIX), (cases, tiny, radix)
    assert 4 * tiny <= cases
