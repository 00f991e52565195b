"""CPU census of the table fuzz (table_fuzz_util.py, test_gpu_fuzz_table.py): the generator run over every seed the GPU tests use,
without a device.  It asserts that the fuzz is not hollow -- every shape, codec, limit position, selectivity, aggregate and tree kind
the GPU tests are there for really occurs -- so that a later change to a default cannot empty it, and it runs the oracle-only half of
every case here, where a case the oracle itself rejects shows up before it reaches a GPU."""
import numpy as np
import pytest

import table_fuzz_util as U
from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, MATCH
from immutable3_amd import native

VALUE_CODECS = [DENSE_INT, DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING]


def check_table(t):
    assert 1 <= len(t.seg_rows) and all(U.layout_ok(br) and sum(br) == n for br, n in zip(t.layouts, t.seg_rows)), t.describe()
    assert all(len(cols) == 5 for cols in t.segs) and all(d.shape[0] == t.n_rows for d in t.data)
    for c, k in enumerate(t.codecs):
        assert k in U.CODECS_OF[c]
        if k == U.SNAPPY:
            assert max([max(br) for br in t.layouts if br], default=0) * t.widths[c] <= U.SNAPPY_MAX_BLOCK_BYTES


@pytest.fixture(scope="module")
def select_census(oracle):
    """every table and flat query of test_fuzz_table_select_project, with the oracle's per-segment results"""
    tables, queries = [], []
    for seed in range(U.SELECT_SEEDS):
        for t, qs in U.select_cases(seed):
            tables.append(t)
            for fq in qs:
                queries.append((t, fq, U.Expected(oracle, t, fq.used, fq.sels, fq.proj)))
    return tables, queries


def test_tables_keep_the_layout_rule_and_cover_the_shapes(select_census):
    tables, _ = select_census
    assert len(tables) == U.SELECT_SEEDS * U.SELECT_TABLES
    for t in tables:
        check_table(t)
        assert 1 <= len(t.seg_rows) <= 6 and set(t.seg_rows) <= set(U.SEG_ROWS) and t.n_rows <= 150_000
    assert {len(t.seg_rows) for t in tables} == set(range(1, 7))
    assert {n for t in tables for n in t.seg_rows} == set(U.SEG_ROWS)
    assert 3 * sum(U.has_tiny_before_last(t.seg_rows) for t in tables) >= len(tables)          # at least one table in three
    assert any(0 in t.seg_rows[1:-1] for t in tables)                                           # an empty segment in the middle
    layouts = [br for t in tables for br in t.layouts if br]
    assert any(U.is_quirk(br) for br in layouts)                                                # the loader's shape
    assert any(len(set(br[:-1])) > 1 for br in layouts)                                         # mixed
    assert {br[0] for br in layouts if len(br) > 1 and len(set(br[:-1])) == 1} >= {64, 128, 512, 1024}
    assert any(br[-1] % 64 for br in layouts if len(br) > 1)                                    # a ragged last block behind full ones
    for c in range(5):                                                                          # every codec on every column that can carry it
        assert {t.codecs[c] for t in tables} == set(U.CODECS_OF[c]), U.COLUMN_NAMES[c]
    assert {t.name_width for t in tables} == {8, 16}
    assert {t.ascending_id for t in tables} == {True, False}


def test_flat_queries_cover_limits_selectivities_and_predicates(select_census):
    _, queries = select_census
    seen = set()
    for t, fq, e in queries:
        assert 1 <= len(fq.used) <= 5 and len(set(fq.used)) == len(fq.used)
        for j in range(len(fq.used)):
            assert sum(s[0] == j for s in fq.sels) <= 2
        for _, cond, operand in fq.sels:
            if cond == MATCH:
                assert operand and len({len(v) for v in operand}) == 1
        assert all(len(s[2]) <= 8 for s in fq.sels if s[1] == MATCH and fq.used[s[0]] == U.STATE)
        if len(set(fq.proj)) < len(fq.proj):
            seen.add("a repeated SELECT column")
        if fq.reserve is not None:
            seen.add("a reservation too small" if fq.reserve < e.total else "a reservation")
        if t.n_rows and e.total == 0:
            seen.add("selectivity 0")
        if t.n_rows and e.total == t.n_rows and fq.sels:
            seen.add("selectivity 1")
        if any(s[1] == MATCH and fq.used[s[0]] == U.NAME for s in fq.sels):
            seen.add("a wide Match")
            names = {bytes(r) for r in np.unique(t.data[U.NAME], axis=0)} if t.n_rows else set()
            for s in fq.sels:
                if s[1] == MATCH and fq.used[s[0]] == U.NAME and names:
                    if any(v not in names for v in s[2]):
                        seen.add("a wide Match value in no row")
                    if any(v not in names and any(v[:-1] == n[:-1] for n in names) for v in s[2]):
                        seen.add("a wide Match value that shares a prefix")
        nonempty = [si for si, c in enumerate(e.counts) if c > 0]
        for kind in fq.limit_kinds:
            limit = U.limit_of(kind, e.counts)
            seen.add("limit " + kind)
            if limit > 0 and len(nonempty) >= 2 and limit == e.counts[nonempty[0]]:
                seen.add("a limit exactly on a segment boundary")
            if limit > 0 and len(nonempty) >= 2 and e.total - e.counts[nonempty[-1]] < limit <= e.total:
                seen.add("a limit reached only in the last segment")
            if limit > 0 and limit == e.total:
                seen.add("a limit equal to the total")
            if limit > 0 and any(n <= 1 for n in t.seg_rows[:-1]) and limit < e.total:
                seen.add("a cut in a table with a tiny segment")
    want = {"a repeated SELECT column", "a reservation too small", "a reservation", "selectivity 0", "selectivity 1", "a wide Match",
            "a wide Match value in no row", "a wide Match value that shares a prefix", "a limit exactly on a segment boundary",
            "a limit reached only in the last segment", "a limit equal to the total", "a cut in a table with a tiny segment"}
    want |= {"limit " + k for k in U.LIMIT_KINDS}
    assert want <= seen, want - seen


LIMIT_CASES_THAT_STOP = 66      # of the 96 cases of test_fuzz_table_limit_stops_right: all but the 5 seeds x 6 with a wide Match


def test_limit_tables_and_which_of_their_cases_stop(oracle):
    grids, compressed, wide = set(), 0, 0
    stop, stop_on = 0, set()
    placed = {}
    for seed in range(U.LIMIT_SEEDS):
        rng = U.limit_rng(seed)
        t, G = U.random_limit_table(rng, seed)
        check_table(t)
        grids.add(G)
        assert 10 <= len(t.seg_rows) <= 16 and set(t.seg_rows) <= set(U.LIMIT_SEG_ROWS) and len(set(t.seg_rows)) >= 4
        # (G = 5 needs more than 160 tiles: only those tables pass 150 000 rows -- table_fuzz_util.limit_table_shape)
        assert sum(t.tiles) > G * native.TABLE_LIMIT_CLAIM_TILES and t.n_rows <= (170_000 if G == 5 else 150_000)
        assert 0 in t.seg_rows[1:-1] and 1 in t.seg_rows[1:-1]
        compressed += t.codecs[U.ID] != U.DENSE
        cases = U.limit_cases(rng, t, seed)
        wide += any(fq_used[-1] == U.NAME for _, fq_used, _, _ in cases)
        for what, used, sels, proj in cases:
            # the library's own plan: the stopping launch for a chain of one tile pass, the whole select behind a wide Match
            stops = U.limit_case_stops(used, sels)
            assert native.plan_table_limit(limit=10, single_tile_pass=int(stops), n_tiles=sum(t.tiles), grid=G) == int(stops)
            if stops:
                stop += 1
                stop_on.add(t.codecs[used[sels[0][0]]])
            e = U.Expected(oracle, t, used, sels, proj)
            where = t.starts[e.seg] + e.row
            key = what.split(",")[0]
            placed.setdefault(key, []).append((t, e, where))
            if key == "from the first tile":
                assert e.total and where[0] < 1024
            elif key == "only in the last third":
                assert e.total == 0 or where[0] > 2 * t.n_rows // 3
            elif key == "from one row before a segment's end":
                assert e.total == 0 or (e.row[0] == t.seg_rows[e.seg[0]] - 1 or "Match" in what)
            elif key == "only in one-row segments":
                assert all(t.seg_rows[s] == 1 for s in e.seg)
            elif key == "sparse":
                assert e.total <= t.n_rows // 50
            else:
                assert e.total == 0
    assert grids == {1, 2, 3, 5}
    # a later change to the generator (or to what vetoes the stopping launch) cannot hollow the fuzzer out unnoticed: the cases that
    # stop are counted, and predicate columns of every codec are among them
    assert stop == LIMIT_CASES_THAT_STOP and stop_on == {U.DENSE, U.PFOR, U.SNAPPY}, (stop, stop_on)
    assert 3 * compressed >= U.LIMIT_SEEDS - 2 and 3 * wide >= U.LIMIT_SEEDS - 2                 # one seed in three each
    assert len(placed) == 6
    assert any(e.total for _, e, _ in placed["only in one-row segments"]) and any(e.total for _, e, _ in placed["sparse"])
    # a survivor run that starts on a segment's last row and goes on behind an empty or one-row segment
    assert any(e.total and any(n <= 1 for n in t.seg_rows[e.seg[0]:]) for t, e, _ in placed["from one row before a segment's end"])


def test_group_queries_cover_the_aggregates_and_agree_with_oracle_np(oracle):
    kinds, seen, groups_seen_late = set(), set(), 0
    for seed in range(U.GROUP_SEEDS):
        for t, qs in U.group_cases(seed):
            check_table(t)
            for aq in qs:
                e = U.Expected(oracle, t, aq.used, aq.sels, [0])
                got = U.expected_groups(t, aq, e.keep(t))
                assert sum(got[2]) == e.total
                kinds |= {k for k, _ in aq.aggs}
                assert 1 <= len(aq.aggs) <= 4
                for k, j in aq.aggs:
                    c = aq.used[j]
                    assert not (c in (U.STATE, U.NAME) and k in ("min", "sum"))
                    if c in (U.STATE, U.NAME) and k == "max":
                        seen.add("a string max" if c == U.STATE else "a wide string max")
                if aq.wide_keys:
                    seen.add("wide keys")
                if any(aq.used[j] == U.NAME for j in aq.group):
                    assert aq.wide_keys
                    seen.add("name as a group key")
                if not aq.group:
                    seen.add("no group column")
                if len(got[2]) > 1 and (np.diff(np.searchsorted(t.starts, got[1], side="right")) > 0).any():
                    groups_seen_late += 1                                     # groups first seen in different segments
                # the two references against each other, for the aggregates oracle_np knows
                if "sum" not in {k for k, _ in aq.aggs} and e.total <= 30_000:
                    seen.add("held against oracle_np")
                    assert U.as_oracle_np(t, aq, got) == U.oracle_np_groups(t, aq), (seed, aq.group, aq.aggs)
    assert kinds == {"count", "min", "max", "sum"}
    assert seen == {"a string max", "a wide string max", "wide keys", "name as a group key", "no group column", "held against oracle_np"}
    assert groups_seen_late >= 10


def test_tree_seed_keeps_the_table_refusals_within_a_quarter():
    tables, cases = U.tree_cases()
    assert len(cases) == U.TREE_COUNT == 40 and len(tables) == U.TREE_TABLES
    refused = with_not = with_or = limited = 0
    for ti, leaves, tree, proj, limit_kind in cases:
        t = tables[ti]
        check_table(t)
        terms = native.expr_normalize(VALUE_CODECS, t.widths, leaves, U.postfix(tree))
        refused += U.tree_is_refused(t, tree, terms)
        with_not += U.has_not(tree)
        with_or += U.has_or_or_not(tree)
        limited += limit_kind in ("one", "half")
        words, keep = U.tree_keep(t, leaves, tree)                            # (the oracle-only half of the GPU test)
        assert keep.size == t.n_rows and sum(w.size for w in words) == sum(-(-b // 64) for br in t.layouts for b in br)
    assert refused == U.TREE_REFUSED and 4 * refused <= U.TREE_COUNT
    assert 2 * with_not >= U.TREE_COUNT and with_or >= with_not and limited >= 8
    assert any(0 in t.seg_rows[:-1] for t in tables) and any(1 in t.seg_rows[:-1] for t in tables)
    assert any(k != U.DENSE for t in tables for k in t.codecs)
