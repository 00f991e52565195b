"""GPU suite: HAVING through the engines, over the loader-made tables of test_gpu_group_order_engine.py (three small segments).  The same
statement through the one-table-query path (blocks of 1024 rows: filter, order and limit on the device), the per-segment path (blocks of
1000 rows: merged groups filtered and ordered on the host) and device_merge=True must give identical groups, equal to a plain-Python
expectation over the rows; imm3_sql --having --order-by prints the same rows on both of its paths, and without --having it gives the
parse failure it has always given.  An AvgDoubleAggr's alias -- the operator level's HAVING on an average -- runs on both paths too."""
import os
import subprocess

import pytest

from immutable3_amd import Count, Max, Min, NoSelect, ProjectAgg, Query, Select
from immutable3_amd.query import EQ, GT, LT, And, Or
from test_gpu_group_order_cli import rows_of
from test_gpu_group_order_engine import BIN, as_plain, tables  # noqa: F401  (tables: that module's fixture)

pytestmark = pytest.mark.gpu

# (aggregates as (kind, column), group by, having as nested tuples, its SQL, order by, limit)
CASES = [
    ([("count", "id"), ("max", "age")], ["state"], ("id_count", ">", 420), "id_count > 420", [("id_count", True)], 3),
    ([("count", "id"), ("max", "age")], ["state"], ("id_count", "<", 420), "count(id) < 420", [], 0),
    ([("count", "id"), ("min", "id")], ["state", "age"], ("and", ("id_count", ">", 55), ("id_min", "<", 0)), "(id_count > 55 and min(id) < 0)",
     [("age", True), ("id_count", False)], 7),
    ([("count", "id"), ("min", "id"), ("max", "id")], ["state"],
     ("or", ("and", ("id_max", "<", 4895), ("id_count", ">", 420)), ("or", ("id_max", "=", 4899), ("id_count", "<", 400))),
     "((id_max < 4895 and id_count > 420) or (max(id) = 4899 or id_count < 400))", [("state", True)], 0),
    ([("max", "name"), ("count", "id")], ["state"], ("id_count", ">", 410), "id_count > 410", [("name_max", True)], 0),
    ([("count", "id")], ["state"], ("id_count", ">", 100000), "id_count > 100000", [("id_count", True)], 5),     # keeps nothing
    ([("count", "id")], ["state"], ("id_count", ">", 400), "id_count > 400", [], 4),                            # a limit without an order
    # a count over a STRING column is a count: the table path's filter refused it as a string maximum (pinned from the statement fuzz)
    ([("count", "name"), ("count", "id"), ("max", "name")], ["state"], ("name_count", ">", 420), "count(name) > 420", [("name_count", True)], 0),
]


def holds(h, g):
    if h[0] in ("and", "or"):
        a, b = holds(h[1], g), holds(h[2], g)
        return (a and b) if h[0] == "and" else (a or b)
    v = g[h[0]]
    return v > h[2] if h[1] == ">" else (v < h[2] if h[1] == "<" else v == h[2])


def adt(h):
    if h[0] in ("and", "or"):
        return (And if h[0] == "and" else Or)(adt(h[1]), adt(h[2]))
    return Select(h[0], {">": GT, "<": LT, "=": EQ}[h[1]](float(h[2])))


def expected(rows, aggs, group, having, order_by, limit):
    """[(group key, {alias: value})]: the groups in first-seen order, the ones `having` keeps, stable sorts from the least significant
    key up, the limit.  The key joins the group columns in batch-column order (the aggregates' columns, then the group-by columns)."""
    used = []
    for c in [c for (_, c) in aggs] + list(group):
        if c not in used:
            used.append(c)
    gcols = [c for c in used if c in group]
    groups, cols = {}, {}
    for r in rows:
        key = "_".join(str(r[c]) for c in gcols)
        g = groups.setdefault(key, {})
        cols.setdefault(key, {c: r[c] for c in gcols})
        for (kind, c) in aggs:
            alias = f"{c}_{kind}"
            g[alias] = g.get(alias, 0) + 1 if kind == "count" else (max if kind == "max" else min)(g.get(alias, r[c]), r[c])
    order = [k for k in groups if holds(having, groups[k])]
    for (name, desc) in reversed(order_by):
        order.sort(key=lambda k: cols[k][name] if name in cols[k] else groups[k][name], reverse=desc)
    if limit > 0:
        order = order[:limit]
    return [(k, groups[k]) for k in order]


def mk_query(aggs, group, having, order_by, limit):
    mk = {"count": Count, "max": Max, "min": Min}
    return Query("people", NoSelect, ProjectAgg([mk[k](c) for (k, c) in aggs], group, order_by, limit, having=adt(having)))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_three_paths_agree(tables, case):  # noqa: F811
    from immutable3_amd.operators import Engine, GpuSegmentManager
    from immutable3_amd.storage import SegmentManager
    rows, dirs = tables
    aggs, group, having, _, order_by, limit = CASES[case]
    want = expected(rows, aggs, group, having, order_by, limit)
    every = expected(rows, aggs, group, ("id_count", ">", 0), order_by, 0)
    assert len(want) < len(every) and (len(want) > 1 or case == 5)
    for block, device_merge in ((1024, False), (1000, False), (1000, True)):
        gsm = GpuSegmentManager(SegmentManager(dirs[block]))
        try:
            assert (gsm.device_table("people") is not None) == (block == 1024)
            got = Engine(gsm, device_merge=device_merge).execute_agg(mk_query(aggs, group, having, order_by, limit))
            assert as_plain(got) == want, (block, device_merge)
        finally:
            gsm.close()


def test_having_on_an_average_at_the_operator_level(tables):  # noqa: F811
    """ProjectAggOp with an AvgDoubleAggr: its alias becomes an `average` leaf on the SUM -- on the device for the table query, in
    filter_groups for merged per-segment groups.  avg(age) < 0 and avg(age) > -1/5 as exact rationals."""
    from fractions import Fraction
    from immutable3_amd.operators import AvgDoubleAggr, CountAggr, Engine, GpuSegmentManager, ProjectAggOp, ScanOp, filter_groups
    from immutable3_amd.storage import SegmentManager
    rows, dirs = tables
    sums = {}
    for r in rows:
        s = sums.setdefault(r["state"], [0, 0])
        s[0] += r["age"]
        s[1] += 1
    for having, keep in ((Select("age_avg", LT(0.0)), lambda s, n: Fraction(s, n) < 0), (Select("age_avg", GT(0.0)), lambda s, n: Fraction(s, n) > 0),
                         (Or(Select("age_avg", EQ(0.0)), And(Select("age_avg", GT(-1.0)), Select("id_count", GT(425)))), lambda s, n: s == 0 or (Fraction(s, n) > -1 and n > 425))):
        want = [(k, {"age_avg": tuple(v), "id_count": v[1]}) for k, v in sums.items() if keep(*v)]
        assert 0 < len(want) < len(sums)
        aggs = [AvgDoubleAggr("age", "age_avg"), CountAggr("id", "id_count")]
        gsm = GpuSegmentManager(SegmentManager(dirs[1024]))
        try:
            dt, used, used_idx, sels, prog = Engine(gsm)._table_plan(Query("people", NoSelect, ProjectAgg([Max("age"), Count("id")], ["state"])))
            op = ProjectAggOp(aggs, ScanOp(gsm, 0, "people", used), ["state"], having=having)
            got = dict(op._run(dt, used, used_idx, sels, gsm.getTable("people").blockSize, prog, ordered=True))
            assert as_plain(got) == want
            merged = {}
            for seg in range(3):
                for k, m in ProjectAggOp(aggs, ScanOp(gsm, seg, "people", used), ["state"], having=having).iterator():
                    if k in merged:
                        for alias in m:
                            merged[k][alias].combine(m[alias])
                    else:
                        merged[k] = m
            assert len(merged) == len(sums)                    # a segment's own iterator does not filter: its groups are partial
            assert as_plain(filter_groups(merged, op.filter_leaves, op.filter_prog)) == want
        finally:
            gsm.close()


def run_sql(sql, d, *flags):
    return subprocess.run([os.path.join(BIN, "imm3_sql"), *flags, "--explain", "-q", sql, "-d", d], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_cli_prints_the_same_rows_on_both_paths(tables, case):  # noqa: F811
    rows, dirs = tables
    aggs, group, having, hsql, order_by, limit = CASES[case]
    want = rows_of(expected(rows, aggs, group, having, order_by, limit), aggs)
    sql = "select " + ", ".join(f"{k}({c})" for (k, c) in aggs) + " from people group by " + ", ".join(group) + " having " + hsql
    if order_by:
        sql += " order by " + ", ".join(f"{n} {'desc' if d else 'asc'}" for (n, d) in order_by)
    if limit:
        sql += f" limit {limit}"
    for block, path in ((1024, "path: one table query"), (1000, "path: per-segment queries")):
        p = run_sql(sql, dirs[block], "--having", "--order-by")
        assert p.returncode == 0, p.stdout + p.stderr
        assert path in p.stderr and p.stdout.splitlines() == want, (sql, block)
    for flags in ((), ("--order-by",)):                       # without the flag: the parse failure of the parent commit, nothing runs
        p = run_sql(sql, dirs[1024], *flags)
        assert p.returncode == 1 and p.stdout == f"[1.{sql.index(' having ') + 2}] failure: end of input expected\n\n{sql}\n"
