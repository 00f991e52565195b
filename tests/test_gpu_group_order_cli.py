"""GPU suite: ORDER BY over groups through the C++ host layer -- imm3_sql --order-by over the loader-made tables of
test_gpu_group_order_engine.py.  The ordered table query (blocks of 1024 rows) and the per-segment fallback with its host ordering
(blocks of 1000 rows) must print the same rows, in the order the plain-Python expectation gives; a limit cuts after the order."""
import os
import subprocess

import pytest

from immutable3_amd.operators import java_double_to_string
from test_gpu_group_order_engine import BIN, CASES, expected, tables  # noqa: F401  (tables: the module's fixture)

pytestmark = pytest.mark.gpu


def sql_of(aggs, group, order_by, limit, where=""):
    s = "select " + ", ".join(f"{k}({c})" for (k, c) in aggs) + " from people" + where
    if group:
        s += " group by " + ", ".join(group)
    if order_by:
        s += " order by " + ", ".join(f"{n} {'desc' if d else 'asc'}" for (n, d) in order_by)
    if limit:
        s += f" limit {limit}"
    return s


def rows_of(want, aggs):
    """Row(...) of the aggregators' repr in SELECT-list order: counts and strings as they are, numeric maxima / minima as Double.toString"""
    out = []
    for (_, m) in want:
        xs = []
        for (kind, c) in aggs:
            v = m[f"{c}_{kind}"]
            xs.append(str(v) if kind == "count" or isinstance(v, str) else java_double_to_string(float(v)))
        out.append("Row(" + ",".join(xs) + ")")
    return out


def run_sql(sql, d):
    p = subprocess.run([os.path.join(BIN, "imm3_sql"), "--order-by", "--explain", "-q", sql, "-d", d], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout.splitlines(), p.stderr


@pytest.mark.parametrize("case", range(len(CASES)))
def test_table_query_and_fallback_print_the_same_rows(tables, case):  # noqa: F811
    rows, dirs = tables
    aggs, group, order_by, limit = CASES[case]
    want = rows_of(expected(rows, aggs, group, order_by, limit), aggs)
    sql = sql_of(aggs, group, order_by, limit)
    got, err = run_sql(sql, dirs[1024])
    assert "path: one table query" in err and got == want, sql
    got, err = run_sql(sql, dirs[1000])
    assert "path: per-segment queries" in err and got == want, sql


def test_aggregate_call_as_key_and_a_where_clause(tables):  # noqa: F811
    rows, dirs = tables
    aggs, group = [("count", "id"), ("max", "age")], ["state"]
    want = rows_of(expected(rows, aggs, group, [("id_count", True), ("state", True)], 6, keep=lambda r: r["age"] > 0), aggs)
    sql = "select count(id), max(age) from people where age > 0 group by state order by count(id) desc, state desc limit 6"
    for block in (1024, 1000):
        assert run_sql(sql, dirs[block])[0] == want, block
