"""CPU suite for IN (sub-query): both parsers with the switch on and off (the same statements accepted and refused, the same messages,
equal ADTs), the error cases of the ADT, the scratch table's sizing through its diagnostic export, the plain-Python evaluation the GPU
suites compare against (tests/int_in_query_util.py) on a case small enough to check by hand and against numpy, and the host decisions of
imm3_int_set_create under the address and undefined-behaviour sanitizers (tests/native/int_set_asan.cpp).  No device is touched."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import int_in_query_util as U
import stmt_fuzz_util as F
from immutable3_amd import native
from immutable3_amd import query as Q

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")


# ---- 1. both parsers ---------------------------------------------------------------------------------------------------------------
def inner(table, col, select=Q.NoSelect):
    return Q.IntInQuery(Q.Query(table, select, Q.Project([col])))


PARSED = [
    ("select a from t where x in (select id from c)", "Select(x,IntInQuery(Query(c,NoSelect,Project(List(id),0))))", Q.Select("x", inner("c", "id"))),
    ("select a from t where x in(select id from c where state = 'CA')", "Select(x,IntInQuery(Query(c,Select(state,Match(List(CA))),Project(List(id),0))))",
     Q.Select("x", inner("c", "id", Q.Select("state", Q.Match(["CA"]))))),
    ("select a, b from t where (x in (select id from c where (s = 'CA' and y > 3)) and a > 3) limit 4",
     "And(Select(x,IntInQuery(Query(c,And(Select(s,Match(List(CA))),Select(y,GT(3))),Project(List(id),0)))),Select(a,GT(3)))",
     Q.And(Q.Select("x", inner("c", "id", Q.And(Q.Select("s", Q.Match(["CA"])), Q.Select("y", Q.GT(3.0))))), Q.Select("a", Q.GT(3.0)))),
    ("select a from t where x in (select id from c where id in (select k from d where k < 9))",
     "Select(x,IntInQuery(Query(c,Select(id,IntInQuery(Query(d,Select(k,LT(9)),Project(List(k),0)))),Project(List(id),0))))",
     Q.Select("x", inner("c", "id", Q.Select("id", inner("d", "k", Q.Select("k", Q.LT(9.0))))))),
    ("select max(a) from t where (x in (select id from c) or s = 'NY') group by s",
     "Or(Select(x,IntInQuery(Query(c,NoSelect,Project(List(id),0)))),Select(s,Match(List(NY))))",
     Q.Or(Q.Select("x", inner("c", "id")), Q.Select("s", Q.Match(["NY"])))),
]
# what the inner statement cannot spell: a second column, an aggregate, a limit, an order, no table, no closing parenthesis
REFUSED = ["select a from t where x in (select id, k from c)", "select a from t where x in (select max(id) from c)", "select a from t where x in (select id from c limit 3)",
           "select a from t where x in (select id from c group by id)", "select a from t where x in (select id)", "select a from t where x in (select id from c",
           "select a from t where x in (select from c)", "select a from t where (x in (select id from c) and", "select a from t where x in select id from c"]


def cpp_parse(sql, *flags):
    return subprocess.run([BIN, "--parse-only", *flags, "-q", sql], capture_output=True, text=True, timeout=60)


def py_failure(sql, **flags):
    from immutable3_amd.sql import ParseError, SQLParser
    with pytest.raises(ParseError) as e:
        SQLParser.parseAll(sql, **flags)
    return str(e.value)


@pytest.mark.parametrize("sql,shown,select", PARSED)
def test_both_parsers_with_the_flag(sql, shown, select):
    """(fails without the feature: neither parser has the switch)"""
    from immutable3_amd.sql import SQLParser
    assert SQLParser.parseAll(sql, subqueries=True).select == select
    assert SQLParser.parseAll(sql, subqueries=True, int_lists=True).select == select
    p = cpp_parse(sql, "--subqueries")
    assert p.returncode == 0 and f",{shown},Project" in p.stdout, p.stdout
    assert cpp_parse(sql, "--subqueries", "--int-lists").stdout == p.stdout
    # with the flag off: the same failure, byte for byte, from both parsers -- the one the statement has always given
    off = cpp_parse(sql)
    assert off.returncode == 1 and off.stdout == py_failure(sql) + "\n" and "failure:" in off.stdout
    assert cpp_parse(sql, "--int-lists").stdout == py_failure(sql, int_lists=True) + "\n"


@pytest.mark.parametrize("sql", REFUSED)
def test_both_parsers_refuse_the_same(sql):
    msg = py_failure(sql, subqueries=True)
    p = cpp_parse(sql, "--subqueries")
    assert p.returncode == 1 and p.stdout == msg + "\n" and msg.endswith("\n\n" + sql)
    assert cpp_parse(sql).stdout == py_failure(sql) + "\n"
    assert cpp_parse(sql, "--subqueries", "--int-lists").stdout == py_failure(sql, subqueries=True, int_lists=True) + "\n"


def test_statements_without_a_sub_query_parse_the_same_either_way():
    from immutable3_amd.sql import SQLParser
    for sql in ("select id from t where (age > 18 and state = 'CA') limit 4", "select id from t where age < 7", "select max(age) from t where id > 3 group by state",
                "select id from t where inn = 3", "select id from t where in > 3", "select id from t where select = 3"):
        assert SQLParser.parseAll(sql, subqueries=True) == SQLParser.parseAll(sql)
        assert cpp_parse(sql, "--subqueries").stdout == cpp_parse(sql).stdout and cpp_parse(sql).returncode == 0
    assert SQLParser.parseAll("select id from t where id in (3, 4)", subqueries=True, int_lists=True).select == Q.Select("id", Q.IntIn([3, 4]))
    for sql in ("select id from t where age >", "select id from t where (age > 1 and", "select id from"):   # failures unrelated to sub-queries, flag off and on
        assert cpp_parse(sql).stdout == py_failure(sql) + "\n" and cpp_parse(sql, "--subqueries").stdout == py_failure(sql, subqueries=True) + "\n"


def test_the_generated_statements_round_trip_through_both_parsers():
    from immutable3_amd.sql import SQLParser
    db = {F.TABLE: F.make_rows(), U.ORDERS: U.make_orders()}
    spelled = 0
    for st in U.fixed_statements() + U.fuzz_statements(db):
        sql = U.to_sql(st)
        if sql is None:
            continue
        spelled += 1
        assert SQLParser.parseAll(sql, int_lists=True, subqueries=True) == U.to_query(st), sql
    assert spelled >= 40
    sql = U.to_sql(U.fixed_statements()[10])                                  # a sub-query in the sub-query: the C++ parser shows the same tree
    p = cpp_parse(sql, "--subqueries")
    assert p.returncode == 0 and "IntInQuery(Query(people,Select(id,IntInQuery(Query(orders,Select(qty,EQ(127)),Project(List(cust),0)))),Project(List(id),0)))" in p.stdout


# ---- 2. the ADT's error cases --------------------------------------------------------------------------------------------------------
def test_the_adt_refuses_what_is_no_plain_projection_of_one_column():
    ok = Q.Query("c", Q.NoSelect, Q.Project(["id"]))
    assert Q.IntInQuery(ok).query == ok and Q.IntInQuery(ok) == Q.IntInQuery(Q.Query("c", Q.NoSelect, Q.Project(["id"])))
    cases = [("not a query", "query"), (Q.Query("c", Q.NoSelect, Q.ProjectAgg([Q.Max("id")], [])), "agg"), (Q.Query("c", Q.NoSelect, Q.Project(["id", "k"])), "cols"),
             (Q.Query("c", Q.NoSelect, Q.Project([])), "cols"), (Q.Query("c", Q.NoSelect, Q.Project(["id"], 0, [("id", False)])), "order"),
             (Q.Query("c", Q.NoSelect, Q.Project(["id"], 5)), "limit")]
    for bad, which in cases:
        with pytest.raises(ValueError) as e:
            Q.IntInQuery(bad)
        assert str(e.value).startswith(Q.INT_IN_QUERY_ERRORS[which]), (which, str(e.value))


# ---- 3. the scratch table's sizing -----------------------------------------------------------------------------------------------------
def test_scratch_table_sizing():
    """(fails without the feature: the export does not exist)"""
    cap = native.INT_IN_MAX_VALUES
    f = native.plan_int_set_scratch_slots
    assert [f(0, 0, 9), f(5, 9, 0), f(3, 0, 9), f(8, 0, 100), f(9, 0, 100)] == [16, 16, 16, 16, 32]
    assert f(1 << 20, -3, 6) == 32                                            # the span bounds it: 10 values
    assert f(100, -(1 << 31), (1 << 31) - 1) == 256                           # the rows bound it
    assert f(1 << 40, -(1 << 31), (1 << 31) - 1) == 1 << 25 == f(cap, 0, cap - 1)   # the cap bounds it: the largest table
    assert f(1 << 40, -(1 << 31), (1 << 31) - 1, 16) == 32 and f(40, 0, 1000, 16) == 32   # a lowered cap (the overflow test's)
    assert f(5, 0, 9, -1) == -1 and f(5, 0, 9, cap + 1) == -1
    rng = np.random.default_rng(3)
    for _ in range(200):
        rows, lo = int(rng.integers(0, 1 << 26)), int(rng.integers(-(1 << 31), 1 << 31))
        hi = int(min((1 << 31) - 1, lo + int(rng.integers(0, 1 << 27))))
        n = min(rows, hi - lo + 1, cap)
        slots = f(rows, lo, hi)
        assert slots >= 16 and slots & (slots - 1) == 0 and slots >= 2 * n and (slots == 16 or slots < 4 * n), (rows, lo, hi)
        assert slots == U_slots(n)


def U_slots(n):
    import int_in_util
    return int_in_util.slots_for(n)


# ---- 4. the plain-Python evaluation ----------------------------------------------------------------------------------------------------
def test_plain_python_evaluation_of_in_query():
    db = {"c": [{"id": 1, "s": "CA"}, {"id": 2, "s": "NY"}, {"id": 3, "s": "CA"}, {"id": 3, "s": "TX"}],
          "o": [{"k": 10, "cust": 3, "qty": 5}, {"k": 11, "cust": 2, "qty": -128}, {"k": 12, "cust": 9, "qty": 1}, {"k": 13, "cust": 1, "qty": 0}, {"k": 14, "cust": 3, "qty": 7}]}
    ca = ("c", "id", [("s", "match", ["CA"])])
    assert U.inner_values(db, ca) == {1, 3}
    assert U.expected(db, ("o", [("cust", "inq", ca)], ["k"], 0)) == [(10,), (13,), (14,)]
    assert U.expected(db, ("o", [("cust", "inq", ca), ("qty", ">", 0)], ["k", "qty"], 0)) == [(10, 5), (14, 7)]
    assert U.expected(db, ("o", [("cust", "inq", ca)], ["k"], 2)) == [(10,), (13,)]
    assert U.expected(db, ("o", [("cust", "inq", ("c", "id", [("s", "match", ["ZZ"])]))], ["k"], 0)) == []               # the empty set
    assert U.expected(db, ("o", [("cust", "inq", ("c", "id", []))], ["k"], 0)) == [(10,), (11,), (13,), (14,)]              # every inner row
    assert U.expected(db, ("o", [("qty", ">", 128)], ["k"], 0)) == [(10,), (12,), (13,), (14,)]                             # d.toByte: qty > -128
    nested = ("c", "id", [("id", "inq", ("o", "cust", [("qty", ">", 4)]))])
    assert U.inner_values(db, nested) == {3} and U.expected(db, ("o", [("cust", "inq", nested)], ["k"], 0)) == [(10,), (14,)]
    big = {F.TABLE: F.make_rows(), U.ORDERS: U.make_orders()}                  # ... and against numpy on the suites' own tables
    ids = np.array([r["id"] for r in big[F.TABLE] if r["state"] == "CA"])
    cust = np.array([r["cust"] for r in big[U.ORDERS]])
    oid = np.array([r["order_id"] for r in big[U.ORDERS]])
    st = U.fixed_statements()[0]
    assert [t[0] for t in U.expected(big, st)] == oid[np.isin(cust, ids)].tolist() and 0 < np.isin(cust, ids).sum() < cust.size
    assert all(U.one_set_per_column(s) for s in U.fuzz_statements(big)) and len(U.fuzz_statements(big)) == 50


# ---- 5. the host unit alone under the sanitizers -------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_set_plan_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "int_set_asan")
    csrc = os.path.join(ROOT, "immutable3_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "int_set_asan.cpp"), os.path.join(csrc, "imm3_int_set_plan.cpp"), os.path.join(csrc, "imm3_int_list_plan.cpp"),
                           "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 25 and all(ln.endswith(" ok") for ln in lines), r.stdout
