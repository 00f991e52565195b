"""COUNT(DISTINCT), the host side (no GPU): the sizing of the pair set (imm3_plan_distinct_capacity), the parser flag in both parsers
and what stays the same with it off, the ADT and the aggregator with their alias defaults, the engines' refusal decided from plain
facts, and the sizing unit alone under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

from immutable3_amd import native
from immutable3_amd import query as Q
from immutable3_amd.sql import ParseError, SQLParser
from test_group_filter_host import PARSED as HAVING_CORPUS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")


# ---- 1. the capacity of the pair set -----------------------------------------------------------------------------------------------
def model(rows, key_bytes, width):
    """the power of two at or above 2 x min(rows, min(rows, 256^key_bytes) x 256^width), at least 1024; -1 above 2^28"""
    r = max(rows, 1)
    pairs = min(r, min(r, 256 ** key_bytes) * 256 ** width)
    cap = 1024
    while cap < 2 * pairs:
        cap *= 2
    return cap if cap <= 2 ** 28 else -1


def test_capacity_minimum_powers_of_two_and_the_refusal():
    cap = native.plan_distinct_capacity
    for width in (1, 2, 3, 4):
        assert cap(0, 0, width) == cap(1, 2, width) == cap(512, 8, width) == 1024           # the minimum
        assert cap(513, 8, width) == 2048
        for rows in (1, 100, 511, 512, 513, 1023, 1024, 1025, 70_000, 10 ** 8, 2 ** 27 - 1, 2 ** 27, 2 ** 27 + 1, 2 ** 31, 2 ** 40):
            for key_bytes in (0, 1, 2, 3, 4, 8, 16, 256):
                got = cap(rows, key_bytes, width)
                assert got == model(rows, key_bytes, width), (rows, key_bytes, width)
                assert got == -1 or (got >= 1024 and got & (got - 1) == 0 and got <= 2 ** 28)
    # no group column: one group, so the value domain bounds the set -- 256 values of an int8 column, whatever the rows
    assert cap(10 ** 8, 0, 1) == 1024 and cap(10 ** 8, 0, 2) == 2 ** 17
    # the README shapes: count(distinct age) group by state (int8 under a 2-byte key), count(distinct id) (int32: bounded by the rows)
    assert cap(10 ** 8, 2, 1) == 2 ** 25 and cap(10 ** 8, 2, 4) == 2 ** 28
    # 2^28 entries is the most: more than 2^27 pairs are refused
    assert cap(2 ** 27, 8, 4) == 2 ** 28 and cap(2 ** 27 + 1, 8, 4) == -1 and cap(2 ** 27 + 1, 2, 1) == 2 ** 25
    for bad in ((-1, 2, 1), (10, -1, 1), (10, 2, 0), (10, 2, 5)):
        assert cap(*bad) == -2


# ---- 2. both parsers ---------------------------------------------------------------------------------------------------------------
def cpp_parse(sql, *flags):
    return subprocess.run([BIN, "--parse-only", *flags, "-q", sql], capture_output=True, text=True, timeout=60)


WITH_FLAG = [   # (statement, aggregates, the flags it needs besides, the ProjectAgg's tail as imm3_sql prints it)
    ("select count(distinct age) from t", [Q.CountDistinct("age")], {}, "List(CountDistinct(age,None)),List())"),
    ("select state, count(distinct age) from t group by state", None, {}, None),          # (no plain column stands in an aggregation's list)
    ("select count(distinct age), count(id) from t group by state", [Q.CountDistinct("age"), Q.Count("id")], {},
     "List(CountDistinct(age,None), Count(id,None)),List(state))"),
    ("select count( distinct  age ),max(age) from t where age > 3 group by state", [Q.CountDistinct("age"), Q.Max("age")], {},
     "List(CountDistinct(age,None), Max(age,None)),List(state))"),
    ("select count(distinct age), count(id) from t group by state having count(distinct age) > 3 order by count(distinct age) desc, state limit 2",
     [Q.CountDistinct("age"), Q.Count("id")], {"group_order": True, "having": True},
     "List(CountDistinct(age,None), Count(id,None)),List(state),List((age_distinct,desc), (state,asc)),2,Some(Select(age_distinct,GT(3))))"),
    ("select count(distinct) from t", [Q.Count("distinct")], {}, "List(Count(distinct,None)),List())"),      # a column called `distinct`
    ("select count(distinctx) from t", [Q.CountDistinct("x")], {}, "List(CountDistinct(x,None)),List())"),   # literals match as prefixes
]


@pytest.mark.parametrize("sql,aggs,flags,tail", WITH_FLAG)
def test_both_parsers_with_the_flag(sql, aggs, flags, tail):
    cflags = ["--count-distinct"] + (["--order-by"] if flags.get("group_order") else []) + (["--having"] if flags.get("having") else [])
    if aggs is None:
        with pytest.raises((ParseError, ValueError)):
            SQLParser.parseAll(sql, count_distinct=True, group_order=True, having=True)
        assert cpp_parse(sql, "--count-distinct", "--order-by", "--having").returncode == 1
        return
    q = SQLParser.parseAll(sql, count_distinct=True, **flags)
    assert isinstance(q.project, Q.ProjectAgg) and list(q.project.aggs) == aggs
    p = cpp_parse(sql, *cflags)
    assert p.returncode == 0 and p.stdout.strip().endswith("ProjectAgg(" + tail + ")"), p.stdout


@pytest.mark.parametrize("sql", [s for (s, a, *_rest) in WITH_FLAG if a is not None and any(isinstance(x, Q.CountDistinct) for x in a)])
def test_flag_off_is_the_failure_it_has_always_been(sql):
    """`count` `(` ident -- the ident being `distinct...` -- and then `)' is expected where the column's name stands"""
    if sql == "select count(distinctx) from t":          # without the flag this one is a count of a column called distinctx
        assert list(SQLParser.parseAll(sql).project.aggs) == [Q.Count("distinctx")]
        assert "Count(distinctx,None)" in cpp_parse(sql).stdout
        return
    head = sql.index("distinct") + len("distinct")
    at = head + (len(sql[head:]) - len(sql[head:].lstrip())) + 1
    want = f"[1.{at}] failure: `)' expected\n\n{sql}"
    for flags in ({}, {"count_distinct": False}, {"group_order": True, "having": True, "order_by": True, "string_ranges": True}):
        with pytest.raises(ParseError) as e:
            SQLParser.parseAll(sql, **flags)
        assert str(e.value) == want
    for flags in ((), ("--order-by", "--having", "--string-ranges")):
        p = cpp_parse(sql, *flags)
        assert p.returncode == 1 and p.stdout == want + "\n"


OTHER_STATEMENTS = ["select id, age from t where (age > 18 and age < 30) limit 10", "select count(id), max(age), min(state) from t group by state",
                    "select sum(id) from t", "select count(id) from t where state = 'CA'", "select id from t where (age > 3 or age < 1) order by id desc limit 3",
                    "select count(id) from t group by state order by count(id) desc limit 3", "select count(distinct) from t"]


@pytest.mark.parametrize("sql", [s for (s, *_rest) in HAVING_CORPUS] + OTHER_STATEMENTS)
def test_statements_without_the_call_parse_the_same_either_way(sql):
    flags = dict(order_by=True, string_ranges=True, group_order=True, having=True)
    assert SQLParser.parseAll(sql, count_distinct=True, **flags) == SQLParser.parseAll(sql, **flags)
    a, b = cpp_parse(sql, "--order-by", "--having", "--string-ranges", "--count-distinct"), cpp_parse(sql, "--order-by", "--having", "--string-ranges")
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout


# ---- 3. the ADT, the aggregator, the aliases ----------------------------------------------------------------------------------------
def test_adt_aggregator_and_alias_defaults():
    from immutable3_amd.operators import Aggregator, CountAggr, CountDistinctAggr, resolveProjectOp
    assert native.AGG_COUNT_DISTINCT == 5 and native.AGG_COUNT_DISTINCT not in (native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM, 4, 9)
    assert Q.default_alias(Q.CountDistinct("age")) == "age_distinct" and Q.default_alias(Q.CountDistinct("age", "ages")) == "ages"
    assert Q.default_alias(Q.Count("age")) == "age_count"                               # (untouched)
    a = CountDistinctAggr("age", "age_distinct")
    assert isinstance(a, Aggregator) and not isinstance(a, CountAggr) and a.kind == native.AGG_COUNT_DISTINCT
    a.set(7)
    assert a.get() == 7 and a.repr() == "7" and a.make().get() == 0
    with pytest.raises(Exception, match="count\\(distinct\\) runs as one table query only"):
        a.combine(CountDistinctAggr("age", "age_distinct"))
    # an order key and a having leaf by the default alias: ProjectAgg's own checks take them
    p = Q.ProjectAgg([Q.CountDistinct("age"), Q.Count("id")], ["state"], [("age_distinct", True)], 3, having=Q.Select("age_distinct", Q.GT(2.0)))
    assert p.order_by == (("age_distinct", True),)
    with pytest.raises(ValueError, match="age_count"):
        Q.ProjectAgg([Q.CountDistinct("age")], ["state"], [("age_count", True)])

    class T:                                                                            # what resolveProjectOp reads of a table
        def getColumn(self, name):
            raise AssertionError("a count(distinct) does not ask for its column's type")
    op = resolveProjectOp(Q.ProjectAgg([Q.CountDistinct("age"), Q.CountDistinct("state", "s")], ["state"]), T())(None)
    assert [(type(x), x.col, x.alias) for x in op.aggs] == [(CountDistinctAggr, "age", "age_distinct"), (CountDistinctAggr, "state", "s")]
    with pytest.raises(Exception, match="Unknown Aggregate type"):                       # Sum and Avg: untouched
        resolveProjectOp(Q.ProjectAgg([Q.Sum("age")], []), T())


# ---- 4. the engines' refusal, from plain facts ---------------------------------------------------------------------------------------
def test_route_and_refusal_text():
    from immutable3_amd.operators import COUNT_DISTINCT_ONE_QUERY, count_distinct_route
    assert COUNT_DISTINCT_ONE_QUERY == "count(distinct) runs as one table query only"
    route = count_distinct_route
    # ONE table query answers whatever else holds; a statement without the aggregate may always merge
    for dm in (False, True):
        for nctx in (1, 2):
            assert route(True, True, 3, dm, nctx) == "table" and route(False, True, 3, dm, nctx) == "table"
            assert route(False, False, 3, dm, nctx) == "merge"
    assert route(True, False, 1, False, 1) == "segment" and route(True, False, 0, False, 1) == "segment" and route(True, False, 1, False, 2) == "segment"
    for args, word in (((True, False, 3, False, 1), "3 segments"), ((True, False, 1, True, 1), "device_merge"), ((True, False, 3, True, 2), "device_merge"),
                       ((True, False, 2, False, 2), "2 contexts")):
        with pytest.raises(Exception) as e:
            route(*args)
        assert str(e.value).startswith(COUNT_DISTINCT_ONE_QUERY) and word in str(e.value)


# ---- 5. the sizing unit alone under AddressSanitizer + UBSan -----------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_capacity_under_asan_ubsan(tmp_path):
    """A stand-alone program (its own main) linked with the host-only unit, built with -fsanitize=address,undefined and run as a child
    process: a sweep of (rows, key bytes, width) against a 128-bit model, and the bad arguments."""
    exe = str(tmp_path / "distinct_plan_asan")
    csrc = os.path.join(ROOT, "immutable3_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "distinct_plan_asan.cpp"), os.path.join(csrc, "imm3_distinct_plan.cpp"), "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and " capacities ok, " in lines[0] and lines[1] == "6 bad arguments ok", r.stdout
