"""ORDER BY over groups, the host side (no GPU): the SQL grammar with and without the flag (Python and C++ parsers), the ProjectAgg ADT's
checks, the shared host ordering of merged groups against np.lexsort, and the argument checks and key layout of
imm3_query_set_group_order alone under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from immutable3_amd import query as Q
from immutable3_amd.schema import CodecType, Column
from immutable3_amd.sql import ParseError, SQLParser

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")

# ---- parser ----------------------------------------------------------------------------------------------------------
PARSED = [
    ("select count(id), max(age) from t group by state order by id_count desc limit 10", ("state",), (("id_count", True),), 10),
    ("select count(id), max(age) from t group by state order by count(id) desc, max(age), state asc limit 3", ("state",),
     (("id_count", True), ("age_max", False), ("state", False)), 3),
    ("select count(id), min(age) from t where (age > 18 and age < 30) group by state, age order by age desc , min(age)", ("state", "age"),
     (("age", True), ("age_min", False)), 0),
    ("select max(age) from t order by age_max", (), (("age_max", False),), 0),
    ("select count(id) from t group by state limit 5", ("state",), (), 5),
    ("select count(id) from t where age > 3 limit 2", (), (), 2),
    ("select count(id) from t group by state", ("state",), (), 0),
]


def cpp_parse(sql, *flags):
    return subprocess.run([BIN, "--parse-only", *flags, "-q", sql], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("sql,group,order_by,limit", PARSED)
def test_both_parsers_with_the_flag(sql, group, order_by, limit):
    q = SQLParser.parseAll(sql, group_order=True)
    assert isinstance(q.project, Q.ProjectAgg)
    assert (q.project.groupBy, q.project.order_by, q.project.limit) == (group, order_by, limit)
    p = cpp_parse(sql, "--order-by")
    assert p.returncode == 0, p.stdout
    tail = f"List({', '.join(group)})"
    if order_by or limit:
        tail += ",List(" + ", ".join(f"({c},{'desc' if d else 'asc'})" for c, d in order_by) + f"),{limit}"
    assert p.stdout.strip().endswith(tail + "))"), p.stdout
    if not order_by and not limit:                       # a statement without the clauses parses to the same ADT either way
        assert SQLParser.parseAll(sql) == q
        assert cpp_parse(sql).stdout == p.stdout


@pytest.mark.parametrize("sql", [s for (s, _, o, l) in PARSED if o or l])
def test_flag_off_fails_to_parse_as_before(sql):
    """Without the flag `order` / `limit` behind an aggregation is leftover input: the reference's parseAll failure at the clause's first
    column, from both parsers, byte for byte the same text."""
    at = (sql.index(" order ") if " order " in sql else sql.index(" limit ")) + 2
    with pytest.raises(ParseError) as e:
        SQLParser.parseAll(sql)
    assert str(e.value) == f"[1.{at}] failure: end of input expected\n\n{sql}"
    for flags in ({"group_order": False}, {"order_by": True}):          # (order_by alone is the projection's clause: aggregations stay the reference's)
        with pytest.raises(ParseError) as e2:
            SQLParser.parseAll(sql, **flags)
        assert str(e2.value) == str(e.value)
    p = cpp_parse(sql)
    assert p.returncode == 1 and p.stdout == str(e.value) + "\n"


def test_clause_order_and_unknown_names():
    for sql in ("select count(id) from t group by state limit 3 order by state", "select count(id) from t order by id_count group by state",
                "select count(id) from t group by state order by"):
        with pytest.raises(ParseError):
            SQLParser.parseAll(sql, group_order=True)
        assert cpp_parse(sql, "--order-by").returncode == 1
    for sql, name in (("select count(id) from t group by state order by age", "age"), ("select count(id) from t order by max(age)", "age_max")):
        with pytest.raises(ValueError, match=name):
            SQLParser.parseAll(sql, group_order=True)
        p = cpp_parse(sql, "--order-by")
        assert p.returncode == 1 and name in p.stdout


# ---- ADT and operator checks -------------------------------------------------------------------------------------------
def test_project_agg_defaults_and_validation():
    from immutable3_amd.operators import AvgDoubleAggr, CountAggr, MaxDoubleAggr, ProjectAggOp
    p = Q.ProjectAgg([Q.Count("id"), Q.Max("age")], ["state"])
    assert (p.order_by, p.limit) == ((), 0) and p == Q.ProjectAgg([Q.Count("id"), Q.Max("age")], ["state"], (), 0)
    p = Q.ProjectAgg([Q.Count("id"), Q.Max("age", "oldest")], ["state"], [("oldest", True), ("state", False), ("id_count", 1)], 10)
    assert p.order_by == (("oldest", True), ("state", False), ("id_count", True)) and p.limit == 10
    with pytest.raises(ValueError, match="'age_max' is neither a group-by column .* nor an aggregate's alias"):
        Q.ProjectAgg([Q.Count("id"), Q.Max("age", "oldest")], ["state"], [("age_max", False)])
    with pytest.raises(ValueError, match="'id'"):
        Q.ProjectAgg([Q.Count("id")], ["state"], [("id", False)])
    with pytest.raises(ValueError, match="'age_avg': ordering by an average"):
        Q.ProjectAgg([Q.Avg("age")], ["state"], [("age_avg", False)])
    aggs = [CountAggr("id", "id_count"), MaxDoubleAggr("age", "age_max"), AvgDoubleAggr("age", "age_avg")]
    op = ProjectAggOp(aggs, None, ["state"])
    assert (op.order_by, op.limit, op.order_spec) == ((), 0, [])
    op = ProjectAggOp(aggs, None, ["state"], [("age_max", True), ("state", False)], 3)
    assert op.order_spec == [(True, "age_max", True), (False, "state", False)] and op.limit == 3
    with pytest.raises(ValueError, match="'age_avg': ordering by an average"):
        ProjectAggOp(aggs, None, ["state"], [("age_avg", False)])
    with pytest.raises(ValueError, match="'name' is neither"):
        ProjectAggOp(aggs, None, ["state"], [("name", False)])


# ---- the shared host ordering of merged groups -----------------------------------------------------------------------------
def _col(name, ctype, codec, size=None):
    return Column(name, ctype, codec, {"size": str(size)} if size else {})


@pytest.mark.parametrize("seed", range(8))
def test_order_groups_against_lexsort(seed):
    """Random merged groups over (k int32, a int8, s string(3)) with count / max / min / string-max aggregators, few distinct values
    (ties): operators.order_groups against np.lexsort over the normal form with the arrival index last."""
    from immutable3_amd.operators import CountAggr, MaxDoubleAggr, MaxStringAggr, MinDoubleAggr, order_groups
    rng = np.random.default_rng(900 + seed)
    g = int(rng.integers(0, 70))
    gcols = [_col("k", "INT", CodecType.DENSE_INT), _col("a", "TINYINT", CodecType.DENSE_TINYINT), _col("s", "STRING", CodecType.DENSE_STRING, 3)]
    k = rng.integers(-3, 3, size=g).astype("<i4")
    a = rng.integers(-2, 2, size=g).astype(np.int8)
    s = rng.integers(0x61, 0x63, size=(g, 3)).astype(np.uint8)
    cnt = rng.integers(1, 4, size=g)
    mx = rng.integers(-2 ** 31, 2 ** 31, size=g) if seed % 2 else rng.integers(-2, 2, size=g)
    mn = rng.integers(-128, 128, size=g)
    sm = rng.integers(0x41, 0x43, size=(g, 2)).astype(np.uint8)
    result, raw = {}, {}
    for i in range(g):
        key = f"g{i}"                                     # (unique: the merged dict has one entry per group)
        c, x, n_, t = CountAggr("id", "id_count"), MaxDoubleAggr("v", "v_max"), MinDoubleAggr("w", "w_min"), MaxStringAggr("n", "n_max")
        c.set(int(cnt[i]))
        x.value, n_.value, t.value = float(mx[i]), float(mn[i]), bytes(sm[i]).decode()
        result[key] = {"id_count": c, "v_max": x, "w_min": n_, "n_max": t}
        raw[key] = [k[i].tobytes(), a[i].tobytes(), bytes(s[i])]
    specs = [[(True, "id_count", True)], [(False, "k", True), (True, "w_min", False)], [(False, "s", False), (False, "a", True)],
             [(True, "n_max", True), (True, "v_max", False)], [(False, "a", False)], [(True, "v_max", True), (False, "k", False), (True, "id_count", False)],
             [(True, "w_min", True)], [(False, "s", True), (True, "n_max", False), (False, "k", True), (True, "id_count", True)]]
    spec, limit = specs[seed], [0, 5, 1, 0, 1000, 7, 0, 3][seed]
    source = {"k": k.astype(np.int64), "a": a.astype(np.int64), "id_count": cnt.astype(np.int64), "v_max": mx.astype(np.int64), "w_min": mn.astype(np.int64)}
    lex = [np.arange(g)]                                  # least significant first: the arrival index, then the keys from the last one up
    for (_, name, desc) in reversed(spec):
        if name in source:
            lex.append(-source[name] if desc else source[name])
        else:
            b = s if name == "s" else sm
            for j in range(b.shape[1] - 1, -1, -1):
                lex.append(255 - b[:, j].astype(np.int64) if desc else b[:, j].astype(np.int64))
    want = np.lexsort(tuple(lex)) if g else np.zeros(0, np.int64)
    if limit > 0:
        want = want[:limit]
    got = order_groups(result, raw, gcols, spec, limit)
    assert list(got) == [f"g{i}" for i in want]
    assert all(got[key] is result[key] for key in got)


def test_order_groups_without_keys_keeps_arrival_order():
    from immutable3_amd.operators import CountAggr, order_groups
    result = {f"k{i}": {"c": CountAggr("id", "c")} for i in range(5)}
    assert list(order_groups(result, {}, [], [], 0)) == list(result)
    assert list(order_groups(result, {}, [], [], 2)) == ["k0", "k1"]


# ---- imm3_query_set_group_order's checks and key layout alone under AddressSanitizer + UBSan ----------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_under_asan_ubsan(tmp_path):
    """A stand-alone program (its own main) linked with the host-only translation unit, built with -fsanitize=address,undefined and run
    as a child process: every kind / width combination, the layout, and the error cases."""
    exe = str(tmp_path / "group_order_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "group_order_asan.cpp"), os.path.join(ROOT, "immutable3_amd", "csrc", "imm3_group_order_plan.cpp"),
                           "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 62 and all(ln.endswith(" ok") for ln in lines), r.stdout
