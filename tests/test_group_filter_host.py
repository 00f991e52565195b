"""HAVING over groups, the host side (no GPU): imm3_query_set_group_filter's argument checks and the kernels' evaluator through the
library (imm3_group_filter_check: plain values, no device), the Python filter_groups and the C++ filterGroups against a brute-force
evaluation in Fractions, the SQL grammar with and without the flag (both parsers), the ADT's and the operator's checks, and the plan
unit with the shared evaluator alone in a stand-alone program under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from immutable3_amd import native
from immutable3_amd import query as Q
from immutable3_amd.sql import ParseError, SQLParser

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")
LIBDIR = os.path.join(ROOT, "immutable3_amd", "lib")
HIPCC = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
GT, LT, EQ = native.GT, native.LT, native.EQ
AND, OR, NOT = native.EXPR_AND, native.EXPR_OR, native.EXPR_NOT
CNT = native.GROUP_FILTER_COUNT
I32, I8, STR = 0, 1, 2
# the aggregates of the checks below: count(id), min(v int32), max(a int8), sum(v), and -- for the refusals -- max(name string)
KINDS, COLS = [C, MN, MX, S], [I32, I32, I8, I32]


def compare(lhs, cond, rhs):
    return lhs > rhs if cond == GT else (lhs < rhs if cond == LT else lhs == rhs)


# ---- 1. the argument checks, through the library ------------------------------------------------------------------------------------------
REFUSED = [
    ("not an aggregation", dict(is_agg=False), [(CNT, 0, GT, 1)], [0], "not an aggregation query"),
    ("nine leaves", {}, [(CNT, 0, GT, 1)] * 9, [0], "n_leaves must be 0 .. 8"),
    ("33 program entries", {}, [(CNT, 0, GT, 1)], [0] + [0, AND] * 16, "n_prog must be 0 .. 32"),
    ("no program, but leaves", {}, [(CNT, 0, GT, 1)], [], "select program: empty, but leaves were given"),
    ("agg past the end", {}, [(4, 0, GT, 1)], [0], "names aggregate 4 of 4"),
    ("agg below IMM3_GROUP_FILTER_COUNT", {}, [(-2, 0, GT, 1)], [0], "names aggregate -2 of 4"),
    ("a string MAX", dict(kinds=[C, MX], cols=[I32, STR]), [(1, 0, GT, 1)], [0], "MAX over a STRING column"),
    ("average on a count", {}, [(0, 1, GT, 1)], [0], "average is for a SUM aggregate only"),
    ("average on a MIN", {}, [(1, 1, GT, 1)], [0], "average is for a SUM aggregate only"),
    ("average on IMM3_GROUP_FILTER_COUNT", {}, [(CNT, 1, GT, 1)], [0], "average is for a SUM aggregate only"),
    ("an average's value above the range", {}, [(3, 1, GT, 2 ** 31)], [0], "value must lie in [-2^31, 2^31 - 1]"),
    ("an average's value below the range", {}, [(3, 1, LT, -2 ** 31 - 1)], [0], "value must lie in [-2^31, 2^31 - 1]"),
    ("cond MATCH", {}, [(3, 0, native.MATCH, 1)], [0], "unknown cond 0"),
    ("cond 17", {}, [(3, 0, 17, 1)], [0], "unknown cond 17"),
    ("stack underflow", {}, [(3, 0, GT, 1)], [0, AND], "select program: stack underflow"),
    ("a NOT on nothing", {}, [(3, 0, GT, 1)], [NOT, 0], "select program: stack underflow"),
    ("two results", {}, [(3, 0, GT, 1)], [0, 0], "select program: more than one result"),
    ("operator -3", {}, [(3, 0, GT, 1)], [0, -3], "select program: unknown operator"),
    ("leaf index out of range", {}, [(3, 0, GT, 1)], [1], "select program: leaf index out of range"),
]


@pytest.mark.parametrize("what,shape,leaves,prog,frag", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_arguments(what, shape, leaves, prog, frag):
    with pytest.raises(native.Imm3Error) as e:
        native.group_filter_check(shape.get("kinds", KINDS), shape.get("cols", COLS), leaves, prog, is_agg=shape.get("is_agg", True))
    assert e.value.code == native.ERR_ARG and frag in e.value.msg, e.value.msg
    if not frag.startswith("select program"):
        assert e.value.msg.startswith("imm3_query_set_group_filter: ")


def test_null_query_and_accepted_shapes():
    L = native.load()
    ls, pg = native.group_filter_arrays([(CNT, 0, GT, 1)], [0])
    assert L.imm3_query_set_group_filter(None, ls.ctypes.data, 1, pg.ctypes.data, 1) == native.ERR_ARG
    assert b"query is null" in L.imm3_last_error()
    out = native.C.c_uint64(0)
    assert L.imm3_query_group_filter_stats(None, native.C.byref(out), native.C.byref(out)) == native.ERR_ARG
    assert native.GROUP_FILTER_LEAF.itemsize == 24 and native.GROUP_FILTER_LEAF.fields["value"][1] == 16     # the C struct's layout
    # removal: no leaves, no program -- every group is kept
    assert native.group_filter_check(KINDS, COLS, [], [], group=(3, [0, 0, 0, 0])) is True
    # the widest accepted call: 8 leaves, 32 entries
    leaves = [(j % 4 if j % 4 != 0 else CNT, 0, GT, -10 ** 18) for j in range(8)]
    prog = [0] + [x for j in range(1, 8) for x in (j, AND)] + [NOT] * 16 + [NOT]
    assert len(prog) == 32
    assert native.group_filter_check(KINDS, COLS, leaves, prog, group=(1, [1, 2, 3, 4])) is False
    # an average's value at both ends of its range, the product at the int64 edge
    assert native.group_filter_check(KINDS, COLS, [(3, 1, EQ, -2 ** 31)], [0], group=(2 ** 32 - 1, [0, 0, 0, -2 ** 31 * (2 ** 32 - 1)])) is True
    assert native.group_filter_check(KINDS, COLS, [(3, 1, GT, -2 ** 31)], [0], group=(2 ** 32 - 1, [0, 0, 0, -2 ** 31 * (2 ** 32 - 1)])) is False
    assert native.group_filter_check(KINDS, COLS, [(3, 1, LT, 2 ** 31 - 1)], [0], group=(2 ** 32 - 1, [0, 0, 0, (2 ** 31 - 1) * (2 ** 32 - 1) - 1])) is True
    # a COUNT aggregate and IMM3_GROUP_FILTER_COUNT both read the group's count, never vals
    for agg in (0, CNT):
        assert native.group_filter_check(KINDS, COLS, [(agg, 0, EQ, 5)], [0], group=(5, [99, 0, 0, 0])) is True
    # ... whatever its column: count(name) over a string column is compared like count(id) (found by the statement fuzz: the table path
    # refused `select count(state) from t group by state having state_count > 537`, which the per-segment path answers)
    assert native.group_filter_check([C, MX], [STR, STR], [(0, 0, GT, 4)], [0], group=(5, [0, 0, 0, 0])) is True
    assert native.group_filter_check([C, MX], [STR, STR], [(0, 0, LT, 5)], [0], group=(5, [0, 0, 0, 0])) is False


# ---- 2. random trees: the library's evaluator, the Python filter_groups and the C++ filterGroups against Fractions ---------------------------
def random_tree(rng, n_leaves, depth=0):
    """nested tuples: ("leaf", i) | ("not", t) | ("and" | "or", t, u)"""
    pick = 0 if depth >= 4 else int(rng.integers(0, 10))
    if pick < 3:
        return ("leaf", int(rng.integers(0, n_leaves)))
    if pick < 5:
        return ("not", random_tree(rng, n_leaves, depth + 1))
    return ("and" if pick < 8 else "or", random_tree(rng, n_leaves, depth + 1), random_tree(rng, n_leaves, depth + 1))


def postfix(tree):
    if tree[0] == "leaf":
        return [tree[1]]
    if tree[0] == "not":
        return postfix(tree[1]) + [NOT]
    return postfix(tree[1]) + postfix(tree[2]) + [AND if tree[0] == "and" else OR]


def truth(tree, answers):
    if tree[0] == "leaf":
        return answers[tree[1]]
    if tree[0] == "not":
        return not truth(tree[1], answers)
    a, b = truth(tree[1], answers), truth(tree[2], answers)
    return (a and b) if tree[0] == "and" else (a or b)


def leaf_truth(leaf, count, vals):
    """what the leaf MEANS: an average is the rational sum / count"""
    agg, average, cond, value = leaf
    if agg == CNT or KINDS[agg] == C:
        return compare(count, cond, value)
    if average:
        return compare(Fraction(vals[agg], count), cond, value)
    return compare(vals[agg], cond, value)


def test_the_library_evaluates_random_programs_like_the_tree():
    rng = np.random.default_rng(41)
    done = 0
    while done < 300:
        n_leaves = int(rng.integers(1, 9))
        leaves = []
        for _ in range(n_leaves):
            agg = int(rng.integers(-1, 4))
            leaves.append((agg, int(agg == 3 and rng.integers(0, 2)), [GT, LT, EQ][int(rng.integers(0, 3))], int(rng.integers(-20, 21))))
        tree = random_tree(rng, n_leaves)
        prog = postfix(tree)
        if len(prog) > 32:
            continue
        for _ in range(4):
            count, vals = int(rng.integers(1, 30)), [int(v) for v in rng.integers(-400, 401, size=4)]
            want = truth(tree, [leaf_truth(l, count, vals) for l in leaves])
            assert native.group_filter_check(KINDS, COLS, leaves, prog, group=(count, vals)) is want, (leaves, prog, count, vals)
        done += 1


AVERAGE_EDGES = [   # (sum, count, cond, value, answer)
    (-7, 2, GT, -4, True), (-7, 2, LT, -3, True), (-7, 2, EQ, -3, False), (-7, 2, EQ, -4, False), (-8, 2, EQ, -4, True),
    (7, 2, GT, 3, True), (7, 2, LT, 4, True), (7, 2, EQ, 3, False),
    (-2 ** 31 * (2 ** 32 - 1), 2 ** 32 - 1, EQ, -2 ** 31, True), (-2 ** 31 * (2 ** 32 - 1) + 1, 2 ** 32 - 1, GT, -2 ** 31, True),
    (-2 ** 31 * (2 ** 32 - 1) - 1, 2 ** 32 - 1, LT, -2 ** 31, True), ((2 ** 31 - 1) * (2 ** 32 - 1), 2 ** 32 - 1, EQ, 2 ** 31 - 1, True),
    (2 ** 63 - 1, 2 ** 32 - 1, GT, 2 ** 31 - 1, True), (-2 ** 63, 2 ** 32 - 1, LT, -2 ** 31, True),
]


def test_average_edges_in_the_library_and_in_python():
    from immutable3_amd.operators import AvgDoubleAggr, group_filter_leaf
    for (s, n, cond, value, want) in AVERAGE_EDGES:
        assert compare(Fraction(s, n), cond, value) is want
        assert native.group_filter_check(KINDS, COLS, [(3, 1, cond, value)], [0], group=(n, [0, 0, 0, s])) is want, (s, n, cond, value)
        a = AvgDoubleAggr("v", "v_avg")
        a.sum, a.counter = s, n
        assert group_filter_leaf({"v_avg": a}, ("v_avg", True, cond, value)) is want, (s, n, cond, value)


def adt_of(tree, named):
    if tree[0] == "leaf":
        alias, cond, value = named[tree[1]]
        return Q.Select(alias, {GT: Q.GT, LT: Q.LT, EQ: Q.EQ}[cond](float(value)))
    return (Q.And if tree[0] == "and" else Q.Or)(adt_of(tree[1], named), adt_of(tree[2], named))


def random_groups(rng, g):
    from immutable3_amd.operators import AvgDoubleAggr, CountAggr, MaxDoubleAggr, MinDoubleAggr
    result, plain = {}, []
    for i in range(g):
        c, x, n_, a = CountAggr("id", "id_count"), MaxDoubleAggr("v", "v_max"), MinDoubleAggr("w", "w_min"), AvgDoubleAggr("v", "v_avg")
        cnt, mx, mn, sm = int(rng.integers(1, 6)), int(rng.integers(-5, 6)), int(rng.integers(-5, 6)), int(rng.integers(-12, 13))
        c.set(cnt)
        x.value, n_.value = float(mx), float(mn)
        a.sum, a.counter = sm, cnt
        result[f"g{i}"] = {"id_count": c, "v_max": x, "w_min": n_, "v_avg": a}
        plain.append({"id_count": cnt, "v_max": mx, "w_min": mn, "v_avg": Fraction(sm, cnt)})
    return result, plain


@pytest.mark.parametrize("seed", range(8))
def test_filter_groups_against_brute_force(seed):
    """operators.filter_groups over random merged groups (few distinct values: every cond hits) against the tree evaluated in Fractions;
    the spec comes from a HAVING tree of the ADT, as the engine makes it.  (The ADT has no NOT: the C++ vectors below carry some.)"""
    from immutable3_amd.operators import AvgDoubleAggr, CountAggr, MaxDoubleAggr, MinDoubleAggr, filter_groups, group_filter_spec
    rng = np.random.default_rng(700 + seed)
    result, plain = random_groups(rng, int(rng.integers(0, 60)))
    aggs = [CountAggr("id", "id_count"), MaxDoubleAggr("v", "v_max"), MinDoubleAggr("w", "w_min"), AvgDoubleAggr("v", "v_avg")]
    aliases = [a.alias for a in aggs]
    named = [(aliases[int(rng.integers(0, 4))], [GT, LT, EQ][int(rng.integers(0, 3))], int(rng.integers(-4, 5))) for _ in range(int(rng.integers(1, 9)))]
    tree = random_tree(rng, len(named))
    while "not" in str(tree):
        tree = random_tree(rng, len(named))
    leaves, prog = group_filter_spec(aggs, ["state"], adt_of(tree, named))
    assert [l[1] for l in leaves] == [l[0] == "v_avg" for l in leaves]
    got = filter_groups(result, leaves, prog)
    want = [f"g{i}" for i, p in enumerate(plain) if truth(tree, [compare(p[a], c, v) for (a, c, v) in named])]
    assert list(got) == want and all(got[k] is result[k] for k in got)
    assert filter_groups(result, [], []) is result


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/native/group_filter_host.cpp: host/operators.hpp's filterGroups and groupFilterCompare on vectors from stdin"""
    exe = str(tmp_path_factory.mktemp("gf") / "group_filter_host")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-Wall", "-Wextra", "-x", "c++", os.path.join(HERE, "native", "group_filter_host.cpp"), "-o", exe,
                           "-L" + LIBDIR, "-limm3", "-Wl,-rpath," + LIBDIR])
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cpp_filter_groups_on_the_same_vectors(host_program):
    from immutable3_amd.operators import filter_groups
    rng = np.random.default_rng(99)
    for case in range(6):
        result, plain = random_groups(rng, int(rng.integers(0, 60)))
        aliases = ["id_count", "v_max", "w_min"]
        named = [(aliases[int(rng.integers(0, 3))], [GT, LT, EQ][int(rng.integers(0, 3))], int(rng.integers(-4, 5))) for _ in range(int(rng.integers(1, 9)))]
        tree = random_tree(rng, len(named))
        prog = postfix(tree)
        want = [str(i) for i, p in enumerate(plain) if truth(tree, [compare(p[a], c, v) for (a, c, v) in named])]
        text = f"L {len(named)}\n" + "".join(f"{a} {c} {v}\n" for (a, c, v) in named) + f"P {len(prog)}\n" + " ".join(str(op) for op in prog) + "\n"
        text += f"G {len(plain)}\n" + "".join(f"{p['id_count']} {p['v_max']} {p['w_min']}\n" for p in plain)
        text += f"C {len(AVERAGE_EDGES)}\n" + "".join(f"{s} {n} {cond} {value} 1\n" for (s, n, cond, value, _) in AVERAGE_EDGES)
        r = subprocess.run([host_program], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        kept, cmp = r.stdout.splitlines()
        assert kept.split()[1:] == want, (case, named, prog)
        assert cmp.split()[1:] == [str(int(w)) for (*_, w) in AVERAGE_EDGES]
        leaves = [(a, False, c, v) for (a, c, v) in named]           # ... and the Python function on the very same vectors, NOTs included
        assert [k[1:] for k in filter_groups(result, leaves, prog)] == want


# ---- 3. the ADT's and the operator's checks ------------------------------------------------------------------------------------------------
def test_project_agg_having_defaults_and_validation():
    from immutable3_amd.operators import AvgDoubleAggr, CountAggr, MaxDoubleAggr, MaxStringAggr, ProjectAggOp
    aggs = [Q.Count("id"), Q.Max("age", "oldest"), Q.Avg("age")]
    p = Q.ProjectAgg(aggs, ["state"])
    assert p.having is None and p == Q.ProjectAgg(aggs, ["state"], (), 0, None)
    h = Q.And(Q.Select("id_count", Q.GT(1000)), Q.Or(Q.Select("oldest", Q.LT(90.0)), Q.Select("age_avg", Q.EQ(-3))))
    p = Q.ProjectAgg(aggs, ["state"], [("id_count", True)], 10, having=h)
    assert p.having == h and p != Q.ProjectAgg(aggs, ["state"], [("id_count", True)], 10)
    assert Q.group_filter_leaves(p.aggs, p.groupBy, h) == ([("id_count", Q.GT, 1000), ("oldest", Q.LT, 90), ("age_avg", Q.EQ, -3)], [0, 1, 2, "or", "and"])
    for bad, frag in ((Q.Select("age_max", Q.GT(1)), "'age_max' is not an aggregate's alias"), (Q.Select("state", Q.EQ(1)), "'state': a group-by column"),
                      (Q.Select("id_count", Q.GT(1.5)), "the threshold 1.5 is not an integer"), (Q.Select("id_count", Q.GT(float("nan"))), "is not an integer"),
                      (Q.Select("id_count", Q.Match(["x"])), "must be GT, LT or EQ"), (Q.And(Q.Select("id_count", Q.GT(1)), Q.NoSelect), "neither And, Or nor Select")):
        with pytest.raises(ValueError, match=frag):
            Q.ProjectAgg(aggs, ["state"], having=bad)
    ops = [CountAggr("id", "id_count"), MaxDoubleAggr("age", "age_max"), AvgDoubleAggr("age", "age_avg"), MaxStringAggr("name", "name_max")]
    op = ProjectAggOp(ops, None, ["state"])
    assert (op.having, op.filter_leaves, op.filter_prog) == (None, [], [])
    op = ProjectAggOp(ops, None, ["state"], [("age_max", True)], 3, having=Q.Or(Q.Select("age_avg", Q.GT(30)), Q.Select("id_count", Q.EQ(2))))
    assert op.filter_leaves == [("age_avg", True, GT, 30), ("id_count", False, EQ, 2)] and op.filter_prog == [0, 1, OR]
    with pytest.raises(ValueError, match="'name_max': a string MAX"):
        ProjectAggOp(ops, None, ["state"], having=Q.Select("name_max", Q.GT(1)))
    with pytest.raises(ValueError, match="an average's threshold"):
        ProjectAggOp(ops, None, ["state"], having=Q.Select("age_avg", Q.GT(2 ** 31)))
    with pytest.raises(ValueError, match="'state': a group-by column"):
        ProjectAggOp(ops, None, ["state"], having=Q.Select("state", Q.GT(1)))


# ---- 4. both parsers -------------------------------------------------------------------------------------------------------------------------
def sel(name, cond, v):
    return Q.Select(name, cond(float(v)))


PARSED = [   # (statement, group by, order by, limit, having, where the parent commit's parsers stop without the flag: its "[1.N]")
    ("select count(id), max(age) from t group by state having id_count > 1000 order by id_count desc limit 10", ("state",), (("id_count", True),), 10,
     sel("id_count", Q.GT, 1000), 50),
    ("select count(id), max(age) from t group by state having count(id) > 5", ("state",), (), 0, sel("id_count", Q.GT, 5), 50),
    ("select count(id), max(age) from t group by state having (id_count > 5 and max(age) < 90)", ("state",), (), 0,
     Q.And(sel("id_count", Q.GT, 5), sel("age_max", Q.LT, 90)), 50),
    ("select count(id), min(age), max(age) from t group by state having ((id_count > 5 and age_max < 90) or (min(age) = 3 or id_count < 2)) order by state",
     ("state",), (("state", False),), 0,
     Q.Or(Q.And(sel("id_count", Q.GT, 5), sel("age_max", Q.LT, 90)), Q.Or(sel("age_min", Q.EQ, 3), sel("id_count", Q.LT, 2))), 60),
    ("select count(id) from t having id_count > 0", (), (), 0, sel("id_count", Q.GT, 0), 25),
    ("select count(id) from t where age > 3 group by state having id_count = 7 limit 5", ("state",), (), 5, sel("id_count", Q.EQ, 7), 54),
]
# the parse failures of the parent commit's build for these statements (Python parser and imm3_sql --parse-only, with and without
# --order-by), recorded there: "[1.N] failure: end of input expected", N the column of `having`
PARENT_FAILURE = "[1.{at}] failure: end of input expected\n\n{sql}"


def show(t):
    if isinstance(t, (Q.And, Q.Or)):
        return f"{type(t).__name__}({show(t.op1)},{show(t.op2)})"
    c = t.cond
    v = c.gt if isinstance(c, Q.GT) else (c.lt if isinstance(c, Q.LT) else c.eq)
    return f"Select({t.col},{type(c).__name__}({int(v)}))"


def cpp_parse(sql, *flags):
    return subprocess.run([BIN, "--parse-only", *flags, "-q", sql], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("sql,group,order_by,limit,having,at", PARSED)
def test_both_parsers_with_the_flag(sql, group, order_by, limit, having, at):
    q = SQLParser.parseAll(sql, group_order=True, having=True)
    assert isinstance(q.project, Q.ProjectAgg)
    assert (q.project.groupBy, q.project.order_by, q.project.limit, q.project.having) == (group, order_by, limit, having)
    p = cpp_parse(sql, "--order-by", "--having")
    assert p.returncode == 0, p.stdout
    tail = f"List({', '.join(group)}),List(" + ", ".join(f"({c},{'desc' if d else 'asc'})" for c, d in order_by) + f"),{limit},Some({show(having)})"
    assert p.stdout.strip().endswith(tail + "))"), p.stdout
    if not order_by and not limit:                         # the having flag alone is enough for a statement without the other clauses
        assert SQLParser.parseAll(sql, having=True) == q
        assert cpp_parse(sql, "--having").stdout == p.stdout


@pytest.mark.parametrize("sql,at", [(s, at) for (s, *_, at) in PARSED])
def test_flag_off_fails_to_parse_as_at_the_parent_commit(sql, at):
    assert sql.index(" having ") + 2 == at
    want = PARENT_FAILURE.format(at=at, sql=sql)
    for flags in ({}, {"having": False}, {"group_order": True}, {"order_by": True, "string_ranges": True}):
        with pytest.raises(ParseError) as e:
            SQLParser.parseAll(sql, **flags)
        assert str(e.value) == want
    for flags in ((), ("--order-by",), ("--order-by", "--string-ranges")):
        p = cpp_parse(sql, *flags)
        assert p.returncode == 1 and p.stdout == want + "\n"


def test_statements_without_the_clause_parse_the_same_either_way():
    for sql in ("select count(id), max(age) from t group by state order by id_count desc limit 10", "select count(id) from t group by state",
                "select id, age from t where age > 3 limit 2"):
        assert SQLParser.parseAll(sql, group_order=True, having=True) == SQLParser.parseAll(sql, group_order=True)
        assert cpp_parse(sql, "--order-by", "--having").stdout == cpp_parse(sql, "--order-by").stdout


def test_clause_order_and_refused_names():
    for sql in ("select count(id) from t group by state order by state having id_count > 1", "select count(id) from t having id_count > 1 group by state",
                "select count(id) from t group by state having", "select count(id) from t group by state having ()",
                "select count(id) from t group by state having id_count > 'x'", "select id from t having id > 1"):
        with pytest.raises(ParseError):
            SQLParser.parseAll(sql, group_order=True, having=True)
        assert cpp_parse(sql, "--order-by", "--having").returncode == 1
    for sql, name in (("select count(id) from t group by state having age_max > 1", "age_max"), ("select count(id) from t group by state having state = 3", "state"),
                      ("select count(id) from t group by state having (id_count > 1 and max(age) < 3)", "age_max")):
        with pytest.raises(ValueError, match=name):
            SQLParser.parseAll(sql, having=True)
        p = cpp_parse(sql, "--having")
        assert p.returncode == 1 and name in p.stdout
    # `having` with order by / limit behind it, but without their own flag: the clause parses, what follows is leftover input
    sql = "select count(id) from t group by state having id_count > 1 limit 3"
    with pytest.raises(ParseError, match="end of input expected"):
        SQLParser.parseAll(sql, having=True)
    assert cpp_parse(sql, "--having").returncode == 1


# ---- 5. the plan unit and the shared evaluator alone under AddressSanitizer + UBSan ------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_and_evaluator_under_asan_ubsan(tmp_path):
    """A stand-alone program (its own main) linked with the host-only translation units, built with -fsanitize=address,undefined and run
    as a child process: 10 000 random programs against the recursive evaluation of their trees, the average's overflow edge, refusals."""
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    exe = str(tmp_path / "group_filter_asan")
    csrc = os.path.join(ROOT, "immutable3_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-D__HIP_PLATFORM_AMD__", "-I", hip_inc,                      # (imm3_expr_norm.cpp reads the handles' header)
                           os.path.join(HERE, "native", "group_filter_asan.cpp"), os.path.join(csrc, "imm3_group_filter_plan.cpp"), os.path.join(csrc, "imm3_expr_norm.cpp"),
                           "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and lines[0].startswith("10000 programs ok") and lines[1] == "17 average edges ok" and lines[2] == "11 refusals ok, removal ok", r.stdout
