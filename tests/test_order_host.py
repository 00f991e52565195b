"""ORDER BY, the host side (no GPU): the SQL grammar with and without the flag (Python and C++ parsers), the query ADT and operator
defaults, the refusal of an order key outside the SELECT list, the host merge of per-segment ordered results against
tests/order_util.py, and the argument checks of imm3_query_set_order alone under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import order_util
from immutable3_amd import query as Q
from immutable3_amd.sql import ParseError, SQLParser

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")
DENSE_INT, DENSE_TINYINT, DENSE_STRING = 1, 2, 3


# ---- parser ----------------------------------------------------------------------------------------------------------
PARSED = [
    ("select id, age from t order by age", (("age", False),), 0),
    ("select id, age from t order by age asc", (("age", False),), 0),
    ("select id, age from t order by age desc", (("age", True),), 0),
    ("select id, age from t where (age > 18 and age < 30) order by age desc limit 10", (("age", True),), 10),
    ("select id, age, state from t order by state, age desc , id asc limit 3", (("state", False), ("age", True), ("id", False)), 3),
    ("select id from t where id > 5 limit 7", (), 7),
    ("select id from t", (), 0),
]


@pytest.mark.parametrize("sql,order_by,limit", PARSED)
def test_parser_with_the_flag(sql, order_by, limit):
    q = SQLParser.parseAll(sql, order_by=True)
    assert isinstance(q.project, Q.Project) and q.project.order_by == order_by and q.project.limit == limit
    if not order_by:                                       # a statement without the clause parses to the same ADT either way
        assert SQLParser.parseAll(sql) == q


def cpp_parse(sql, *flags):
    return subprocess.run([BIN, "--parse-only", *flags, "-q", sql], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("sql,order_by,limit", PARSED)
def test_cpp_parser_agrees(sql, order_by, limit):
    p = cpp_parse(sql, "--order-by")
    assert p.returncode == 0, p.stdout
    shown = ",List(" + ", ".join(f"({c},{'desc' if d else 'asc'})" for c, d in order_by) + ")" if order_by else ""
    assert p.stdout.strip().endswith(f",{limit}{shown}))"), p.stdout


ORDERED = [s for (s, o, _) in PARSED if o]


@pytest.mark.parametrize("sql", ORDERED)
def test_flag_off_fails_to_parse_as_before(sql):
    """Without the flag `order` is leftover input: the reference's parseAll failure at the clause's first column, from both parsers,
    byte for byte the same text."""
    at = sql.index("order") + 1
    with pytest.raises(ParseError) as e:
        SQLParser.parseAll(sql)
    assert str(e.value) == f"[1.{at}] failure: end of input expected\n\n{sql}"
    with pytest.raises(ParseError):
        SQLParser.parseAll(sql, order_by=False)
    p = cpp_parse(sql)
    assert p.returncode == 1 and p.stdout == str(e.value) + "\n"


def test_order_by_sits_between_where_and_limit():
    for sql in ("select id from t limit 3 order by id", "select id from t order by id where id > 3", "select id from t order by"):
        with pytest.raises(ParseError):
            SQLParser.parseAll(sql, order_by=True)
        assert cpp_parse(sql, "--order-by").returncode == 1
    # aggregation statements have no such clause, flag or not
    with pytest.raises(ParseError):
        SQLParser.parseAll("select max(age) from t group by state order by state", order_by=True)


# ---- ADT and operator defaults -----------------------------------------------------------------------------------------
def test_defaults_unchanged():
    from immutable3_amd.operators import ProjectOp
    p = Q.Project(["id", "age"], 10)
    assert p.cols == ("id", "age") and p.limit == 10 and p.order_by == ()
    assert Q.Project(["id"]) == Q.Project(["id"], 0, ()) and Q.Project(["id"]).limit == 0
    op = ProjectOp(["id", "age"], None)
    assert (op.cols, op.limit, op.order_by, op.order_keys) == (["id", "age"], 0, (), [])
    op = ProjectOp.mkProjectOp(["id", "age"], 5)(None)
    assert (op.limit, op.order_by) == (5, ())
    op = ProjectOp.mkProjectOp(["id", "age"], 5, [("age", True)])(None)
    assert op.order_keys == [(1, True)] and op.limit == 5
    assert Q.Project(["id", "age"], 0, [("age", True), ("id", False)]).order_by == (("age", True), ("id", False))


def test_unselected_order_key_is_a_value_error():
    from immutable3_amd.operators import ProjectOp
    with pytest.raises(ValueError, match="state"):
        Q.Project(["id", "age"], 0, [("age", False), ("state", True)])
    with pytest.raises(ValueError, match="state"):
        ProjectOp(["id", "age"], None, 0, [("state", False)])
    with pytest.raises(ValueError, match="state"):
        SQLParser.parseAll("select id, age from t order by state", order_by=True)


# ---- the host merge of per-segment ordered results ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_host_merge(seed):
    """Per-segment results, each ordered (and cut to the limit) by order_util, merged by operators.merge_ordered: equal to ordering
    all segments' rows at once by (keys, segment, row)."""
    from immutable3_amd.operators import merge_ordered
    rng = np.random.default_rng(600 + seed)
    codecs = [DENSE_INT, DENSE_TINYINT, DENSE_STRING]
    order_by = [[(1, True)], [(2, False), (1, True)], [(0, False)], [(1, False), (2, True), (0, True)], [(2, True)], [(1, True), (0, False)]][seed]
    limit = [0, 7, 1, 40, 1000, 0][seed]
    segs = []
    for s in range(4):
        n = int(rng.integers(0, 60))
        rows = np.sort(rng.permutation(200)[:n]).astype(np.int64)
        vals = [rng.integers(-3, 3, size=n).astype("<i4").view(np.uint8).reshape(n, 4),
                rng.integers(-2, 2, size=n).astype(np.int8).view(np.uint8).reshape(n, 1),
                rng.integers(0x7F, 0x81, size=(n, 2)).astype(np.uint8)]
        segs.append((s, rows, vals))
    wseg, wrow, wvals = order_util.merge_ordered(segs, codecs, order_by, limit)          # everything at once
    parts = []
    for (s, rows, vals) in segs:                                                            # what a per-segment ordered query returns
        perm = order_util.order_permutation(order_util.normalised_keys(vals, codecs, order_by), limit)
        parts.append((s, rows[perm], [vals[0][perm].view("<i4").reshape(-1), vals[1][perm].view(np.int8).reshape(-1), vals[2][perm]]))
    seg, row, cols = merge_ordered(parts, order_by, limit)
    assert seg.tolist() == wseg.tolist() and row.tolist() == wrow.tolist()
    assert cols[0].tolist() == wvals[0].view("<i4").reshape(-1).tolist() and cols[1].tolist() == wvals[1].view(np.int8).reshape(-1).tolist()
    assert cols[2].tobytes() == wvals[2].tobytes()


# ---- imm3_query_set_order's argument checks alone under AddressSanitizer + UBSan ------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_order_args_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "order_args_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "order_args_asan.cpp"), os.path.join(ROOT, "immutable3_amd", "csrc", "imm3_order_args.cpp"),
                           "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    assert len(r.stdout.splitlines()) == 21
