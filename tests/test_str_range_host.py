"""String ranges, the host side (no GPU): where a range goes (imm3_plan_string_range_route), the fold logic of csrc/imm3_str_range.cpp
alone under AddressSanitizer + UBSan, the SQL spellings with and without the flag (Python and C++ parsers), and the query ADT's
leaves -- the bytes the library gets -- from both languages."""
import json
import os
import shutil
import subprocess

import pytest

import str_range_util as U
from immutable3_amd import native
from immutable3_amd import query as Q
from immutable3_amd.sql import ParseError, SQLParser

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")


def test_route_over_every_width():
    for width in range(0, 258):
        want = -1 if width < 1 or width > 256 else (1 if width % 4 == 0 else 2)
        assert native.plan_string_range_route(width) == want, width
    # the widths the string pass takes for a range are the ones it takes for a Match
    assert all((native.plan_string_range_route(w) == 1) == (native.plan_string_route(w, 3) == 1) for w in range(1, 257))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fold_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "str_range_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "str_range_asan.cpp"), os.path.join(ROOT, "immutable3_amd", "csrc", "imm3_str_range.cpp"),
                           "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 37 and all(ln.endswith(" ok") for ln in lines), r.stdout


# ---- parsers -----------------------------------------------------------------------------------------------------------
PARSED = [
    ("select id from t where name like 'Jo%'", "Select(name,Prefix(Jo))", Q.Select("name", Q.Prefix("Jo"))),
    ("select id from t where name > 'M'", "Select(name,StrGT(M))", Q.Select("name", Q.StrGT("M"))),
    ("select id from t where name < 'M'", "Select(name,StrLT(M))", Q.Select("name", Q.StrLT("M"))),
    ("select id, name from t where (name like 'Jo%' and age > 18) order by name limit 5",
     "And(Select(name,Prefix(Jo)),Select(age,GT(18)))", Q.And(Q.Select("name", Q.Prefix("Jo")), Q.Select("age", Q.GT(18.0)))),
    ("select id, name from t where (name > 'M' and name < 'Zz' and state = 'CA') order by name desc, id limit 3",
     "And(And(Select(name,StrGT(M)),Select(name,StrLT(Zz))),Select(state,Match(List(CA))))",
     Q.And(Q.And(Q.Select("name", Q.StrGT("M")), Q.Select("name", Q.StrLT("Zz"))), Q.Select("state", Q.Match(["CA"])))),
]


def cpp_parse(sql, *flags):
    return subprocess.run([BIN, "--parse-only", *flags, "-q", sql], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("sql,shown,select", PARSED)
def test_both_parsers_with_the_flag(sql, shown, select):
    q = SQLParser.parseAll(sql, order_by=True, string_ranges=True)
    assert q.select == select
    p = cpp_parse(sql, "--string-ranges", "--order-by")
    assert p.returncode == 0 and f",{shown},Project(" in p.stdout, p.stdout
    if "order by" in sql:
        assert q.project.order_by and q.project.limit > 0 and ",List((name," in p.stdout


@pytest.mark.parametrize("sql", [s for (s, _, _) in PARSED])
def test_flag_off_fails_to_parse_as_before(sql):
    """Without the flag the grammar is the reference's: the same failure, byte for byte, from both parsers -- and (a statement that
    needs no order by) the same one under order_by alone"""
    with pytest.raises(ParseError) as e:
        SQLParser.parseAll(sql, order_by=True)
    p = cpp_parse(sql, "--order-by")
    assert p.returncode == 1 and p.stdout == str(e.value) + "\n"
    assert "failure:" in str(e.value) and str(e.value).endswith("\n\n" + sql)
    if "order by" not in sql:
        with pytest.raises(ParseError) as e2:
            SQLParser.parseAll(sql)
        assert str(e2.value) == str(e.value) and cpp_parse(sql).stdout == p.stdout
        with pytest.raises(ParseError):
            SQLParser.parseAll(sql, string_ranges=False)


def test_statements_without_the_spellings_parse_the_same_either_way():
    for sql in ("select id from t where (age > 18 and state = 'CA') limit 4", "select id from t where age < 7", "select max(age) from t where id > 3 group by state"):
        assert SQLParser.parseAll(sql, string_ranges=True) == SQLParser.parseAll(sql)
        assert cpp_parse(sql, "--string-ranges").stdout == cpp_parse(sql).stdout
    for sql in ("select id from t where name like 'Jo'", "select id from t where name like Jo%", "select id from t where name > 'M"):
        with pytest.raises(ParseError):
            SQLParser.parseAll(sql, string_ranges=True)
        assert cpp_parse(sql, "--string-ranges").returncode == 1


# ---- ADT to leaf --------------------------------------------------------------------------------------------------------
def test_adt_bounds():
    b = Q.str_range_bounds
    assert b(Q.StrRange("Jo", "M"), 8) == (b"Jo", b"M") and b(Q.Prefix("Jo"), 8) == (b"Jo", b"Jo")
    assert b(Q.StrGT("M"), 4) == (b"M\x00\x00\x01", b"") and b(Q.StrLT("M"), 4) == (b"", b"L\xff\xff\xff")
    assert b(Q.StrGT(b"m\x00\xff\xff\xff\xff"), 6) == (b"m\x01\x00\x00\x00\x00", b"") and b(Q.StrLT(b"m\x01\x00\x00\x00\x00"), 6) == (b"", b"m\x00\xff\xff\xff\xff")
    assert b(Q.StrGT(b"\xff" * 4), 4) == Q.STR_RANGE_NONE and b(Q.StrLT(b""), 4) == Q.STR_RANGE_NONE and b(Q.StrLT(b"\x00\x00"), 4) == Q.STR_RANGE_NONE
    assert b(Q.StrGT(b"\xff" * 3), 4) == (b"\xff\xff\xff\x01", b"")
    lo, hi = U.pad(*Q.STR_RANGE_NONE, 4)
    assert lo > hi
    for cond in (Q.StrRange("abcde", ""), Q.Prefix("abcde"), Q.StrGT("abcde"), Q.StrLT("abcde")):
        with pytest.raises(ValueError):
            b(cond, 4)
    # strictness, against the reference: StrGT(v) / StrLT(v) leave out v padded with 00 and take its neighbours
    for v in (b"M", b"m\x00\xff", b"\x00", b"\xff\xff\xff\xfe"):
        pv = v + b"\x00" * (4 - len(v))
        rows = U.rows_array([r for r in (pv, U.predecessor(pv), U.successor(pv)) if r is not None], 4)
        assert U.in_range(rows, *b(Q.StrGT(v), 4)).tolist() == [bytes(r) > pv for r in rows]
        assert U.in_range(rows, *b(Q.StrLT(v), 4)).tolist() == [bytes(r) < pv for r in rows]


def test_operators_emit_the_leaf():
    from immutable3_amd.operators import SelectOp, _cond_spec, select_program
    assert _cond_spec(Q.Prefix("Jo"), 8) == (native.STR_RANGE, [b"Jo", b"Jo"])
    assert _cond_spec(Q.StrGT("M"), 2) == (native.STR_RANGE, [b"M\x01", b""])
    assert _cond_spec(Q.Match(["CA"]), 2) == (native.MATCH, [b"CA"]) and _cond_spec(Q.GT(3.0)) == (native.GT, 3.0)
    op = SelectOp.mkSelectOp("name", Q.Prefix("Jo"))(None)
    assert (op.col, op.cond) == ("name", Q.Prefix("Jo"))
    leaves, prog = select_program(Q.And(Q.Select("name", Q.StrGT("M")), Q.Select("age", Q.GT(1.0))))
    assert leaves == [("name", Q.StrGT("M")), ("age", Q.GT(1.0))] and prog == [0, 1, native.EXPR_AND]


@pytest.mark.parametrize("width", [2, 4, 6, 16])
def test_adt_to_leaf_is_the_same_bytes_in_both_languages(tmp_path, width):
    """the leaves of the three spellings on a string column of `width` bytes: query.str_range_bounds against what imm3_sql hands the
    library (--parse-only --string-ranges with a table's schema prints them), carries and the ends included"""
    from immutable3_amd.schema import Column, Table, TableIO
    TableIO.store(str(tmp_path), Table("t", [Column.make("id", "DENSE_INT"), Column.make("name", "DENSE_STRING", {"size": str(width)})], 1024))
    values = ["M", "Jo", "z" * width, "0" * width, "a" + "z" * (width - 1)]
    for v in values:
        for spelling, cond in ((f"name like '{v}%'", Q.Prefix(v)), (f"name > '{v}'", Q.StrGT(v)), (f"name < '{v}'", Q.StrLT(v))):
            sql = f"select id from t where {spelling}"
            assert SQLParser.parseAll(sql, string_ranges=True).select == Q.Select("name", cond)
            lo, hi = Q.str_range_bounds(cond, width)
            p = subprocess.run([BIN, "--parse-only", "--string-ranges", "-d", str(tmp_path), "-q", sql], capture_output=True, text=True, timeout=60)
            assert p.returncode == 0 and p.stdout.splitlines()[-1] == f"leafbytes: name:{lo.hex()}:{hi.hex()}", p.stdout
    p = subprocess.run([BIN, "--parse-only", "--string-ranges", "-d", str(tmp_path), "-q", f"select id from t where name > '{'x' * (width + 1)}'"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "longer than the column" in p.stdout
