"""CPU suite for IMM3_INT_IN: the probe table's properties (imm3_plan_int_list_table against a Python set), the folding of lists and
intervals (imm3_expr_normalize), the Python front end's condition, the fuzz generator's refusal rate, and the host unit alone under
the address and undefined-behaviour sanitizers (tests/native/int_list_asan.cpp).  No device is touched."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from immutable3_amd import native
from immutable3_amd import query as Q
import int_in_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DI, DT, DS = native.DENSE_INT, native.DENSE_TINYINT, native.DENSE_STRING
IN, GT, LT, EQ, MATCH = native.INT_IN, native.GT, native.LT, native.EQ, native.MATCH
AND, OR, NOT = native.EXPR_AND, native.EXPR_OR, native.EXPR_NOT
I32_MIN, I32_MAX = U.INT32_MIN, U.INT32_MAX


# ---- 1. the table ------------------------------------------------------------------------------------------------------
def hard_lists():
    rng = np.random.default_rng(7)
    l = U.lds_largest_n()
    out = {f"{n} random": rng.integers(I32_MIN, I32_MAX + 1, size=n).tolist() for n in (1, 2, 8, 9, 16, 17, l, l + 1, 100_000)}
    out["the ends, -1 and 0"] = [I32_MIN, I32_MAX, -1, 0]
    out["the ends among others"] = [I32_MIN, I32_MAX, -1, 0] + rng.integers(-1000, 1000, size=50).tolist()
    out["duplicates"] = [5, 5, 5, -7, -7, 123456, 5]
    out["one home slot"] = U.same_home_values(24)
    out["consecutive"] = list(range(-3000, 3000))
    out["from INT32_MIN up"] = list(range(I32_MIN, I32_MIN + 40))
    return out


@pytest.mark.parametrize("what,values", list(hard_lists().items()), ids=list(hard_lists().keys()))
def test_table_properties(what, values):
    members = set(int(v) for v in values)
    slots, empty, max_probe = native.plan_int_list_table(values)
    n_slots = slots.size
    assert n_slots >= max(16, 2 * len(members)) and n_slots & (n_slots - 1) == 0 and n_slots < 4 * max(8, len(members))
    assert empty not in members and max_probe >= 1
    held = slots[slots != empty].tolist()
    assert sorted(held) == sorted(members)                                      # every value once, nothing else
    rng = np.random.default_rng(len(values))
    sample = list(members) if len(members) <= 5000 else rng.choice(np.array(sorted(members)), size=5000, replace=False).tolist()
    for v in sample:                                                            # found within max_probe steps: the library's probe and its restatement
        assert native.plan_int_list_probe(slots, empty, max_probe, int(v)) == 1, (what, v)
        assert U.probe_py(slots, empty, max_probe, int(v)), (what, v)
    if what == "one home slot":
        assert max_probe == len(members) and len({U.home(v, n_slots) for v in members}) == 1
    # 10 000 non-members, `empty` and the members' neighbours among them
    near = [v + d for v in sample[:2000] for d in (-1, 1) if I32_MIN <= v + d <= I32_MAX]
    non = [empty] + [int(v) for v in near if int(v) not in members]
    non += [int(v) for v in rng.integers(I32_MIN, I32_MAX + 1, size=12_000).tolist() if int(v) not in members][:10_000 - len(non)]
    assert len(non) == 10_000
    s32 = np.ascontiguousarray(slots, dtype=np.int32)
    for v in non[:3000]:
        assert native.plan_int_list_probe(s32, empty, max_probe, v) == 0, (what, v)
    for v in non[3000:]:
        assert not U.probe_py(s32, empty, max_probe, v), (what, v)
    again = native.plan_int_list_table(values)
    assert again[0].tolist() == slots.tolist() and again[1:] == (empty, max_probe)   # deterministic
    shuffled = native.plan_int_list_table(rng.permutation(np.array(values, dtype=np.int64)).tolist())
    assert shuffled[0].tolist() == slots.tolist()                                # ... and independent of the order the values came in


def test_forms_and_their_thresholds():
    a, l = U.args_largest_n(), U.lds_largest_n()
    assert 1 <= a < l < native.INT_IN_MAX_VALUES
    assert [native.plan_int_list_form(4, n) for n in (0, 1, a, a + 1, l, l + 1, native.INT_IN_MAX_VALUES)] == \
        [native.INT_LIST_ARGS] * 3 + [native.INT_LIST_LDS] * 2 + [native.INT_LIST_GLOBAL] * 2
    assert all(native.plan_int_list_form(1, n) == native.INT_LIST_I8 for n in (0, 1, 64, 256, 100_000))
    assert [native.plan_int_list_form(w, n) for w, n in ((2, 1), (0, 1), (4, -1), (4, native.INT_IN_MAX_VALUES + 1))] == [-1] * 4
    # the LDS form's table and the kernel's own 16 bytes fit the 64 KiB of static LDS a work-group may hold
    assert U.slots_for(l) * 4 + 16 <= 64 * 1024


# ---- 2. folding --------------------------------------------------------------------------------------------------------
def norm(leaves, prog, codecs=(DI, DT, DS), widths=(4, 1, 4)):
    return native.expr_normalize(list(codecs), list(widths), leaves, prog)


def test_folding():
    # a list alone: sorted, each value once, the interval its minimum and maximum
    assert norm([(0, IN, [9, 1, 5, 5, 100])], [0]) == [[{"col": 0, "lo": 1, "hi": 100, "list": [1, 5, 9, 100]}]]
    # list and range, either order, GT / LT strict
    want = [[{"col": 0, "lo": 5, "hi": 9, "list": [5, 9]}]]
    assert norm([(0, IN, [9, 1, 5, 100]), (0, GT, 1.0), (0, LT, 100.0)], [0, 1, AND, 2, AND]) == want
    assert norm([(0, GT, 1.0), (0, IN, [9, 1, 5, 100]), (0, LT, 100.0)], [0, 1, AND, 2, AND]) == want
    # list and list: the intersection
    assert norm([(0, IN, [1, 2, 3, 4, 5]), (0, IN, [9, 5, 3, -1])], [0, 1, AND]) == [[{"col": 0, "lo": 3, "hi": 5, "list": [3, 5]}]]
    # list and EQ
    assert norm([(0, IN, [1, 2, 3]), (0, EQ, 2.0)], [0, 1, AND]) == [[{"col": 0, "lo": 2, "hi": 2, "list": [2]}]]
    # empty results: always false (no term)
    for leaves, prog in (([(0, IN, [])], [0]), ([(0, IN, [1, 2]), (0, IN, [3])], [0, 1, AND]), ([(0, IN, [1, 2]), (0, GT, 5.0)], [0, 1, AND]),
                         ([(0, IN, [1, 2, 3]), (0, EQ, 7.0)], [0, 1, AND]), ([(1, IN, [300, -129, 1 << 20])], [0])):
        assert norm(leaves, prog) == [], leaves
    # int8: values outside -128 .. 127 are no members (no d.toByte wrap: 300 is not 44)
    assert norm([(1, IN, [300, -128, 127, -129, 44 + 256])], [0]) == [[{"col": 1, "lo": -128, "hi": 127, "list": [-128, 127]}]]
    # the ends of int32
    assert norm([(0, IN, [I32_MIN, I32_MAX])], [0]) == [[{"col": 0, "lo": I32_MIN, "hi": I32_MAX, "list": [I32_MIN, I32_MAX]}]]
    # lists on two columns beside a range and a Match: one term, one predicate per column, in program order
    got = norm([(0, IN, [3, 1]), (1, IN, [7]), (2, MATCH, [b"abcd"]), (1, GT, 0.0)], [0, 1, AND, 2, AND, 3, AND])
    assert got == [[{"col": 0, "lo": 1, "hi": 3, "list": [1, 3]}, {"col": 1, "lo": 7, "hi": 7, "list": [7]}, {"col": 2, "match": [b"abcd"]}]]
    # an AND-only program is the flat list, whatever its shape
    flat = norm([(0, IN, [1, 2, 3]), (0, GT, 1.0), (1, LT, 5.0)], [0, 1, AND, 2, AND])
    assert norm([(0, IN, [1, 2, 3]), (0, GT, 1.0), (1, LT, 5.0)], [0, 1, 2, AND, AND]) == flat
    assert flat == [[{"col": 0, "lo": 2, "hi": 3, "list": [2, 3]}, {"col": 1, "lo": -128, "hi": 4}]]


def test_refusals_and_unchanged_errors():
    for prog in ([0, 1, OR], [0, NOT], [0, 1, AND, NOT], [1, NOT, 0, AND]):
        with pytest.raises(native.Imm3Error) as e:
            norm([(0, IN, [1, 2]), (1, GT, 1.0)], prog)
        assert e.value.code == native.ERR_ARG and not e.value.msg.startswith(native.TABLE_TREE_REFUSED)
        assert e.value.msg == ("a select program with an IMM3_EXPR_OR or an IMM3_EXPR_NOT does not take IMM3_INT_IN leaves (its normal form would "
                               "need negated lists and intervals with exclusions); a program of IMM3_EXPR_AND alone does")
    for col in (0, 1):                                                          # Match on an int column keeps its error
        with pytest.raises(native.Imm3Error) as e:
            norm([(col, MATCH, [b"abcd"])], [0])
        assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    with pytest.raises(native.Imm3Error) as e:                                  # the list on a string column
        norm([(2, IN, [1])], [0])
    assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    for operand, word in ((native.RawIntList(-1, [1]), "negative"), (native.RawIntList(2, None), "null"),
                          (native.RawIntList(native.INT_IN_MAX_VALUES + 1, [1]), "IMM3_INT_IN_MAX_VALUES")):
        with pytest.raises(native.Imm3Error) as e:
            norm([(0, IN, operand)], [0])
        assert e.value.code == native.ERR_ARG and word in e.value.msg
    for cond in (native.NOTMATCH, native.NOOP, 8, 9):                            # 7 is a condition now; its neighbours are not
        with pytest.raises(native.Imm3Error) as e:
            norm([(0, cond, None)], [0])
        assert e.value.code == native.ERR_UNSUPPORTED_CONDITION
    assert native.load().imm3_abi_version() == 1


# ---- 3. the Python front end's condition ---------------------------------------------------------------------------------
def test_query_condition():
    from immutable3_amd import operators
    c = Q.IntIn([3, 1, 3, -5])
    assert c.values == (3, 1, 3, -5) and c == Q.IntIn((3, 1, 3, -5)) and isinstance(c, operators.SUPPORTED_CONDS)
    assert operators._cond_spec(c, 4) == (native.INT_IN, [3, 1, 3, -5])
    assert Q.IntIn([]).values == ()
    assert Q.IntIn([I32_MIN, I32_MAX]).values == (I32_MIN, I32_MAX)
    for bad in (I32_MAX + 1, I32_MIN - 1):
        with pytest.raises(ValueError) as e:
            Q.IntIn([1, bad])
        assert str(e.value) == Q.INT_IN_RANGE_ERROR + str(bad)
    for bad in (1.5, True, "x"):
        with pytest.raises((ValueError, TypeError)):
            Q.IntIn([bad])
    with pytest.raises(ValueError):
        native._cselects([(0, native.INT_IN, [1 << 31])])
    # an AND tree keeps the leaf; select_program spells it as the flat list's leaves
    tree = Q.And(Q.Select("id", Q.IntIn([1, 2])), Q.Select("age", Q.GT(3)))
    leaves, prog = operators.select_program(tree, False)
    assert leaves == [("id", Q.IntIn([1, 2])), ("age", Q.GT(3))] and prog == [0, 1, native.EXPR_AND]


# ---- 3b. both parsers: the same statements accepted and refused, the same messages, equal ADTs ----------------------------------------
BIN = os.path.join(ROOT, "immutable3_amd", "bin", "imm3_sql")
PARSED = [
    ("select id from t where id in (3, -17,4096)", "Select(id,IntIn(List(3, -17, 4096)))", Q.Select("id", Q.IntIn([3, -17, 4096]))),
    ("select id from t where id in(7)", "Select(id,IntIn(List(7)))", Q.Select("id", Q.IntIn([7]))),
    ("select id from t where age in (-128, 0002147483647 , -2147483648)", "Select(age,IntIn(List(-128, 2147483647, -2147483648)))",
     Q.Select("age", Q.IntIn([-128, 2147483647, -2147483648]))),
    ("select id, age from t where (id in (1,2,3) and age > 18 and age in (20, 30)) limit 5",
     "And(And(Select(id,IntIn(List(1, 2, 3))),Select(age,GT(18))),Select(age,IntIn(List(20, 30))))",
     Q.And(Q.And(Q.Select("id", Q.IntIn([1, 2, 3])), Q.Select("age", Q.GT(18.0))), Q.Select("age", Q.IntIn([20, 30])))),
    ("select max(age) from t where (id in (5) or state = 'CA') group by state", "Or(Select(id,IntIn(List(5))),Select(state,Match(List(CA))))",
     Q.Or(Q.Select("id", Q.IntIn([5])), Q.Select("state", Q.Match(["CA"])))),
]
REFUSED = ["select id from t where id in ()", "select id from t where id in (1,)", "select id from t where id in (1, 2", "select id from t where id in (a)",
           "select id from t where id in 1, 2", "select id from t where (id in (1 2) and age > 3)", "select id from t where id in (+1)",
           "select id from t where id in (1.5)", "select id from t where id in (- 1)"]
OUT_OF_RANGE = [("select id from t where id in (2147483648)", "2147483648"), ("select id from t where id in (1, -2147483649)", "-2147483649"),
                ("select id from t where (age > 1 and id in (99999999999999999999))", "99999999999999999999")]


def cpp_parse(sql, *flags):
    return subprocess.run([BIN, "--parse-only", *flags, "-q", sql], capture_output=True, text=True, timeout=60)


def py_failure(sql, **flags):
    from immutable3_amd.sql import ParseError, SQLParser
    with pytest.raises(ParseError) as e:
        SQLParser.parseAll(sql, **flags)
    return str(e.value)


@pytest.mark.parametrize("sql,shown,select", PARSED)
def test_both_parsers_with_the_flag(sql, shown, select):
    from immutable3_amd.sql import SQLParser
    assert SQLParser.parseAll(sql, int_lists=True).select == select
    p = cpp_parse(sql, "--int-lists")
    assert p.returncode == 0 and f",{shown},Project" in p.stdout, p.stdout
    # with the flag off: the same failure, byte for byte, from both parsers -- the one the statement has always given
    off = cpp_parse(sql)
    assert off.returncode == 1 and off.stdout == py_failure(sql) + "\n" and "failure:" in off.stdout


@pytest.mark.parametrize("sql", REFUSED)
def test_both_parsers_refuse_the_same(sql):
    msg = py_failure(sql, int_lists=True)
    p = cpp_parse(sql, "--int-lists")
    assert p.returncode == 1 and p.stdout == msg + "\n" and msg.endswith("\n\n" + sql)
    assert cpp_parse(sql).stdout == py_failure(sql) + "\n"


@pytest.mark.parametrize("sql,literal", OUT_OF_RANGE)
def test_a_literal_outside_int32_is_an_error_with_a_fixed_text(sql, literal):
    from immutable3_amd.sql import SQLParser
    with pytest.raises(ValueError) as e:
        SQLParser.parseAll(sql, int_lists=True)
    assert str(e.value) == "integer literal out of range for an IN-list (int32): " + literal
    p = cpp_parse(sql, "--int-lists")
    assert p.returncode == 1 and p.stdout == str(e.value) + "\n"


def test_statements_without_a_list_parse_the_same_either_way():
    from immutable3_amd.sql import SQLParser
    for sql in ("select id from t where (age > 18 and state = 'CA') limit 4", "select id from t where age < 7", "select max(age) from t where id > 3 group by state",
                "select id from t where inn = 3", "select id from t where in > 3"):
        assert SQLParser.parseAll(sql, int_lists=True) == SQLParser.parseAll(sql)
        assert cpp_parse(sql, "--int-lists").stdout == cpp_parse(sql).stdout and cpp_parse(sql).returncode == 0
    for sql in ("select id from t where age >", "select id from t where (age > 1 and", "select id from"):   # failures unrelated to lists, flag off and on
        assert cpp_parse(sql).stdout == py_failure(sql) + "\n" and cpp_parse(sql, "--int-lists").stdout == py_failure(sql, int_lists=True) + "\n"


# ---- the fuzz's generator: at most one statement in ten may be left out ------------------------------------------------------
def test_fuzz_generator_leaves_out_at_most_a_tenth():
    rng = np.random.default_rng(20260)                                          # test_gpu_int_in.py's seed
    out, lists, present, empties = 0, 0, 0, 0
    for _ in range(200):
        st = U.draw_statement(rng)
        out += U.refused(st) is not None
        assert 1 <= len(st.segments) <= 4 and all(1 <= n <= 3000 and sum(br) == n for n, br in st.segments)
        for name, kind, operand in st.leaves:
            if kind == "in":
                assert 0 <= len(operand) <= 40
                lists += 1
                empties += not operand
                col = np.concatenate([c[U.COLS.index(name)] for c in st.cols]).astype(np.int64)
                present += int(np.isin(np.array(operand, dtype=np.int64), col).sum()) if operand else 0
        assert any(kind == "in" for _, kind, _ in st.leaves)
        m = U.truth(st, 0)
        assert m.dtype == bool and m.size == st.segments[0][0]
    assert out <= 20 and lists >= 200 and present > 0.3 * 20 * lists and empties >= 1


# ---- 4. the host unit alone under the sanitizers ---------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_list_plan_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "int_list_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "int_list_asan.cpp"), os.path.join(ROOT, "immutable3_amd", "csrc", "imm3_int_list_plan.cpp"),
                           "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 32 and all(ln.endswith(" ok") for ln in lines), r.stdout
