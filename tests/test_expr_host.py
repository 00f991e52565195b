"""Select trees on the host (no device): the normal form the tree kernels evaluate (csrc/imm3_expr_norm.cpp through
include/imm3_diag.h's imm3_expr_normalize) -- a disjunction of terms, each a conjunction with at most one interval / IN-list per
column -- against the tree itself, and the program's and the leaves' errors."""
import itertools

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, EQ, GT, LT, MATCH, NOOP, NOTMATCH
from expr_util import AND, OR, combine, has_or, postfix, random_tree
from immutable3_amd import native
from oracle import oracle_np

CODECS, WIDTHS = [DENSE_INT, DENSE_TINYINT, DENSE_STRING], [4, 1, 2]
CODES = [b"CA", b"NY", b"TX", b"WA"]
INT_T = [-5.0, 0.0, 17.0, 1000.0, 2 ** 31 + 5.0]       # (the last narrows: d.toInt saturates)
BYTE_T = [-100.0, 18.0, 65.0, 127.0, 200.0]            # (200 narrows to -56: d.toByte)


def random_leaf(rng):
    col = int(rng.integers(0, 3))
    if col == 2:
        k = int(rng.integers(1, 4))
        vals = [CODES[i] for i in rng.choice(len(CODES), size=k, replace=False)]
        if rng.random() < 0.2:
            vals.append(b"XYZ")                         # wrong length: can never match
        return (2, MATCH, vals)
    t = float(rng.choice(INT_T if col == 0 else BYTE_T))
    return (col, int(rng.choice([GT, LT, EQ])), t)


def boundary_table():
    """every combination of each column's boundary values +- 1"""
    ints = sorted({int(np.clip(oracle_np.to_int(t) + d, -2 ** 31, 2 ** 31 - 1)) for t in INT_T for d in (-1, 0, 1)})
    bytes_ = sorted({int(np.clip(oracle_np.to_byte(t) + d, -128, 127)) for t in BYTE_T for d in (-1, 0, 1)} | {-128, 127})
    strs = CODES + [b"ZZ"]
    rows = list(itertools.product(ints, bytes_, range(len(strs))))
    c0 = np.array([r[0] for r in rows], np.int32)
    c1 = np.array([r[1] for r in rows], np.int8)
    c2 = np.array([list(strs[r[2]]) for r in rows], np.uint8)
    return c0, c1, c2


def leaf_mask(leaf, table):
    col, cond, operand = leaf
    return oracle_np._predicate(table[col], CODECS[col], WIDTHS[col], cond, operand)


def terms_mask(terms, table):
    out = np.zeros(table[0].shape[0], bool)
    for term in terms:
        keep = np.ones_like(out)
        assert len({p["col"] for p in term}) == len(term), "at most one predicate per column in a term"
        for p in term:
            v = table[p["col"]]
            if "match" in p:
                hit = np.zeros_like(out)
                for m in p["match"]:
                    assert len(m) == 2
                    hit |= (v[:, 0] == m[0]) & (v[:, 1] == m[1])
                keep &= hit
            else:
                assert p["lo"] <= p["hi"], "empty terms are dropped"
                keep &= (v.astype(np.int64) >= p["lo"]) & (v.astype(np.int64) <= p["hi"])
        out |= keep
    return out


def test_normal_form_has_the_trees_truth_table():
    rng = np.random.default_rng(2024)
    table = boundary_table()
    most = 0
    for case in range(400):
        n = int(rng.integers(1, 7))
        leaves = [random_leaf(rng) for _ in range(n)]
        tree = random_tree(rng, n)
        terms = native.expr_normalize(CODECS, WIDTHS, leaves, postfix(tree))
        want = combine(tree, [leaf_mask(l, table) for l in leaves])
        assert terms_mask(terms, table).tolist() == want.tolist(), (case, leaves, tree, terms)
        assert len(terms) <= 9, "6 leaves make at most 3 x 3 terms"
        most = max(most, len(terms))
    assert most >= 4   # (the generator reaches real disjunctions)


def test_tree_without_or_is_the_flat_fold():
    rng = np.random.default_rng(7)
    for _ in range(100):
        n = int(rng.integers(1, 7))
        leaves = [random_leaf(rng) for _ in range(n)]
        tree = 0
        for i in range(1, n):
            tree = (AND, tree, i) if rng.random() < 0.5 else (AND, i, tree)
        order = [op for op in postfix(tree) if op >= 0]
        # the fold of the flat list (csrc/imm3_api.cpp: fold_selects), per column in first-seen order
        fold = {}
        for i in order:
            col, cond, operand = leaves[i]
            if col == 2:
                vals = [v for k, v in enumerate(operand) if len(v) == 2 and v not in operand[:k]]
                fold[col] = vals if col not in fold else [v for v in fold[col] if v in vals]
            else:
                t = oracle_np.to_int(operand) if col == 0 else oracle_np.to_byte(operand)
                lo, hi = fold.get(col, ((-2 ** 31, 2 ** 31 - 1) if col == 0 else (-128, 127)))
                if cond == GT:
                    lo = max(lo, t + 1)
                elif cond == LT:
                    hi = min(hi, t - 1)
                else:
                    lo, hi = max(lo, t), min(hi, t)
                fold[col] = (lo, hi)
        empty = any((not v) if c == 2 else v[0] > v[1] for c, v in fold.items())
        terms = native.expr_normalize(CODECS, WIDTHS, leaves, postfix(tree))
        if empty:
            assert terms == []
            continue
        assert len(terms) == 1
        got = [(p["col"], p["match"] if "match" in p else (p["lo"], p["hi"])) for p in terms[0]]
        assert got == [(c, v) for c, v in fold.items()]


def test_duplicate_and_empty_terms_are_dropped():
    leaves = [(1, LT, 18.0), (1, GT, 65.0), (1, LT, 18.0), (1, GT, 127.0)]
    assert native.expr_normalize(CODECS, WIDTHS, leaves, postfix((OR, 0, 2))) == [[{"col": 1, "lo": -128, "hi": 17}]]
    assert native.expr_normalize(CODECS, WIDTHS, leaves, postfix((AND, 0, 1))) == []           # age < 18 and age > 65
    assert native.expr_normalize(CODECS, WIDTHS, leaves, postfix((OR, 0, 3))) == [[{"col": 1, "lo": -128, "hi": 17}]]
    assert native.expr_normalize(CODECS, WIDTHS, leaves, postfix((OR, 0, 1))) == [[{"col": 1, "lo": -128, "hi": 17}], [{"col": 1, "lo": 66, "hi": 127}]]
    assert native.expr_normalize(CODECS, WIDTHS, [], []) == []


@pytest.mark.parametrize("prog,what", [
    ([native.EXPR_OR], "underflow"), ([0, native.EXPR_AND], "underflow"), ([0, 1], "more than one result"),
    ([0, 2, native.EXPR_OR], "out of range"), ([0, 1, -3], "unknown operator"), ([], "empty"),
])
def test_malformed_programs(prog, what):
    leaves = [(0, GT, 1.0), (1, LT, 5.0)]
    with pytest.raises(native.Imm3Error) as e:
        native.expr_normalize(CODECS, WIDTHS, leaves, prog)
    assert e.value.code == native.ERR_ARG and what in e.value.msg


def test_more_than_64_terms():
    # (a0 or b0) and (a1 or b1) and ... : 2^k terms over distinct values of ONE column would collapse, so alternate three columns'
    # disjoint intervals: 3 columns x 4 alternatives = 64 terms pass, one more alternative does not
    def alternatives(col, k):
        return [(col, EQ, float(10 * i)) for i in range(k)]

    def ors(idx):
        t = idx[0]
        for i in idx[1:]:
            t = (OR, t, i)
        return t

    for k2, ok in ((4, True), (5, False)):
        leaves = alternatives(0, 4) + alternatives(1, 4) + [(2, MATCH, [c]) for c in (CODES + [b"DC"])[:k2]]
        tree = (AND, (AND, ors(list(range(0, 4))), ors(list(range(4, 8)))), ors(list(range(8, 8 + k2))))
        if ok:
            assert len(native.expr_normalize(CODECS, WIDTHS, leaves, postfix(tree))) == 64
        else:
            with pytest.raises(native.Imm3Error) as e:
                native.expr_normalize(CODECS, WIDTHS, leaves, postfix(tree))
            assert e.value.code == native.ERR_ARG and "terms" in e.value.msg


def test_leaf_errors_keep_their_codes_and_texts():
    for cond in (NOTMATCH, NOOP):
        with pytest.raises(native.Imm3Error) as e:
            native.expr_normalize(CODECS, WIDTHS, [(0, GT, 1.0), (0, cond, None)], [0, 1, native.EXPR_OR])
        assert e.value.code == native.ERR_UNSUPPORTED_CONDITION and e.value.msg.startswith("Unsupported condition")
    for leaf in ((2, GT, 1.0), (0, MATCH, [b"CA"])):
        with pytest.raises(native.Imm3Error) as e:
            native.expr_normalize(CODECS, WIDTHS, [leaf, (1, LT, 3.0)], [0, 1, native.EXPR_OR])
        assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    with pytest.raises(native.Imm3Error) as e:
        native.expr_normalize([9], [4], [(0, GT, 1.0)], [0])
    assert e.value.code == native.ERR_NO_CODEC and e.value.msg.startswith("No implementation for")


def test_has_or_helper():
    assert has_or((AND, 0, (OR, 1, 2))) and not has_or((AND, 0, (AND, 1, 2))) and not has_or(0)


def test_python_engine_flag_off_is_the_old_chain_and_on_is_one_tree_operator():
    from immutable3_amd import query as Q
    from immutable3_amd.operators import Engine, SelectOp, SelectTreeOp, has_or as tree_has_or, resolveSelectOps, select_program
    sel = Q.And(Q.Or(Q.Select("age", Q.LT(18)), Q.Select("age", Q.GT(65))), Q.Select("state", Q.Match(["CA"])))
    q = Q.Query("test_100", sel, Q.Project(["id", "age"], 0))
    off, ref = Engine(None)._select_ops(q), resolveSelectOps(q)           # default: the reference's conjunction, leaf by leaf
    assert len(off) == len(ref) == 3
    for a, b in zip(off, ref):
        x, y = a(None), b(None)
        assert isinstance(x, SelectOp) and (x.col, x.cond) == (y.col, y.cond)
    on = Engine(None, honour_and_or=True)._select_ops(q)
    assert len(on) == 1 and isinstance(on[0](None), SelectTreeOp)
    leaves, prog = select_program(sel)
    assert [c for c, _ in leaves] == ["age", "age", "state"] and prog == [0, 1, native.EXPR_OR, 2, native.EXPR_AND]
    # a tree without Or keeps the old operators (and the table plan) under either setting
    flat = Q.Query("test_100", Q.And(Q.Select("age", Q.GT(18)), Q.Select("age", Q.LT(30))), Q.Project(["id"], 0))
    assert not tree_has_or(flat.select) and tree_has_or(sel)
    assert all(isinstance(f(None), SelectOp) for f in Engine(None, honour_and_or=True)._select_ops(flat))


def test_cli_switch_is_off_by_default_and_prints_the_program_when_on():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "immutable3_amd", "bin", "imm3_sql")
    golden = os.path.join(root, "tests", "golden")
    sql = "select id, age from test_100 where ((age < 20 or age > 60) and state = 'CA')"
    off = subprocess.run([exe, "--parse-only", "-q", sql, "-d", golden], capture_output=True, text=True, check=True).stdout
    on = subprocess.run([exe, "--parse-only", "--honour-and-or", "-q", sql, "-d", golden], capture_output=True, text=True, check=True).stdout
    assert "leaves: age:LT(20) age:GT(60) state:" in off and "program:" not in off      # the old resolveSelectOps result, nothing else
    assert on.startswith(off) and on[len(off):] == "program: 0 1 OR 2 AND\n"
    flat = "select id from test_100 where (age > 18 and age < 30)"
    a = subprocess.run([exe, "--parse-only", "-q", flat, "-d", golden], capture_output=True, text=True, check=True).stdout
    b = subprocess.run([exe, "--parse-only", "--honour-and-or", "-q", flat, "-d", golden], capture_output=True, text=True, check=True).stdout
    assert a == b                                                                         # no Or: the switch changes nothing
