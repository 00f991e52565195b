"""IMM3_EXPR_NOT on the host (no device): the normal form of trees with complements (csrc/imm3_expr_norm.cpp through
imm3_expr_normalize) -- NOT pushed down to the leaves, complemented intervals, negated IN-lists, the universal term -- against the
tree's own truth table, the pinned shapes, the program's errors, the engines' flag, and the normaliser alone in a stand-alone
program built with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, EQ, GT, LT, MATCH
from expr_not_util import AND, NOT, OR, combine, has_not, postfix, random_tree
from immutable3_amd import native
from oracle import oracle_np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CODECS, WIDTHS = [DENSE_INT, DENSE_TINYINT, DENSE_STRING, DENSE_STRING], [4, 1, 2, 4]
CODES2 = [b"CA", b"NY", b"TX", b"WA"]
CODES4 = [b"ab12", b"zz00", b"q\\N\x00"]
INT_T = [-5.0, 0.0, 17.0, 1000.0, 2 ** 31 + 5.0, -2.0 ** 31, 2.0 ** 31 - 1]   # (saturating ones and the type's ends included)
BYTE_T = [-100.0, 18.0, 65.0, 127.0, -128.0, 200.0]                           # (200 narrows to -56: d.toByte)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
NOT_OP = native.EXPR_NOT


def random_leaf(rng):
    col = int(rng.integers(0, 4))
    if col >= 2:
        codes = CODES2 if col == 2 else CODES4
        k = int(rng.integers(1, len(codes)))
        vals = [codes[i] for i in rng.choice(len(codes), size=k, replace=False)]
        if rng.random() < 0.25:
            vals.append(b"XYZ")                         # wrong length for either column: can never match
        return (col, MATCH, vals)
    t = float(rng.choice(INT_T if col == 0 else BYTE_T))
    return (col, int(rng.choice([GT, LT, EQ])), t)


def probe_values():
    """per column: each threshold, its neighbours, the type's MIN and MAX, every list value and one value outside the lists"""
    ints = sorted({int(np.clip(oracle_np.to_int(t) + d, I32_MIN, I32_MAX)) for t in INT_T for d in (-1, 0, 1)} | {I32_MIN, I32_MAX})
    bytes_ = sorted({int(np.clip(oracle_np.to_byte(t) + d, -128, 127)) for t in BYTE_T for d in (-1, 0, 1)} | {-128, 127})
    return [np.array(ints, np.int32), np.array(bytes_, np.int8),
            np.array([list(v) for v in CODES2 + [b"ZZ"]], np.uint8), np.array([list(v) for v in CODES4 + [b"none"]], np.uint8)]


def probe_grid(cols_used):
    """the cross product of the probe values of the columns a tree uses (the others at their first value): one table of 4 columns"""
    vals = probe_values()
    axes = [np.arange(len(vals[c])) if c in cols_used else np.zeros(1, int) for c in range(4)]
    idx = np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")])
    return [vals[c][idx[c]] for c in range(4)]


def leaf_mask(leaf, table):
    col, cond, operand = leaf
    return np.asarray(oracle_np._predicate(table[col], CODECS[col], WIDTHS[col], cond, operand), bool)


def pred_mask(p, table):
    v = table[p["col"]]
    if "lo" in p:
        assert p["lo"] <= p["hi"], "empty terms are dropped"
        lo_full, hi_full = (I32_MIN, I32_MAX) if p["col"] == 0 else (-128, 127)
        assert (p["lo"], p["hi"]) != (lo_full, hi_full), "a predicate every value passes leaves its term"
        return (v.astype(np.int64) >= p["lo"]) & (v.astype(np.int64) <= p["hi"])
    key = "match" if "match" in p else "not_match"
    assert p[key], "an empty IN-list drops its term, an empty exclusion list leaves it"
    hit = np.zeros(v.shape[0], bool)
    for m in p[key]:
        assert len(m) == WIDTHS[p["col"]]
        hit |= (v == np.frombuffer(m, np.uint8)).all(axis=1)
    return hit if key == "match" else ~hit


def terms_mask(terms, table):
    out = np.zeros(table[0].shape[0], bool)
    for term in terms:
        keep = np.ones_like(out)
        assert len({p["col"] for p in term}) == len(term), "at most one predicate per column in a term"
        for p in term:
            keep &= pred_mask(p, table)
        out |= keep
    return out


def test_normal_form_has_the_trees_truth_table():
    rng = np.random.default_rng(4711)
    with_not = negated_lists = universal = 0
    for case in range(200):
        n = int(rng.integers(2, 7))
        leaves = [random_leaf(rng) for _ in range(n)]
        tree = random_tree(rng, n)
        terms = native.expr_normalize(CODECS, WIDTHS, leaves, postfix(tree))
        table = probe_grid({l[0] for l in leaves})
        want = combine(tree, [leaf_mask(l, table) for l in leaves])
        assert terms_mask(terms, table).tolist() == want.tolist(), (case, leaves, tree, terms)
        if terms == [[]]:
            assert want.all()
            universal += 1
        else:
            assert all(term for term in terms), "the universal term absorbs every other"
        with_not += has_not(tree)
        negated_lists += any("not_match" in p for t in terms for p in t)
    assert with_not >= 150 and negated_lists >= 30   # (the generator reaches complements, and they reach the terms)


def norm(leaves, tree):
    return native.expr_normalize(CODECS, WIDTHS, leaves, postfix(tree))


def test_double_not_is_the_operand():
    rng = np.random.default_rng(5)
    for _ in range(50):
        n = int(rng.integers(1, 6))
        leaves = [random_leaf(rng) for _ in range(n)]
        tree = random_tree(rng, n, p_not=0.0)
        assert norm(leaves, (NOT, (NOT, tree))) == norm(leaves, tree)
    # ... and the JSON itself, byte for byte
    import ctypes as C
    cs, keep = native._cselects([(1, GT, 18.0), (2, MATCH, [b"CA"])])
    cc, cw = np.array(CODECS, np.int32), np.array(WIDTHS, np.int32)
    texts = []
    for prog in ([0, 1, native.EXPR_OR], [0, 1, native.EXPR_OR, NOT_OP, NOT_OP], [0, NOT_OP, NOT_OP, 1, NOT_OP, NOT_OP, native.EXPR_OR]):
        pg = np.array(prog, np.int32)
        buf = C.create_string_buffer(4096)
        assert native.load().imm3_expr_normalize(cc.ctypes.data, cw.ctypes.data, 4, cs, 2, pg.ctypes.data, len(prog), C.cast(buf, C.c_void_p), 4096, None) == 0
        texts.append(buf.value)
    assert texts[0] == texts[1] == texts[2] == b'[[{"col":1,"lo":19,"hi":127}],[{"col":2,"match":["4341"]}]]'


# the pinned shapes: (leaves, tree, normal form)
PINNED = [
    # NOT EQ at the type's ends: one term (the other piece is empty); in the middle: two
    ([(1, EQ, -128.0)], (NOT, 0), [[{"col": 1, "lo": -127, "hi": 127}]]),
    ([(1, EQ, 127.0)], (NOT, 0), [[{"col": 1, "lo": -128, "hi": 126}]]),
    ([(0, EQ, -2.0 ** 31)], (NOT, 0), [[{"col": 0, "lo": I32_MIN + 1, "hi": I32_MAX}]]),
    ([(0, EQ, 2.0 ** 31 - 1)], (NOT, 0), [[{"col": 0, "lo": I32_MIN, "hi": I32_MAX - 1}]]),
    ([(0, EQ, 7.0)], (NOT, 0), [[{"col": 0, "lo": I32_MIN, "hi": 6}], [{"col": 0, "lo": 8, "hi": I32_MAX}]]),
    # a threshold that saturates: its complement is every row
    ([(0, GT, 1e12)], (NOT, 0), [[]]),
    ([(0, LT, -1e12)], (NOT, 0), [[]]),
    ([(0, GT, float("nan"))], (NOT, 0), [[{"col": 0, "lo": I32_MIN, "hi": 0}]]),       # NaN.toInt == 0
    ([(1, GT, 18.0)], (NOT, 0), [[{"col": 1, "lo": -128, "hi": 18}]]),
    ([(1, LT, 30.0)], (NOT, 0), [[{"col": 1, "lo": 30, "hi": 127}]]),
    # NotMatch
    ([(2, MATCH, [b"CA", b"NY", b"CA", b"XYZ"])], (NOT, 0), [[{"col": 2, "not_match": [b"CA", b"NY"]}]]),
    ([(2, MATCH, [b"XYZ", b"Q"])], (NOT, 0), [[]]),                                    # wrong lengths only: no exclusion at all
    ([(3, MATCH, [b"ab12"])], (NOT, 0), [[{"col": 3, "not_match": [b"ab12"]}]]),
    # x or not x / x and not x, for a leaf of every kind
    ([(1, GT, 18.0)], (OR, 0, (NOT, 0)), [[]]),
    ([(0, EQ, 7.0)], (OR, 0, (NOT, 0)), [[]]),
    ([(0, EQ, 7.0)], (OR, (NOT, 0), 0), [[]]),
    ([(2, MATCH, [b"CA", b"NY"])], (OR, 0, (NOT, 0)), [[]]),
    ([(1, GT, 18.0)], (AND, 0, (NOT, 0)), []),
    ([(0, EQ, 7.0)], (AND, 0, (NOT, 0)), []),
    ([(2, MATCH, [b"CA", b"NY"])], (AND, 0, (NOT, 0)), []),
    # conjunctions on one string column
    ([(2, MATCH, [b"CA", b"NY"]), (2, MATCH, [b"NY", b"TX"])], (AND, (NOT, 0), (NOT, 1)), [[{"col": 2, "not_match": [b"CA", b"NY", b"TX"]}]]),
    ([(2, MATCH, [b"CA", b"NY"]), (2, MATCH, [b"NY", b"TX"])], (NOT, (OR, 0, 1)), [[{"col": 2, "not_match": [b"CA", b"NY", b"TX"]}]]),
    ([(2, MATCH, [b"CA", b"NY", b"TX"]), (2, MATCH, [b"NY"])], (AND, 0, (NOT, 1)), [[{"col": 2, "match": [b"CA", b"TX"]}]]),
    ([(2, MATCH, [b"CA", b"NY", b"TX"]), (2, MATCH, [b"NY"])], (AND, (NOT, 1), 0), [[{"col": 2, "match": [b"CA", b"TX"]}]]),
    ([(2, MATCH, [b"CA"]), (2, MATCH, [b"CA", b"NY"])], (AND, 0, (NOT, 1)), []),                  # the difference may be empty
    # De Morgan: not (age > 18 and age < 30) = age <= 18 or age >= 30
    ([(1, GT, 18.0), (1, LT, 30.0)], (NOT, (AND, 0, 1)), [[{"col": 1, "lo": -128, "hi": 18}], [{"col": 1, "lo": 30, "hi": 127}]]),
    ([(1, GT, 18.0), (2, MATCH, [b"CA"])], (NOT, (OR, 0, 1)), [[{"col": 1, "lo": -128, "hi": 18}, {"col": 2, "not_match": [b"CA"]}]]),
    # three terms that become one: [MIN, 4] and [6, MAX] stand, then [5, 5] merges with the first and the merged pair meets the
    # third (add_term's recursion); id < 5 or not id < 6 or id = 5
    ([(0, LT, 5.0), (0, EQ, 5.0), (0, LT, 6.0)], (OR, (OR, 0, (NOT, 2)), 1), [[]]),
    ([(0, LT, 5.0), (0, EQ, 5.0), (0, LT, 6.0)], (OR, (OR, 0, 1), (NOT, 2)), [[]]),
    ([(0, LT, 5.0), (0, EQ, 5.0), (0, LT, 6.0), (1, GT, 18.0)], (OR, (OR, (AND, 0, 3), (AND, 3, (NOT, 2))), (AND, 1, 3)), [[{"col": 1, "lo": 19, "hi": 127}]]),
    ([(0, LT, 5.0), (0, EQ, 5.0), (0, LT, 7.0)], (OR, (OR, 0, (NOT, 2)), 1), [[{"col": 0, "lo": 7, "hi": I32_MAX}], [{"col": 0, "lo": I32_MIN, "hi": 5}]]),   # (a gap at 6: two terms, the merged one last)
    # a universal operand: the identity under AND, absorbing under OR
    ([(0, GT, 1e12), (1, GT, 18.0)], (AND, (NOT, 0), 1), [[{"col": 1, "lo": 19, "hi": 127}]]),
    ([(0, GT, 1e12), (1, GT, 18.0)], (OR, 1, (NOT, 0)), [[]]),
]


@pytest.mark.parametrize("leaves,tree,want", PINNED)
def test_pinned_shapes(leaves, tree, want):
    assert norm(leaves, tree) == want


@pytest.mark.parametrize("prog,what", [
    ([NOT_OP], "stack underflow"), ([NOT_OP, 0], "stack underflow"), ([0, 1, NOT_OP], "more than one result"),
    ([0, 1, -3], "unknown operator"), ([0, -7], "unknown operator"), ([0, NOT_OP, 2, native.EXPR_OR], "out of range"),
])
def test_malformed_programs(prog, what):
    leaves = [(0, GT, 1.0), (1, LT, 5.0)]
    with pytest.raises(native.Imm3Error) as e:
        native.expr_normalize(CODECS, WIDTHS, leaves, prog)
    assert e.value.code == native.ERR_ARG and what in e.value.msg


def test_notmatch_leaves_stay_unsupported_and_not_is_minus_four():
    from conftest import NOOP, NOTMATCH
    assert native.EXPR_NOT == -4 and (native.EXPR_AND, native.EXPR_OR) == (-1, -2)
    for cond in (NOTMATCH, NOOP):
        with pytest.raises(native.Imm3Error) as e:
            native.expr_normalize(CODECS, WIDTHS, [(2, cond, [b"CA"] if cond == NOTMATCH else None)], [0, NOT_OP])
        assert e.value.code == native.ERR_UNSUPPORTED_CONDITION and e.value.msg.startswith("Unsupported condition")


def test_a_complemented_eq_counts_as_two_terms():
    # not (id = 0 or id = 10 or ...) over k values is ONE column's k + 1 gaps; AND-ed over three columns: (k + 1)^3 terms
    def not_any(idx):
        t = idx[0]
        for i in idx[1:]:
            t = (OR, t, i)
        return (NOT, t)
    leaves = [(0, EQ, float(10 * i)) for i in range(3)] + [(1, EQ, float(10 * i)) for i in range(3)]
    assert len(norm(leaves, (AND, not_any([0, 1, 2]), not_any([3, 4, 5])))) == 16
    leaves = [(0, EQ, float(10 * i)) for i in range(8)] + [(1, EQ, float(10 * i)) for i in range(8)]
    with pytest.raises(native.Imm3Error) as e:
        norm(leaves, (AND, not_any(list(range(8))), not_any(list(range(8, 16)))))      # 9 x 9 = 81 > 64
    assert e.value.code == native.ERR_ARG and "terms" in e.value.msg


def test_python_engine_flag():
    from immutable3_amd import query as Q
    from immutable3_amd.operators import Engine, SelectOp, SelectTreeOp, has_not_match, select_program
    leaf = Q.Select("state", Q.NotMatch(["CA"]))
    under_and = Q.And(Q.Select("age", Q.GT(30)), leaf)
    under_or = Q.Or(Q.Select("age", Q.GT(30)), leaf)
    for sel in (leaf, under_and, under_or):
        q = Q.Query("test_100", sel, Q.Project(["id"], 0))
        assert has_not_match(sel)
        off = Engine(None)._select_ops(q)                                   # default: the reference's chain, which raises on the leaf
        assert all(isinstance(f(None), SelectOp) for f in off)
        assert any(isinstance(f(None).cond, Q.NotMatch) for f in off)
        on = Engine(None, honour_not_match=True)._select_ops(q)
        assert len(on) == 1 and isinstance(on[0](None), SelectTreeOp) and on[0](None).honour_not_match
    leaves, prog = select_program(under_or, honour_not_match=True)
    assert [(c, type(k).__name__) for c, k in leaves] == [("age", "GT"), ("state", "Match")] and list(leaves[1][1].values) == ["CA"]
    assert prog == [0, 1, native.EXPR_NOT, native.EXPR_OR]
    leaves, prog = select_program(under_or)
    assert isinstance(leaves[1][1], Q.NotMatch) and prog == [0, 1, native.EXPR_OR]       # off: the leaf as it is
    # an Or tree under honour_and_or alone keeps rejecting the leaf; a tree without NotMatch is untouched by the new flag
    assert not Engine(None, honour_and_or=True)._select_ops(Q.Query("t", under_or, Q.Project(["id"], 0)))[0](None).honour_not_match
    flat = Q.Query("t", Q.And(Q.Select("age", Q.GT(18)), Q.Select("age", Q.LT(30))), Q.Project(["id"], 0))
    assert all(isinstance(f(None), SelectOp) for f in Engine(None, honour_not_match=True)._select_ops(flat))


# ---- the normaliser alone under AddressSanitizer + UBSan: a stand-alone program (tests/native/expr_not_asan.cpp) ----
# This leg is about the sanitizers: it holds the program's output against the library's own expr_normalize of the same programs, so
# it is no independent oracle.  The constants are PINNED's (and the truth tables), which check the library above.
# its leaves, in its order; the programs are the pinned shapes' (and the malformed ones), restated over these leaves
ASAN_LEAVES = [(0, GT, 1e12), (0, LT, -1e12), (0, GT, float("nan")), (0, EQ, -2.0 ** 31), (0, EQ, 2.0 ** 31 - 1), (0, EQ, 7.0),
               (1, EQ, -128.0), (1, EQ, 127.0), (1, GT, 18.0), (1, LT, 30.0),
               (2, MATCH, [b"CA"]), (2, MATCH, [b"CA", b"NY"]), (2, MATCH, [b"NY", b"TX"]), (2, MATCH, [b"XYZ", b"Q"]), (3, MATCH, [b"ab12"])]
A, O, N = native.EXPR_AND, native.EXPR_OR, native.EXPR_NOT
ASAN_PROGRAMS = [[i, N] for i in range(15)] + [[i, N, N] for i in (5, 10)] + [
    [8, 8, N, O], [5, 5, N, O], [5, N, 5, O], [11, 11, N, O], [8, 8, N, A], [5, 5, N, A], [11, 11, N, A],
    [11, N, 12, N, A], [11, 12, O, N], [11, 12, N, A], [12, N, 11, A], [10, 11, N, A], [8, 9, A, N], [8, 10, O, N],
    [0, N, 8, A], [8, 0, N, O], [8, 9, A, N, 10, N, 5, N, A, O], [3, N, 4, N, A, 6, N, A, 7, N, A, 14, N, O],
    [N], [0, 1, N], [0, 1, -3], [0, -7],
]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_normaliser_alone_under_address_and_ub_sanitizers(tmp_path):
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    exe = str(tmp_path / "expr_not_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",   # (the runtimes inside the program)
                           "-D__HIP_PLATFORM_AMD__", "-I", hip_inc,
                           os.path.join(HERE, "native", "expr_not_asan.cpp"), os.path.join(ROOT, "immutable3_amd", "csrc", "imm3_expr_norm.cpp"),
                           "-o", exe])
    text = "".join(" ".join(str(v) for v in prog) + "\n" for prog in ASAN_PROGRAMS)
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(ASAN_PROGRAMS)
    import json
    for prog, line in zip(ASAN_PROGRAMS, lines):
        try:
            want = native.expr_normalize(CODECS, WIDTHS, ASAN_LEAVES, prog)
        except native.Imm3Error as e:
            assert line == f"error {e.code} {e.msg}", (prog, line)
            continue
        got = json.loads(line)
        for t in got:
            for p in t:
                for key in ("match", "not_match"):
                    if key in p:
                        p[key] = [bytes.fromhex(h) for h in p[key]]
        assert got == want, (prog, line)
