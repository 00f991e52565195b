#!/usr/bin/env python3
"""Development tool: what a one-launch disjunction costs.  For I8, I32, I8 + I32 and S2 + I8 predicate columns and T = 1, 2, 4, 8
terms over `rows` rows (default 100 M), kernel time of the select launch by the library's event timing (kernel id 0):
  (a) the tree query (imm3_query_create_expr): ONE launch of k_filter_expr;
  (b) the conjunctive query over the same columns through imm3_query_create: k_filter_tile, which reads the same bytes -- the floor;
  (c) the sum of the T single-term conjunctive runs: what the disjunction costs without the tree (before the host ORs the bitmaps).
The queries of one shape are alternated round by round in one process; medians.  Every tree's count is checked against numpy.
With IMM3_LIB_PATH pointing at another build of the library (one without the tree entry points), only (b) and (c) are measured.

    python tools/expr_bench.py [rows] [out.txt]"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS = 11
have_tree = hasattr(native.load(), "imm3_query_create_expr") and getattr(native.load().imm3_query_create_expr, "restype", None) is not None

ctx = native.Context(0)
ids = synth.uniform_int30(1, n)
age = synth.uniform_below(2, n, 100, np.int8)
st = synth.state_codes(3, n)
seg = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids.view(np.uint8), n * 4, synth.block_offsets(n, 4)),
                                 (native.DENSE_STRING, 2, st.reshape(-1), n * 2, synth.block_offsets(n, 2)),
                                 (native.DENSE_TINYINT, 1, age.view(np.uint8), n, synth.block_offsets(n, 1))])
codes = sorted({bytes(c) for c in st[:100_000]})
GT, LT, MATCH = native.GT, native.LT, native.MATCH


def is_code(code):
    return (st[:, 0] == code[0]) & (st[:, 1] == code[1])


def term(shape, t):
    """term t of a shape: (leaves over the shape's used columns, numpy mask); ~1/16 of the rows each, disjoint in the first column"""
    if shape == "I8":
        return [(0, GT, 6.0 * t - 1), (0, LT, 6.0 * t + 6)], (age > 6 * t - 1) & (age < 6 * t + 6)
    step = 1 << 26
    if shape == "I32":
        return [(0, GT, float(step * t)), (0, LT, float(step * t + step))], (ids > step * t) & (ids < step * t + step)
    if shape == "I8+I32":
        return [(0, GT, 6.0 * t - 1), (0, LT, 6.0 * t + 6), (1, LT, float(1 << 29))], (age > 6 * t - 1) & (age < 6 * t + 6) & (ids < (1 << 29))
    return [(0, MATCH, [codes[t]]), (1, GT, 50.0)], is_code(codes[t]) & (age > 50)


USED = {"I8": [2], "I32": [0], "I8+I32": [2, 0], "S2+I8": [1, 2]}
lines = [f"# rows = {n}; kernel time of the select launch (us), median of {ROUNDS} alternated rounds", f"# tree entry points: {'yes' if have_tree else 'no (older build: b and c only)'}",
         f"{'shape':8s} {'T':>2s} {'(a) tree':>10s} {'(b) conj':>10s} {'(c) T runs':>11s} {'a/b':>6s} {'a/c':>6s}"]
for shape in ("I8", "I32", "I8+I32", "S2+I8"):
    for T in (1, 2, 4, 8):
        terms = [term(shape, t) for t in range(T)]
        singles = [native.DeviceQuery(ctx, seg, USED[shape], lv) for lv, _ in terms]
        queries = list(singles)
        if have_tree:
            leaves, prog = [], []
            for ti, (lv, _) in enumerate(terms):
                first = len(leaves)
                leaves += lv
                prog += [first] + [x for i in range(first + 1, len(leaves)) for x in (i, native.EXPR_AND)] + ([native.EXPR_OR] if ti else [])
            if T == 1:   # one term twice: still a tree query (duplicates are dropped in the normal form)
                leaves, prog = leaves + leaves, prog + [len(leaves) + p if p >= 0 else p for p in prog] + [native.EXPR_OR]
            tree = native.DeviceQuery(ctx, seg, USED[shape], leaves, expr=prog)
            queries.append(tree)
        for q in queries:
            q.run_select()
            q.sync()
        if have_tree:
            want = np.zeros(n, bool)
            for _, m in terms:
                want |= m
            assert tree.count() == int(want.sum()) and tree.expr_form() == native.EXPR_FORM_TILE, (shape, T)
        ctx.timing_enable(ROUNDS * len(queries) + 8)
        ctx.timing_mask(1)
        ctx.timing_reset()
        for _ in range(ROUNDS):
            for q in queries:
                q.run_select()
        ctx.sync()
        us = ctx.timing_collect(0).reshape(ROUNDS, len(queries)) * 1e3
        ctx.timing_enable(0)
        b = float(np.median(us[:, 0]))
        c = float(np.median(us[:, :T].sum(axis=1)))
        a = float(np.median(us[:, T])) if have_tree else float("nan")
        lines.append(f"{shape:8s} {T:2d} {a:10.1f} {b:10.1f} {c:11.1f} {a / b:6.2f} {a / c:6.2f}")
        print(lines[-1], flush=True)
        for q in queries:
            q.close()
text = "\n".join(lines) + "\n"
print(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
