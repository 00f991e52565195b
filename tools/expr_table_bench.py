#!/usr/bin/env python3
"""Development tool: what the one table-tree launch buys.  I8 + I32 predicate columns, the two-term tree of
tests/test_gpu_zz_perf_expr.py -- (age < 18 and id < 2^29) or (age > 65 and id > 2^29) -- over a table cut into segments; kernel
time of the select launch by the library's event timing (kernel id 0):
  (a) the table tree query (imm3_query_create_table_expr): ONE launch of k_filter_expr's TABLE instance over all segments;
  (c) the sum of the per-segment tree launches it replaces (imm3_query_create_expr on every segment; kernel times only: the gaps
      between the dependent launches are not counted);
  (b) one conjunctive table launch over the same columns (imm3_query_create_table, the first term): k_filter_tile's TABLE instance,
      which reads the same bytes -- the floor;
  (w) the single-segment tree launch over the same rows as ONE segment.
All queries are alternated round by round in one process; medians of 11.  The table's count is checked against numpy.

    python tools/expr_table_bench.py [out.txt]       # 64 x 262 144 rows, then 100 M rows as 98 segments of <= 1 024 000"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

out_path = sys.argv[1] if len(sys.argv) > 1 else None
ROUNDS = 11
GT, LT = native.GT, native.LT
T1 = [(0, LT, 18.0), (1, LT, float(1 << 29))]
T2 = [(0, GT, 65.0), (1, GT, float(1 << 29))]
PROG = [0, 1, native.EXPR_AND, 2, 3, native.EXPR_AND, native.EXPR_OR]


def measure(ctx, seg_rows):
    n = int(sum(seg_rows))
    ids = synth.uniform_int30(1, n)
    age = synth.uniform_below(2, n, 100, np.int8)

    def segment(lo, hi):
        m = hi - lo
        return native.DeviceSegment(ctx, [(native.DENSE_TINYINT, 1, age[lo:hi].view(np.uint8), m, synth.block_offsets(m, 1)),
                                         (native.DENSE_INT, 4, ids[lo:hi].view(np.uint8), m * 4, synth.block_offsets(m, 4))])
    bounds = np.concatenate([[0], np.cumsum(seg_rows)])
    segs = [segment(int(bounds[i]), int(bounds[i + 1])) for i in range(len(seg_rows))]
    whole = segment(0, n)
    table = native.DeviceTable(ctx, segs)
    q_table = native.DeviceQuery(ctx, table, [0, 1], T1 + T2, expr=PROG)
    q_segs = [native.DeviceQuery(ctx, s, [0, 1], T1 + T2, expr=PROG) for s in segs]
    q_conj = native.DeviceQuery(ctx, table, [0, 1], T1)
    q_whole = native.DeviceQuery(ctx, whole, [0, 1], T1 + T2, expr=PROG)
    queries = [q_table] + q_segs + [q_conj, q_whole]
    for q in queries:
        q.run_select()
        q.sync()
    want = int((((age < 18) & (ids < (1 << 29))) | ((age > 65) & (ids > (1 << 29)))).sum())
    assert q_table.count() == want == sum(q.count() for q in q_segs) == q_whole.count() and q_table.expr_form() == native.EXPR_FORM_TILE
    ctx.timing_enable(ROUNDS * len(queries) + 8)
    ctx.timing_mask(1)
    ctx.timing_reset()
    for _ in range(ROUNDS):
        for q in queries:
            q.run_select()
    ctx.sync()
    us = ctx.timing_collect(0).reshape(ROUNDS, len(queries)) * 1e3
    ctx.timing_enable(0)
    k = len(segs)
    a, c = float(np.median(us[:, 0])), float(np.median(us[:, 1:1 + k].sum(axis=1)))
    b, w = float(np.median(us[:, 1 + k])), float(np.median(us[:, 2 + k]))
    for q in queries:
        q.close()
    table.close()
    whole.close()
    for s in segs:
        s.close()
    return f"{n:11d} {k:5d} {a:10.1f} {c:12.1f} {b:10.1f} {w:10.1f} {c / a:6.2f} {a / b:6.2f} {a / w:6.2f}"


ctx = native.Context(0)
lines = [f"# I8 + I32, two terms; kernel time of the select launch (us), median of {ROUNDS} alternated rounds",
         f"{'rows':>11s} {'segs':>5s} {'(a) table':>10s} {'(c) per-seg':>12s} {'(b) conj':>10s} {'(w) whole':>10s} {'c/a':>6s} {'a/b':>6s} {'a/w':>6s}"]
print("\n".join(lines), flush=True)
for seg_rows in ([262144] * 64, [1_024_000] * 97 + [100_000_000 - 97 * 1_024_000]):
    lines.append(measure(ctx, seg_rows))
    print(lines[-1], flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
