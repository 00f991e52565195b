#!/usr/bin/env python3
"""Development tool: the group-by SUM (IMM3_AGG_SUM, AvgDoubleAggr's sum) against MAX over 100 M rows, group by state (51 keys),
each pair in the same process, alternated round by round, timed by the library's event timing of the aggregation launch (kernel id
4: with the select fused into it, the whole query).  Every sum is checked against numpy.  Output: profiles/agg_sum.txt.

    python tools/agg_sum_bench.py [rows] [out.txt]"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
RUNS, ROUNDS, AGG_KERNEL = 20, 7, 4
FORM = {0: "lanes", 1: "lanes-127", 2: "direct", 3: "tile", 4: "general"}
C, MX, S = native.AGG_COUNT, native.AGG_MAX, native.AGG_SUM

ctx = native.Context(0)
ids = np.arange(n, dtype=np.int32)
age = synth.uniform_below(2, n, 100, np.int8)
st = synth.state_codes(3, n)
seg = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids.view(np.uint8), n * 4, synth.block_offsets(n, 4)),
                                 (native.DENSE_STRING, 2, st.reshape(-1), n * 2, synth.block_offsets(n, 2)),
                                 (native.DENSE_TINYINT, 1, age.view(np.uint8), n, synth.block_offsets(n, 1))])
USED, COLS = [0, 1, 2], {"id": 0, "age": 2}
RANGE = [(2, native.GT, 18.0), (2, native.LT, 30.0)]
key = st[:, 0].astype(np.int64) | (st[:, 1].astype(np.int64) << 8)


def np_sums(col, mask):
    """exact per-state sums (float64 bincount is exact here: every partial sum stays below 2^53)"""
    v = (ids if col == "id" else age).astype(np.float64)
    return np.bincount(key[mask], weights=v[mask], minlength=1 << 16).astype(np.int64)


def make(aggs, sels):
    return native.DeviceQuery(ctx, seg, USED, sels, (), 0, 1024, group_cols=[1], aggs=[(k, COLS[c]) for k, c in aggs])


def check(q, aggs, sels):
    keys, first, counts, vals = q.fetch_groups()
    mask = np.ones(n, bool) if not sels else (age > 18) & (age < 30)
    for j, (k, c) in enumerate(aggs):
        if k == S:
            assert vals[:, j].tolist() == np_sums(c, mask)[keys.astype(np.int64)].tolist(), (aggs, sels)


def timed(q):
    ctx.timing_enable(RUNS + 8)
    ctx.timing_mask(1 << AGG_KERNEL)
    ctx.timing_reset()
    for _ in range(RUNS):
        q.run()
    ctx.sync()
    us = float(np.median(ctx.timing_collect(AGG_KERNEL))) * 1e3
    ctx.timing_enable(0)
    return us


def label(aggs):
    return ", ".join(f"{'count' if k == C else ('max' if k == MX else 'sum')}({c})" for k, c in aggs)


PAIRS = [([(C, "id"), (MX, "age")], [(C, "id"), (S, "age")]), ([(MX, "id")], [(S, "id")])]
lines = [f"group by state over {n} rows (51 keys); aggregation launch by event timing, median of {RUNS} runs per round, "
         f"{ROUNDS} rounds alternating the pair: median [min, max] of the round medians, us",
         f"{'query':48s} {'form':>9s} {'us':>8s} {'[min, max]':>16s} {'sum / max':>10s}"]
for sels, where in (([], ""), (RANGE, " where age > 18 and age < 30")):
    for base, new in PAIRS:
        qs = [make(base, sels), make(new, sels)]
        for q in qs:
            for _ in range(3):
                q.run()
        check(qs[1], new, sels)
        per = [[], []]
        for _ in range(ROUNDS):
            for i, q in enumerate(qs):
                per[i].append(timed(q))
        med = [float(np.median(p)) for p in per]
        for i, (q, aggs) in enumerate(zip(qs, (base, new))):
            ratio = f"{med[1] / med[0]:9.2f}x" if i == 1 else ""
            lines.append(f"{label(aggs) + where:48s} {FORM.get(q.agg_form(), '?'):>9s} {med[i]:8.1f} "
                         f"{'[%.1f, %.1f]' % (min(per[i]), max(per[i])):>16s} {ratio:>10s}")
        check(qs[1], new, sels)      # (after the timed runs too)
        for q in qs:
            q.close()
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
seg.close()
ctx.close()
