#!/usr/bin/env python3
"""Development tool: what IN (sub-query) costs, by the two routes a caller has.  Over `rows` rows on either side (default 100 M), with
10^3 / 10^5 / 10^6 / 10^7 distinct values in the inner selection (half the inner rows are selected), wall-clock time of the whole
route, host work included:
  new   imm3_int_set_create over the inner query + creation of the consumer with the IMM3_INT_IN_SET leaf + its run + its count
  old   imm3_query_fetch_rows of the inner projection + numpy.unique over the fetched values + creation of the consumer with
        IMM3_INT_IN over them (query creation builds the probe table on the CPU and uploads it) + its run + its count.
Both inner queries have run before the clock starts.  The routes are alternated round by round in one process; medians.  The new
route's three steps are also timed apart (set / consumer creation / run + count), which says where its time goes.  Every count is
checked against numpy.

    python tools/int_set_bench.py [rows] [out.txt] [rounds]"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
FORMS = {native.INT_LIST_I8: "I8", native.INT_LIST_ARGS: "ARGS", native.INT_LIST_LDS: "LDS", native.INT_LIST_GLOBAL: "GLOBAL"}

ctx = native.Context(0)
rng = np.random.default_rng(7)
lines = [f"# rows = {n} on either side; wall-clock ms of the whole route, median of {ROUNDS} alternated rounds (one warm-up round in front)",
         f"# {'distinct':>9s} {'form':>6s} {'new':>9s} {'old':>10s} {'new/old':>8s}   new = {'set':>8s} + {'create':>7s} + {'run':>7s}   host route"]
flag = rng.integers(-1, 1, size=n).astype(np.int8)
offs4, offs1 = synth.block_offsets(n, 4), synth.block_offsets(n, 1)
for distinct in (1_000, 100_000, 1_000_000, 10_000_000):
    if distinct * 4 > n:
        continue
    domain = rng.permutation(np.unique(rng.integers(0, 1 << 30, size=2 * distinct + distinct // 4 + 8)))[: 2 * distinct].astype(np.int32)   # distinct values, no permutation of the whole domain
    assert domain.size == 2 * distinct
    inner_ids = domain[rng.integers(0, distinct, size=n)]
    outer_ids = domain[rng.integers(0, 2 * distinct, size=n)]
    inner = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, inner_ids.view(np.uint8), n * 4, offs4), (native.DENSE_TINYINT, 1, flag.view(np.uint8), n, offs1)])
    outer = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, outer_ids.view(np.uint8), n * 4, offs4)])
    members = np.unique(inner_ids[flag > -1])
    want = int(np.isin(outer_ids, members).sum())
    src_select = native.DeviceQuery(ctx, inner, [1, 0], [(0, native.GT, -1.0)])
    src_project = native.DeviceQuery(ctx, inner, [1, 0], [(0, native.GT, -1.0)], [1], 0, 1024)
    src_select.run_select()
    src_project.run()
    src_select.sync(), src_project.sync()
    steps = []

    def new_route(describe=False):
        t0 = time.perf_counter()
        s = native.IntSet(ctx, [(src_select, 1)])
        t1 = time.perf_counter()
        q = native.DeviceQuery(ctx, outer, [0], [(0, native.INT_IN_SET, s)])
        t2 = time.perf_counter()
        q.run_select()
        c = q.count()
        t3 = time.perf_counter()
        steps.append((t1 - t0, t2 - t1, t3 - t2))
        info = (s.info(), s.table()[4]) if describe else None      # (table() copies the whole table: the warm-up round only)
        q.close(), s.close()
        return c, info

    def old_route():
        _, cols = src_project.fetch_rows()
        values = np.unique(cols[0].view("<i4").reshape(-1)).tolist()
        q = native.DeviceQuery(ctx, outer, [0], [(0, native.INT_IN, values)])
        q.run_select()
        c = q.count()
        q.close()
        return c

    (c_new, info), c_old = new_route(True), old_route()
    assert c_new == want and c_old == want and info[0][0] == members.size, (distinct, c_new, c_old, want, info)
    steps.clear()
    t_new, t_old = [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        new_route()
        t1 = time.perf_counter()
        old_route()
        t2 = time.perf_counter()
        t_new.append(t1 - t0)
        t_old.append(t2 - t1)
    new, old = float(np.median(t_new)) * 1e3, float(np.median(t_old)) * 1e3
    st = np.median(np.array(steps), axis=0) * 1e3
    lines.append(f"  {members.size:9d} {FORMS[info[0][3]]:>6s} {new:9.2f} {old:10.2f} {new / old:8.3f}         {st[0]:8.2f}   {st[1]:7.2f}   {st[2]:7.2f}   {info[1]}")
    print(lines[-1], flush=True)
    for h in (src_select, src_project, inner, outer):
        h.close()
text = "\n".join(lines) + "\n"
print(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
