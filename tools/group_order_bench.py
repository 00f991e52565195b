#!/usr/bin/env python3
"""Development tool: what ORDER BY over groups costs (imm3_query_set_group_order; csrc/imm3_group_order.hip).  Over 1 M rows:
    select count(id) from t group by state order by id_count desc limit 10     -- 51 groups: the one-work-group launch
    select max(age) from t group by id order by age_max desc limit 10          -- 1 M groups: the radix path (select)
For each, the device time of the ordered settle's order launches (the library's event timing, kernel id 8: from the first order
kernel's start to the last one's end; medians of ROUNDS settles) by the path the library takes and -- on 51 groups -- by the radix path
pinned (tuning variant 25); the 1 M groups also as a full sort (no limit).  Then the wall time of set_group_order + fetch_groups on
the 1 M groups against what a caller did before: fetch_groups of every group, unordered, plus np.lexsort.  Every result is checked
against numpy.

    python tools/group_order_bench.py [out.txt]        (the committed copy: profiles/group_order.txt)"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

out_path = sys.argv[1] if len(sys.argv) > 1 else None
N, ROUNDS = 1_000_000, 15
C, MX, A = native.AGG_COUNT, native.AGG_MAX, native.GROUP_ORDER_AGG
PATHS = {native.GROUP_ORDER_SMALL: "small", native.GROUP_ORDER_RADIX_FULL: "radix full", native.GROUP_ORDER_RADIX_SELECT: "radix select"}

rng = np.random.default_rng(8)
ctx = native.Context(0)
ids = rng.permutation(N).astype(np.int32)
age = rng.integers(-128, 128, size=N).astype(np.int8)
states = np.array([list(b"%c%c" % (65 + i // 26, 65 + i % 26)) for i in range(51)], np.uint8)[rng.integers(0, 51, size=N)]
seg = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids.view(np.uint8), N * 4, synth.block_offsets(N, 4)),
                                 (native.DENSE_STRING, 2, states.reshape(-1), N * 2, synth.block_offsets(N, 2)),
                                 (native.DENSE_TINYINT, 1, age.view(np.uint8), N, synth.block_offsets(N, 1))])
ctx.timing_enable(4 * ROUNDS)
ctx.timing_mask(1 << 8)


def settle_us(q, order, limit, variant=0):
    """(median device time of one ordered settle's order launches in us, the path it took)"""
    ctx.set_tuning(variant, 0)
    q.set_group_order(order, limit)
    q.fetch_groups()
    ctx.timing_reset()
    for _ in range(ROUNDS):
        q.set_group_order(order, limit)
        q.fetch_groups()
    t = ctx.timing_collect(8) * 1e3
    path = PATHS[q.group_order_path()]
    ctx.set_tuning(0, 0)
    return float(np.median(t)), path


lines = [f"# rows = {N}; device time of the order launches of one ordered settle (kernel id 8), us, medians of {ROUNDS} settles",
         f"{'statement':58s} {'groups':>8s} {'path':>13s} {'order':>10s}"]
# ---- 51 groups ----
q = native.DeviceQuery(ctx, seg, [0, 1], [], (), 0, 1024, group_cols=[1], aggs=[(C, 0)])
q.run()
order = [(A, 0, True)]
small, p_small = settle_us(q, order, 10)
res = q.fetch_groups()
counts = np.bincount(np.unique(states.view(np.uint16).reshape(-1), return_inverse=True)[1].reshape(-1))
assert res[2].tolist() == sorted(counts.tolist(), reverse=True)[:10]
radix51, p_radix51 = settle_us(q, order, 10, native.TV_GROUP_ORDER_RADIX)
assert [x.tolist() for x in q.fetch_groups()] == [x.tolist() for x in res]
stmt = "group by state order by id_count desc limit 10"
lines.append(f"{stmt:58s} {51:8d} {p_small:>13s} {small:10.1f}")
lines.append(f"{stmt + ' (tuning 25)':58s} {51:8d} {p_radix51:>13s} {radix51:10.1f}")
lines.append(f"# 51 groups: small launch / pinned radix path = {small / radix51:.3f}")
q.close()
# ---- 1 M groups ----
q = native.DeviceQuery(ctx, seg, [0, 2], [], (), 0, 1024, group_cols=[0], aggs=[(MX, 1)])
q.run()
assert q.fetch_groups()[1].size == N
sel, p_sel = settle_us(q, order, 10)
new = tuple(x.tolist() for x in q.fetch_groups())
want = np.lexsort((np.arange(N), -age.astype(np.int64)))[:10]
assert new[1] == want.tolist()
full, p_full = settle_us(q, order, 0)
stmt = "group by id order by age_max desc limit 10"
lines.append(f"{stmt:58s} {N:8d} {p_sel:>13s} {sel:10.1f}")
lines.append(f"{'group by id order by age_max desc':58s} {N:8d} {p_full:>13s} {full:10.1f}")
# ---- wall time: ordered top-10 against fetch everything + lexsort ----
t_new, t_old = [], []
for _ in range(5):
    q.set_group_order([], 0)
    ctx.sync()
    t0 = time.perf_counter()
    keys, first, cnt, vals = q.fetch_groups()
    top = np.lexsort((first, -vals[:, 0]))[:10]
    old = (keys[top].tolist(), first[top].tolist(), cnt[top].tolist(), vals[top].tolist())
    t_old.append(time.perf_counter() - t0)
    ctx.sync()
    t0 = time.perf_counter()
    q.set_group_order(order, 10)
    got = tuple(x.tolist() for x in q.fetch_groups())
    t_new.append(time.perf_counter() - t0)
    assert got == old == new
new_ms, old_ms = float(np.median(t_new)) * 1e3, float(np.median(t_old)) * 1e3
lines.append(f"# top-10 of {N} groups, wall time, ms, medians of 5: set_group_order + fetch_groups {new_ms:.2f}; fetch_groups of every group + np.lexsort {old_ms:.2f}; ratio {new_ms / old_ms:.3f}")
q.close()
text = "\n".join(lines) + "\n"
print(text, end="")
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
seg.close()
ctx.close()
