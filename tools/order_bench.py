#!/usr/bin/env python3
"""Development tool: what ORDER BY costs (imm3_query_set_order; csrc/imm3_order.hip).  Over `rows` rows (default 100 M), on the
survivors of age in (18, 30) (about 11 %), three queries:
    select id, age ... order by age desc limit 10        -- the radix select
    select id, age ... order by id desc                  -- the full sort of every survivor
    select id, state, age ... order by state, age limit 1000
For each: the time of the ORDER alone (the library's event timing, kernel id 7: from the key build's start to the apply's end) and of
the WHOLE query (an event pair on the context's stream around back-to-back runs of the settled query); medians of ROUNDS rounds.
Yardstick for the full sort: torch.sort(stable=True) of the same normalised keys (rocPRIM's tuned radix sort) plus one index gather
per SELECT-list column and for the row index, on the same device, timed the same way.  Then the select / full-sort threshold: `order by id desc limit survivors / f` for f = 1.5 .. 64 with the select pinned (tuning variant 24)
and with the full sort pinned (23).  Every result is checked against numpy.

    python tools/order_bench.py [rows] [out.txt]"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS, RUNS = 7, 5
GT, LT = native.GT, native.LT

ctx = native.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream)
ids = np.random.default_rng(1).permutation(n).astype(np.int32)          # id < 10^8: the key's top byte is constant at the default size
age = synth.uniform_below(2, n, 100, np.int8)
st = synth.state_codes(3, n)
seg = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids.view(np.uint8), n * 4, synth.block_offsets(n, 4)),
                                 (native.DENSE_STRING, 2, st.reshape(-1), n * 2, synth.block_offsets(n, 2)),
                                 (native.DENSE_TINYINT, 1, age.view(np.uint8), n, synth.block_offsets(n, 1))])
SELS = [(0, GT, 18.0), (0, LT, 30.0)]
keep = np.flatnonzero((age > 18) & (age < 30))


def event_us(fn, runs=RUNS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(runs):
        fn()
    b.record(stream)
    ctx.sync()
    return a.elapsed_time(b) / runs * 1e3


def measure(q):
    """(order alone, whole query) in us: medians"""
    q.run()
    q.row_count()
    whole, order = [], []
    for _ in range(ROUNDS):
        whole.append(event_us(q.run))
    ctx.timing_enable(4 * ROUNDS * RUNS)
    for _ in range(ROUNDS):
        q.run()
    ctx.sync()
    order = ctx.timing_collect(7) * 1e3
    ctx.timing_enable(0)
    return float(np.median(order)), float(np.median(whole))


lines = [f"# rows = {n}, survivors = {keep.size} ({100.0 * keep.size / n:.1f} %); us, medians of {ROUNDS} rounds",
         f"{'query':46s} {'path':>9s} {'order':>10s} {'query':>10s}"]
# ---- 1. order by age desc limit 10 ----
q = native.DeviceQuery(ctx, seg, [2, 0], SELS, [1, 0], 0, 1024)
q.set_order([(1, True)], 10)
o, w = measure(q)
idx, _ = q.fetch_rows()
assert idx.tolist() == keep[np.lexsort((keep, -age[keep].astype(np.int64)))][:10].tolist()
p = q.plan()
lines.append(f"{'order by age desc limit 10':46s} {'select' if p['order_select_runs'] else 'full':>9s} {o:10.1f} {w:10.1f}")
q.close()
# ---- 2. order by id desc (full) ----
q = native.DeviceQuery(ctx, seg, [2, 0], SELS, [1, 0], 0, 1024)
q.set_order([(0, True)], 0)
o_full, w_full = measure(q)
idx, vals = q.fetch_rows()
want = keep[np.argsort(-ids[keep].astype(np.int64), kind="stable")]
assert idx.tolist() == want.tolist() and vals[0].view("<i4").reshape(-1).tolist() == ids[want].tolist()
p = q.plan()
lines.append(f"{'order by id desc':46s} {'select' if p['order_select_runs'] else 'full':>9s} {o_full:10.1f} {w_full:10.1f}")
q.close()
# ---- 3. order by state, age limit 1000 ----
q = native.DeviceQuery(ctx, seg, [2, 0, 1], SELS, [1, 2, 0], 0, 1024)
q.set_order([(1, False), (2, False)], 1000)
o, w = measure(q)
idx, _ = q.fetch_rows()
sk = st[keep].astype(np.int64)
assert idx.tolist() == keep[np.lexsort((keep, age[keep].astype(np.int64), sk[:, 1], sk[:, 0]))][:1000].tolist()
p = q.plan()
lines.append(f"{'order by state, age limit 1000':46s} {'select' if p['order_select_runs'] else 'full':>9s} {o:10.1f} {w:10.1f}")
q.close()
# ---- yardstick: torch.sort(stable=True) of the normalised key of query 2 + one gather per column ----
with torch.cuda.stream(stream):
    row = torch.from_numpy(keep.astype(np.int64)).cuda()
    c_id = torch.from_numpy(ids[keep]).cuda()
    c_age = torch.from_numpy(age[keep]).cuda()
    key32 = torch.from_numpy(~ids[keep]).cuda()               # the 4-byte key: ~id as a signed int32 has the normalised key's order

    def torch_order():
        _, perm = torch.sort(key32, stable=True)
        return row[perm], c_id[perm], c_age[perm]

    torch_order()
    ctx.sync()
    t = []
    for _ in range(ROUNDS):
        t.append(event_us(torch_order))
    r, _, _ = torch_order()
    ctx.sync()
    assert r.cpu().numpy().tolist() == want.tolist()
torch_us = float(np.median(t))
lines.append(f"{'torch.sort(stable) + 3 gathers (order by id desc)':46s} {'':>9s} {torch_us:10.1f}")
lines.append(f"# full sort: order alone / torch = {o_full / torch_us:.2f}")
# ---- the select / full-sort threshold: order by id desc limit survivors / f, the select pinned (tuning 24) against the full sort (23) ----
lines.append("# threshold sweep, order by id desc limit L, the order alone: select pinned (tuning 24) vs full sort pinned (tuning 23)")
lines.append(f"{'survivors / L':>14s} {'L':>10s} {'select':>10s} {'full sort':>10s} {'select/full':>12s}")
for f in (1.5, 2, 3, 4, 6, 8, 16, 64):
    L = int(keep.size / f)
    q = native.DeviceQuery(ctx, seg, [2, 0], SELS, [1, 0], 0, 1024)
    q.set_order([(0, True)], L)
    t = {}
    for v in (native.TV_ORDER_SELECT_ALWAYS, native.TV_ORDER_FULL_SORT):
        ctx.set_tuning(v, 0)
        t[v], _ = measure(q)
    ctx.set_tuning(0, 0)
    idx, _ = q.fetch_rows()
    assert idx.tolist() == want[:L].tolist()
    q.close()
    lines.append(f"{f:14.1f} {L:10d} {t[native.TV_ORDER_SELECT_ALWAYS]:10.1f} {t[native.TV_ORDER_FULL_SORT]:10.1f} {t[native.TV_ORDER_SELECT_ALWAYS] / t[native.TV_ORDER_FULL_SORT]:12.2f}")
text = "\n".join(lines) + "\n"
print(text, end="")
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
seg.close()
ctx.close()
