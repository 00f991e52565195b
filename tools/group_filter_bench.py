#!/usr/bin/env python3
"""Development tool: what HAVING over groups costs (imm3_query_set_group_filter; csrc/imm3_group_order.hip), row for row beside
tools/group_order_bench.py.  Over 1 M rows, three group counts:
    select count(id), sum(age) from t group by state  having ...     -- 51 groups: the one-work-group launch
    select count(id), sum(age) from t group by k      having ...     -- 2 048 groups: the largest the one-work-group launch takes
    select count(id), sum(age) from t group by id     having ...     -- 1 M groups: the radix path
each with a filter keeping about 1 %, about 50 % and all of its groups (on the count; on the 1 M one-row groups on the sum), with
`order by id_count desc limit 10` and unordered.  Per row: the device time of the view's launches (the library's event timing, kernel
id 8: from the first kernel's start to the last one's end; medians of ROUNDS settles), the wall time of set_group_filter +
set_group_order + fetch_groups, and the wall time of what a caller did without the filter: fetch_groups of every group, numpy filter,
np.lexsort, cut (medians of WALL rounds; for the new side also the smallest and the largest round).  Every filtered result is checked
against that numpy result.

    python tools/group_filter_bench.py [out.txt]        (the committed copy: the first part of profiles/group_filter.txt)"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

out_path = sys.argv[1] if len(sys.argv) > 1 else None
N, ROUNDS, WALL = 1_000_000, 15, 5
C, S, A = native.AGG_COUNT, native.AGG_SUM, native.GROUP_ORDER_AGG
PATHS = {native.GROUP_ORDER_SMALL: "small", native.GROUP_ORDER_RADIX_FULL: "radix full", native.GROUP_ORDER_RADIX_SELECT: "radix select"}

rng = np.random.default_rng(8)
ctx = native.Context(0)
ids = rng.permutation(N).astype(np.int32)
age = rng.integers(-128, 128, size=N).astype(np.int8)
states = np.array([list(b"%c%c" % (65 + i // 26, 65 + i % 26)) for i in range(51)], np.uint8)[rng.integers(0, 51, size=N)]
k2048 = rng.integers(0, 2048, size=N).astype(np.int32)
seg = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids.view(np.uint8), N * 4, synth.block_offsets(N, 4)),
                                 (native.DENSE_STRING, 2, states.reshape(-1), N * 2, synth.block_offsets(N, 2)),
                                 (native.DENSE_TINYINT, 1, age.view(np.uint8), N, synth.block_offsets(N, 1)),
                                 (native.DENSE_INT, 4, k2048.view(np.uint8), N * 4, synth.block_offsets(N, 4))])
ctx.timing_enable(4 * ROUNDS)
ctx.timing_mask(1 << 8)


def settle_us(q, leaves, prog, order, limit):
    """(median device time of one settle's view launches in us, the path it took, groups kept)"""
    q.set_group_filter(leaves, prog)
    q.set_group_order(order, limit)
    q.fetch_groups()
    ctx.timing_reset()
    for _ in range(ROUNDS):
        q.set_group_filter(leaves, prog)
        q.fetch_groups()
    t = ctx.timing_collect(8) * 1e3
    return float(np.median(t)), PATHS[q.group_order_path()], q.group_filter_stats()[1]


lines = [f"# rows = {N}; view = device time of the launches of one filtered settle (kernel id 8), us, medians of {ROUNDS} settles; new = wall time of",
         f"# set_group_filter + set_group_order + fetch_groups, ms; old = wall time of fetch_groups of every group + numpy filter + np.lexsort + cut, ms; medians of {WALL}",
         f"{'statement':64s} {'groups':>8s} {'kept':>8s} {'path':>13s} {'view us':>9s} {'new ms':>8s} {'(min - max)':>15s} {'old ms':>8s} {'new/old':>8s}"]
order = [(A, 0, True)]
for what, group_col, n_groups in (("state", 1, 51), ("k", 3, 2048), ("id", 0, N)):
    q = native.DeviceQuery(ctx, seg, [0, 1, 2, 3], [], (), 0, 1024, group_cols=[group_col], aggs=[(C, 0), (S, 2)])
    q.run()
    keys, first, cnt, vals = q.fetch_groups()
    assert first.size == n_groups
    if n_groups == N:       # one-row groups: the sum is the row's age, uniform in -128 .. 127
        filters = [("sum > 125", (1, 0, native.GT, 125), vals[:, 1] > 125), ("sum > -1", (1, 0, native.GT, -1), vals[:, 1] > -1), ("sum > -129", (1, 0, native.GT, -129), vals[:, 1] > -129)]
    else:
        hi, mid = int(np.sort(cnt)[-max(1, n_groups // 100) - 1]), int(np.median(cnt))
        filters = [(f"count > {hi}", (0, 0, native.GT, hi), cnt > hi), (f"count > {mid}", (0, 0, native.GT, mid), cnt > mid), ("count > 0", (0, 0, native.GT, 0), cnt > 0)]
    for text, leaf, keep in filters:
        for ordered in (True, False):
            o, limit = (order, 10) if ordered else ([], 0)
            view, path, kept = settle_us(q, [leaf], [0], o, limit)
            assert kept == int(keep.sum())
            t_new, t_old = [], []
            for _ in range(WALL):
                q.set_group_filter([], [])
                q.set_group_order([], 0)
                ctx.sync()
                t0 = time.perf_counter()
                k_, f_, c_, v_ = q.fetch_groups()
                m = (v_[:, 1] if n_groups == N else c_.astype(np.int64)) > leaf[3]
                idx = np.flatnonzero(m)
                if ordered:
                    idx = idx[np.lexsort((f_[idx], -c_[idx].astype(np.int64)))[:10]]
                old = (k_[idx], f_[idx], c_[idx], v_[idx])
                t_old.append(time.perf_counter() - t0)
                ctx.sync()
                t0 = time.perf_counter()
                q.set_group_filter([leaf], [0])
                q.set_group_order(o, limit)
                got = q.fetch_groups()
                t_new.append(time.perf_counter() - t0)
                assert all(np.array_equal(x, y) for x, y in zip(got, old))
            new_ms, old_ms = float(np.median(t_new)) * 1e3, float(np.median(t_old)) * 1e3
            stmt = f"group by {what} having {text}" + (" order by id_count desc limit 10" if ordered else "")
            lines.append(f"{stmt:64s} {n_groups:8d} {kept:8d} {path:>13s} {view:9.1f} {new_ms:8.2f} {f'({min(t_new) * 1e3:.2f} - {max(t_new) * 1e3:.2f})':>15s} {old_ms:8.2f} {new_ms / old_ms:8.3f}")
    q.close()
text = "\n".join(lines) + "\n"
print(text, end="")
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
seg.close()
ctx.close()
