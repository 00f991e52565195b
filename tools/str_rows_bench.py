#!/usr/bin/env python3
"""Development tool: Match on string columns, k_filter_str_rows against the word-at-a-time kernel (tuning variant 1: the same query,
the same build, interleaved), HIP-event kernel times.  Rows S4 / S8 / S16 / S64 take the string kernel, S5 only the generic one.
Three copies of every column rotate so that no run finds its column in the 256 MB Infinity Cache.  Then a README-shaped table
(98 segments of 1000 blocks of 1024 rows + the loader's 1-row block) with a 16-byte name column: `select id where name = ...` as one
table query against 98 per-segment queries.  Usage: str_rows_bench.py [kernel] [table]   (default: both)."""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth  # noqa: E402

MATCH = native.MATCH
DENSE_INT, DENSE_STRING = 1, 3
what = sys.argv[1:] or ["kernel", "table"]
ctx = native.Context(0)


def strings(seed, n, width, pool_size=64):
    rng = np.random.default_rng(seed)
    pool = rng.integers(97, 123, size=(pool_size, width)).astype(np.uint8)
    return pool, pool[rng.integers(0, pool_size, size=n, dtype=np.int32)]


def kernel_ms(queries, variant, reps):
    """median kernel time of the select launch, the queries (one per column copy) taking turns"""
    ctx.set_tuning(variant, 0)
    for q in queries:
        q.run_select()
    ctx.sync()
    ctx.timing_enable(4 * reps * len(queries))
    ctx.timing_mask(1)
    ctx.timing_reset()
    for _ in range(reps):
        for q in queries:
            q.run_select()
    ctx.sync()
    ms = float(np.median(ctx.timing_collect(0)))
    ctx.timing_enable(0)
    ctx.set_tuning(0, 0)
    return ms


if "kernel" in what:
    print(f"{'kind':6s} {'rows':>10s} {'str_rows us':>12s} {'% of 8 TB/s':>12s} {'generic us':>11s} {'% of 8 TB/s':>12s} {'speed-up':>9s}")
    for width, n in ((4, 100_000_000), (8, 100_000_000), (16, 100_000_000), (64, 25_000_000), (5, 100_000_000)):
        pool, v = strings(width, n, width)
        offs = synth.block_offsets(n, width)
        seg = native.DeviceSegment(ctx, [(DENSE_STRING, width, v.reshape(-1), n * width, offs)] * 3)
        sels = [(0, MATCH, [bytes(pool[0])])]
        ctx.set_tuning(0, 0)
        new_q = [native.DeviceQuery(ctx, seg, [c], sels) for c in range(3)]
        ctx.set_tuning(1, 0)
        old_q = [native.DeviceQuery(ctx, seg, [c], sels) for c in range(3)]
        ctx.set_tuning(0, 0)
        new_ms, old_ms = [], []
        for _ in range(3):  # interleaved
            new_ms.append(kernel_ms(new_q, 0, 5))
            old_ms.append(kernel_ms(old_q, 1, 3))
        for q in new_q:
            q.run_select()
        counts = {q.count() for q in new_q} | {q.count() for q in old_q}
        assert len(counts) == 1, counts
        a, b = float(np.median(new_ms)), float(np.median(old_ms))
        frac = lambda ms: (width + 0.125) * n / (ms * 1e-3) / 8e12 * 100
        if native.plan_string_route(width, 1) == 1:
            print(f"S{width:<5d} {n:10d} {a * 1e3:12.1f} {frac(a):11.1f}% {b * 1e3:11.1f} {frac(b):11.1f}% {b / a:8.2f}x")
        else:  # (the default plan IS the generic kernel)
            print(f"S{width:<5d} {n:10d} {'-':>12s} {'-':>12s} {b * 1e3:11.1f} {frac(b):11.1f}% {'(generic)':>9s}")
        for q in new_q + old_q:
            q.close()
        seg.close()
        del v

if "table" in what:
    n_seg, n = 98, 1000 * 1024 + 1
    block_rows = [1024] * 1000 + [1]
    pool, names = strings(99, n, 16)
    ids = np.arange(n, dtype=np.int32)
    offs4 = np.concatenate([[0], np.cumsum(np.array(block_rows, np.int64) * 4)]).astype(np.int32)
    offs16 = np.concatenate([[0], np.cumsum(np.array(block_rows, np.int64) * 16)]).astype(np.int32)
    segs = [native.DeviceSegment(ctx, [(DENSE_INT, 4, ids.view(np.uint8), n * 4, offs4), (DENSE_STRING, 16, names.reshape(-1), n * 16, offs16)])
            for _ in range(n_seg)]
    table = native.DeviceTable(ctx, segs)
    sels = [(1, MATCH, [bytes(pool[0])])]

    def wall_us(queries, reps=5):
        for q in queries:
            q.run()
        ctx.sync()
        best = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for q in queries:
                q.run()
            ctx.sync()
            best.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(best))

    tq = native.DeviceQuery(ctx, table, [0, 1], sels, [0], 0, 1024)
    t_table = wall_us([tq])
    rows = tq.row_count()
    per = [native.DeviceQuery(ctx, s, [0, 1], sels, [0], 0, 1024) for s in segs]
    t_per = wall_us(per)
    assert sum(q.row_count() for q in per) == rows
    ctx.set_tuning(1, 0)
    old = [native.DeviceQuery(ctx, s, [0, 1], sels, [0], 0, 1024) for s in segs]
    t_old = wall_us(old)
    ctx.set_tuning(0, 0)
    assert sum(q.row_count() for q in old) == rows
    print(f"table of {n_seg} segments x {n} rows, select id where name = <16 bytes> ({rows} rows), enqueue to completion:")
    print(f"  one table query                                  {t_table:9.1f} us")
    print(f"  {n_seg} per-segment queries, k_filter_str_rows        {t_per:9.1f} us")
    print(f"  {n_seg} per-segment queries, k_filter_generic (before) {t_old:9.1f} us   ({t_old / t_table:.1f}x the table query)")
ctx.close()
