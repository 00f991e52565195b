#!/usr/bin/env python3
"""Development tool: byte-order ranges on string columns (IMM3_STR_RANGE), k_filter_str_range against Match of two values on the same
column (k_filter_str_rows) and against the word-at-a-time kernel's range form (tuning variant 1: the same query, the same build),
all interleaved, HIP-event kernel times.  Columns S4 / S8 / S16 at 100 M rows, S64 at 25 M, uniformly random bytes; per width a wide
range (3/4 of the rows), a prefix (one row in 256) and a range whose lower bound ties with a tenth of the rows' first min(width, 16)
bytes -- on S64 those rows are decided in the tail loop.  Three copies of every column rotate so that no run finds its column in the
256 MB Infinity Cache.  Usage: str_range_bench.py > profiles/str_range.txt"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth  # noqa: E402

MATCH, STR_RANGE = native.MATCH, native.STR_RANGE
DENSE_STRING = 3
ctx = native.Context(0)


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


print("# tools/str_range_bench.py on one MI355X (HIP-event kernel times, median; Match of two values and the generic kernel's range form,")
print("# tuning variant 1, are the same column and build, interleaved with the range)")
print(f"{'kind':5s} {'rows':>10s} {'range':>7s} {'selected':>10s} {'str_range us':>13s} {'% of 8 TB/s':>12s} {'match2 us':>10s} {'range/match2':>13s} {'generic us':>11s} {'generic/range':>14s}")
for width, n in ((4, 100_000_000), (8, 100_000_000), (16, 100_000_000), (64, 25_000_000)):
    rng = np.random.default_rng(width)
    v = rng.integers(0, 256, size=(n, width), dtype=np.uint8)
    p = min(width, 16)
    tie = bytes(rng.integers(0x30, 0x70, size=width).astype(np.uint8))
    v[::10, :p] = np.frombuffer(tie[:p], dtype=np.uint8)
    offs = synth.block_offsets(n, width)
    seg = native.DeviceSegment(ctx, [(DENSE_STRING, width, v.reshape(-1), n * width, offs)] * 3)
    match2 = (0, MATCH, [bytes(v[1]), bytes(v[2])])
    ranges = [("wide", (b"\x20", b"\xdf")), ("prefix", (b"\x41", b"\x41")), ("tie", (tie, b"\xdf"))]
    ctx.set_tuning(0, 0)
    match_q = [native.DeviceQuery(ctx, seg, [c], [match2]) for c in range(3)]
    for name, bounds in ranges:
        sels = [(0, STR_RANGE, bounds)]
        ctx.set_tuning(0, 0)
        new_q = [native.DeviceQuery(ctx, seg, [c], sels) for c in range(3)]
        ctx.set_tuning(1, 0)
        old_q = [native.DeviceQuery(ctx, seg, [c], sels) for c in range(3)]
        ctx.set_tuning(0, 0)
        new_ms, match_ms, old_ms = [], [], []
        for _ in range(3):  # interleaved
            new_ms.append(kernel_ms(new_q, 0, 5))
            match_ms.append(kernel_ms(match_q, 0, 5))
            old_ms.append(kernel_ms(old_q, 1, 2))
        for q in new_q:
            q.run_select()
        counts = {q.count() for q in new_q} | {q.count() for q in old_q}
        assert len(counts) == 1, counts
        a, m, b = float(np.median(new_ms)), float(np.median(match_ms)), float(np.median(old_ms))
        frac = (width + 0.125) * n / (a * 1e-3) / 8e12 * 100
        print(f"S{width:<4d} {n:10d} {name:>7s} {counts.pop():10d} {a * 1e3:13.1f} {frac:11.1f}% {m * 1e3:10.1f} {a / m:13.3f} {b * 1e3:11.1f} {b / a:13.2f}x")
        for q in new_q + old_q:
            q.close()
    for q in match_q:
        q.close()
    seg.close()
    del v
ctx.close()
