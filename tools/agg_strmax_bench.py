#!/usr/bin/env python3
"""Development tool: MAX over strings wider than 8 bytes (the prefix launch + refine passes) over 100 M rows, group by
state (51 keys): count(id), max(name) with name 16 and 32 bytes wide, on random ASCII (ties on the first 8 bytes rare) and on
"prefix-heavy" data (half the rows share their first 8 bytes, which are every group's maximum prefix), with and without
age > 18 and age < 30.  Next to each, count(id), max(state) in the same process.  Stage times by the library's event timing: the
aggregation launch (kernel id 4), each refine pass (kernel id 6); the collect as the host time of fetch_group_strings (launch, copy,
sort).  Every result is checked against numpy on the first run.  Output: profiles/agg_strmax.txt.

    python tools/agg_strmax_bench.py [rows] [out.txt]"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
RUNS = 10
C, MX = native.AGG_COUNT, native.AGG_MAX
FORM = {0: "lanes", 1: "lanes-127", 2: "direct", 3: "tile", 4: "general"}

ctx = native.Context(0)
rng = np.random.default_rng(7)
ids = np.arange(n, dtype=np.int32)
age = synth.uniform_below(2, n, 100, np.int8)
st = synth.state_codes(3, n)
key = st[:, 0].astype(np.int64) | (st[:, 1].astype(np.int64) << 8)
RANGE = [(2, native.GT, 18.0), (2, native.LT, 30.0)]


def names_of(w, heavy, n):
    v = rng.integers(97, 123, size=(n, w), dtype=np.uint8)
    if heavy:
        v[::2, :8] = ord("z")
    return v


def np_max(names, mask, key):
    """per state: the byte-lexicographic max of the selected names (first 8 bytes, then the rest among the ties)"""
    out = {}
    sel = np.flatnonzero(mask)
    order = np.argsort(key[sel], kind="stable")
    sel = sel[order]
    ks = key[sel]
    for rows in np.split(sel, np.flatnonzero(np.diff(ks)) + 1):
        alive = rows
        for c in range(0, names.shape[1], 8):
            v = np.zeros(alive.size, np.uint64)
            for b in range(c, min(c + 8, names.shape[1])):
                v = (v << np.uint64(8)) | names[alive, b].astype(np.uint64)
            alive = alive[v == v.max()]
        out[int(key[rows[0]])] = bytes(names[alive[0]])
    return out


def timed(q, wide):
    ctx.timing_enable(RUNS * 8 + 8)
    ctx.timing_mask((1 << 4) | (1 << 6))
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(RUNS):
        q.run()
    ctx.sync()
    wall = (time.perf_counter() - t0) / RUNS * 1e6
    agg = float(np.median(ctx.timing_collect(4))) * 1e3
    ref = np.array(ctx.timing_collect(6), np.float64) * 1e3 if wide else np.zeros(0)
    ctx.timing_enable(0)
    collect = 0.0
    if wide:
        t0 = time.perf_counter()
        for _ in range(3):
            q.fetch_group_strings(1)
        collect = (time.perf_counter() - t0) / 3 * 1e6
    return agg, ref, wall, collect


lines = [f"group by state over {n} rows (51 keys); event timing, median of {RUNS} runs, us.  refine: per pass; collect: host time of",
         "fetch_group_strings (k_group_collect has run already: the strings' launch, the copy and the sort); wall: whole run() incl. select",
         f"{'query':58s} {'form':>8s} {'agg':>8s} {'refine passes':>22s} {'collect':>8s} {'wall':>8s} {'vs max(state)':>14s}"]
for w in (16, 32):
    # (a segment's block offsets are int32: a column holds < 2^31 bytes, so a 32-byte column has at most 64 M rows per segment)
    m = min(n, (2 ** 31 - 1) // w // 1024 * 1024)
    for heavy in (False, True):
        names = names_of(w, heavy, m)
        seg = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids[:m].view(np.uint8), m * 4, synth.block_offsets(m, 4)),
                                         (native.DENSE_STRING, 2, st[:m].reshape(-1), m * 2, synth.block_offsets(m, 2)),
                                         (native.DENSE_TINYINT, 1, age[:m].view(np.uint8), m, synth.block_offsets(m, 1)),
                                         (native.DENSE_STRING, w, names.reshape(-1), m * w, synth.block_offsets(m, w))])
        for sels, where in (([], ""), (RANGE, " where age > 18 and age < 30")):
            base = native.DeviceQuery(ctx, seg, [0, 1, 2, 3], sels, (), 0, 1024, group_cols=[1], aggs=[(C, 0), (MX, 1)])
            q = native.DeviceQuery(ctx, seg, [0, 1, 2, 3], sels, (), 0, 1024, group_cols=[1], aggs=[(C, 0), (MX, 3)])
            for x in (base, q):
                for _ in range(3):
                    x.run()
            keys, _, _, _ = q.fetch_groups()
            got = q.fetch_group_strings(1)
            want = np_max(names, np.ones(m, bool) if not sels else (age[:m] > 18) & (age[:m] < 30), key[:m])
            assert {int(k): bytes(g) for k, g in zip(keys, got)} == want, (w, heavy, where)
            b_agg, _, b_wall, _ = timed(base, False)
            agg, ref, wall, collect = timed(q, True)
            per_pass = ref.reshape(RUNS, -1) if ref.size else ref.reshape(RUNS, 0)
            passes = ", ".join(f"{v:.1f}" for v in np.median(per_pass, axis=0))
            data = ("prefix-heavy" if heavy else "random") + ("" if m == n else f", {m / 1e6:.0f} M rows")
            lines.append(f"{'count(id), max(state)' + where + ('' if m == n else f' [{m / 1e6:.0f} M rows]'):58s} {FORM.get(base.agg_form(), '?'):>8s} {b_agg:8.1f} {'':>22s} {'':>8s} {b_wall:8.1f}")
            lines.append(f"{f'count(id), max(name{w}) [{data}]' + where:58s} {FORM.get(q.agg_form(), '?'):>8s} {agg:8.1f} {passes:>22s} "
                         f"{collect:8.1f} {wall:8.1f} {wall / b_wall:13.2f}x")
            print(lines[-2], "\n" + lines[-1], flush=True)
            base.close()
            q.close()
        seg.close()
        del names
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
ctx.close()
