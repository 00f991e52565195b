#!/usr/bin/env python3
"""Development tool: the group merge by byte key (imm3_comm_merge_groups_wide) on one rank.
  * 8 queries x 100 000 groups: merge_groups_wide over 16-byte keys against merge_groups over 8-byte keys (the existing path, the
    yardstick) in the same process, and merge_groups_wide over the same 8-byte keys (the record path at the yardstick's key width);
  * 98 queries x 51 groups with a 16-byte key (the README-shaped table's `group by name`): merge_groups_wide against the host combine
    Engine.execute_agg does today -- every query's fetch_groups + fetch_group_keys, then a Python dict by key.
Wall time of the synchronous call (both ABI calls of the binding: the count, then the fetch), median of RUNS.  The group counts and
the sum of the counts are checked on the first run.  Output: profiles/merge_wide.txt.

    python tools/merge_wide_bench.py [out.txt]"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

out_path = sys.argv[1] if len(sys.argv) > 1 else None
RUNS = 10
C, MX = native.AGG_COUNT, native.AGG_MAX

ctx = native.Context(0)
comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
rng = np.random.default_rng(5)


def names_of(codes, w):
    """distinct codes -> distinct w-byte names: "n" and the code's base-26 digits"""
    out = np.full((codes.size, w), ord("a"), np.uint8)
    out[:, 0] = ord("n")
    c = codes.astype(np.int64)
    for b in range(w - 1, 0, -1):
        out[:, b] = (c % 26 + 97).astype(np.uint8)
        c //= 26
    return out


def segment(codes, w):
    n = codes.size
    cols = [(native.DENSE_INT, 4, np.arange(n, dtype=np.int32).view(np.uint8), n * 4, synth.block_offsets(n, 4)),
            (native.DENSE_TINYINT, 1, synth.uniform_below(2, n, 100, np.int8).view(np.uint8), n, synth.block_offsets(n, 1)),
            (native.DENSE_STRING, w, names_of(codes, w).reshape(-1), n * w, synth.block_offsets(n, w))]
    return native.DeviceSegment(ctx, cols)


def queries_over(code_lists, w):
    segs = [segment(c, w) for c in code_lists]
    qs = [native.DeviceQuery(ctx, s, [0, 1, 2], [], (), 0, 1024, group_cols=[2], aggs=[(C, 0), (MX, 1)], wide_keys=True) for s in segs]
    for q in qs:
        q.run()
        q.fetch_groups()           # (the dense group lists are settled: the merges time the merge)
    return segs, qs


def median_us(fn):
    fn()
    t = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t))


def host_combine(qs):
    table = {}
    for q in qs:
        _, first, counts, vals = q.fetch_groups()
        kb = q.fetch_group_keys()
        for g in range(kb.shape[0]):
            k = bytes(kb[g])
            cur = table.get(k)
            if cur is None:
                table[k] = [int(counts[g]), int(vals[g, 1])]
            else:
                cur[0] += int(counts[g])
                cur[1] = max(cur[1], int(vals[g, 1]))
    return table


lines = [f"one rank, count(id), max(age); wall time of the synchronous merge, median of {RUNS}, us"]

# ---- 8 queries x 100 000 groups: every row its own group, the segments' key ranges overlap by three quarters
code_lists = [np.arange(100_000, dtype=np.int64)[rng.permutation(100_000)] + s * 25_000 for s in range(8)]
distinct = 100_000 + 7 * 25_000
res = {}
for w in (8, 16):
    segs, qs = queries_over(code_lists, w)
    idx = list(range(8))
    if w == 8:
        keys, first, counts, vals = comm.merge_groups(qs, idx)
        assert keys.size == distinct and int(counts.sum()) == 800_000
        res["old8"] = median_us(lambda: comm.merge_groups(qs, idx))
    kb, first, counts, vals, _ = comm.merge_groups_wide(qs, idx)
    assert kb.shape == (distinct, w) and int(counts.sum()) == 800_000 and np.all(np.diff(first.astype(np.int64)) > 0)
    res[f"wide{w}"] = median_us(lambda: comm.merge_groups_wide(qs, idx))
    for q in qs:
        q.close()
    for s in segs:
        s.close()
lines += [f"8 queries x 100000 groups ({distinct} distinct)",
          f"  merge_groups,       8-byte keys (yardstick)   {res['old8']:10.1f}",
          f"  merge_groups_wide,  8-byte keys               {res['wide8']:10.1f}   x{res['wide8'] / res['old8']:.2f}",
          f"  merge_groups_wide, 16-byte keys               {res['wide16']:10.1f}   x{res['wide16'] / res['old8']:.2f}",
          f"  bytes per entry: 56 (list of the existing merge), 56 / 64 (records of 8- / 16-byte keys)"]

# ---- 98 queries x 51 groups, 16-byte key
code_lists = [rng.integers(0, 51, size=10_000).astype(np.int64) * 7919 for _ in range(98)]
for c in code_lists:
    c[:51] = np.arange(51) * 7919
segs, qs = queries_over(code_lists, 16)
idx = list(range(98))
kb, first, counts, vals, _ = comm.merge_groups_wide(qs, idx)
want = host_combine(qs)
assert kb.shape == (51, 16) and {bytes(k): [int(c), int(v[1])] for k, c, v in zip(kb, counts, vals)} == want
dev = median_us(lambda: comm.merge_groups_wide(qs, idx))
host = median_us(lambda: host_combine(qs))
lines += ["98 queries x 51 groups, 16-byte key",
          f"  merge_groups_wide                              {dev:10.1f}",
          f"  host combine (fetch per query + Python dict)    {host:10.1f}   x{host / dev:.2f} of the device merge"]
for q in qs:
    q.close()
for s in segs:
    s.close()

text = "\n".join(lines)
print(text, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
comm.close()
ctx.close()
