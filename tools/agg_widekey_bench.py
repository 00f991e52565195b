#!/usr/bin/env python3
"""Development tool: group-by on keys wider than 8 bytes (the tag tables of the general kernel's wide-key instance)
over 100 M rows, count(id), max(age):
  * group by a 16-byte name of 51 distinct values, all rows and behind age > 18 and age < 30;
  * group by a 16-byte name of 1 M and of 50 M distinct values (every one of them selected at least once or so);
  * group by three int32 columns (a 12-byte key, 8 x 8 x 8 values).
Next to them, count(id), max(age) group by state (51 two-byte keys: the narrow path) in the same process.  Stage times by the
library's event timing: the aggregation launch (kernel id 4); collect: host time of fetch_groups + fetch_group_keys (k_group_collect,
the key gather, copies, sort); wall: the whole run() including the select.  Every result's groups and counts are checked against
numpy on the first run.  Output: profiles/agg_widekey.txt.

    python tools/agg_widekey_bench.py [rows] [out.txt]"""
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
RANGE = [(2, native.GT, 18.0), (2, native.LT, 30.0)]


def names_of(codes, w=16):
    """distinct codes -> distinct w-byte names: "n" and the code's base-26 digits (a shared leading run of 'a's)"""
    out = np.full((codes.size, w), ord("a"), np.uint8)
    out[:, 0] = ord("n")
    c = codes.astype(np.int64)
    for b in range(w - 1, 0, -1):
        out[:, b] = (c % 26 + 97).astype(np.uint8)
        c //= 26
    return out


def col(codec, w, arr):
    return (codec, w, np.ascontiguousarray(arr).reshape(-1).view(np.uint8), n * w, synth.block_offsets(n, w))


def timed(q):
    ctx.timing_enable(RUNS * 4 + 8)
    ctx.timing_mask(1 << 4)
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(RUNS):
        q.run()
    ctx.sync()
    wall = (time.perf_counter() - t0) / RUNS * 1e6
    agg = float(np.median(ctx.timing_collect(4))) * 1e3
    ctx.timing_enable(0)
    t0 = time.perf_counter()
    for _ in range(3):
        q.fetch_groups()
        q.fetch_group_keys()
    collect = (time.perf_counter() - t0) / 3 * 1e6
    return agg, wall, collect


def check(q, key_of_row_code, n_codes, mask):
    """the groups and their counts against numpy: key_of_row_code(code) -> key bytes; codes per selected row via bincount"""
    keys, first, counts, _ = q.fetch_groups()
    kb = q.fetch_group_keys()
    want = np.bincount(row_codes[mask] if mask is not None else row_codes, minlength=n_codes)
    present = np.flatnonzero(want)
    assert kb.shape[0] == present.size, (kb.shape, present.size)
    assert int(counts.sum()) == int(want.sum())
    assert np.all(np.diff(first.astype(np.int64)) > 0)
    code_at_first = row_codes[first]
    assert np.array_equal(kb, key_of_row_code(code_at_first))
    assert np.array_equal(counts, want[code_at_first].astype(counts.dtype))


lines = [f"count(id), max(age) over {n} rows; event timing, median of {RUNS} runs, us.  agg: the aggregation launch; collect: host time of",
         "fetch_groups + fetch_group_keys (collect launch, key gather, copies, sort); wall: whole run() incl. the select",
         f"{'query':64s} {'form':>8s} {'groups':>10s} {'agg':>9s} {'collect':>10s} {'wall':>9s}"]


def report(label, q, groups):
    agg, wall, collect = timed(q)
    lines.append(f"{label:64s} {FORM.get(q.agg_form(), '?'):>8s} {groups:10d} {agg:9.1f} {collect:10.1f} {wall:9.1f}")
    print(lines[-1], flush=True)


base_cols = [col(native.DENSE_INT, 4, ids), col(native.DENSE_STRING, 2, st), col(native.DENSE_TINYINT, 1, age)]
mask_range = (age > 18) & (age < 30)

# narrow reference: group by state
seg = native.DeviceSegment(ctx, base_cols)
for sels, where in (([], ""), (RANGE, " where age > 18 and age < 30")):
    q = native.DeviceQuery(ctx, seg, [0, 1, 2], sels, (), 0, 1024, group_cols=[1], aggs=[(C, 0), (MX, 2)])
    for _ in range(3):
        q.run()
    report("group by state (2 bytes, 51 keys)" + where, q, q.fetch_groups()[0].size)
    q.close()
seg.close()

# 16-byte names: 51, 1 M, 50 M distinct values
for k in (51, 1_000_000, 50_000_000):
    pool = names_of(np.arange(k, dtype=np.int64) * 7919)
    row_codes = rng.integers(0, k, size=n)
    names = pool[row_codes]
    seg = native.DeviceSegment(ctx, base_cols + [col(native.DENSE_STRING, 16, names)])
    for sels, where, mask in (([], "", None), (RANGE, " where age > 18 and age < 30", mask_range)):
        if k > 51 and sels:
            continue
        q = native.DeviceQuery(ctx, seg, [0, 1, 2, 3], sels, (), 0, 1024, group_cols=[3], aggs=[(C, 0), (MX, 2)], wide_keys=True)
        for _ in range(3):
            q.run()
        check(q, lambda c: pool[c], k, mask)
        report(f"group by name (16 bytes, {k} distinct)" + where, q, q.fetch_groups()[0].size)
        q.close()
    seg.close()
    del pool, names

# 12 bytes: three int32 columns
parts = [rng.integers(0, 8, size=n).astype(np.int32) for _ in range(3)]
row_codes = parts[0].astype(np.int64) * 64 + parts[1] * 8 + parts[2]
seg = native.DeviceSegment(ctx, base_cols + [col(native.DENSE_INT, 4, p) for p in parts])
q = native.DeviceQuery(ctx, seg, [0, 1, 2, 3, 4, 5], [], (), 0, 1024, group_cols=[3, 4, 5], aggs=[(C, 0), (MX, 2)], wide_keys=True)
for _ in range(3):
    q.run()
check(q, lambda c: np.stack([(c // 64).astype(np.int32), (c // 8 % 8).astype(np.int32), (c % 8).astype(np.int32)], 1).view(np.uint8), 512, None)
report("group by a, b, c (three int32 columns: 12 bytes, 512 keys)", q, q.fetch_groups()[0].size)
q.close()
seg.close()

text = "\n".join(lines)
print(text, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
ctx.close()
