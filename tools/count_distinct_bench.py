#!/usr/bin/env python3
"""Development tool: COUNT(DISTINCT) in the group-by aggregation (IMM3_AGG_COUNT_DISTINCT) over 100 M rows of the README schema (id
int32 = the row number, state 2 bytes / 51 codes, age int8 / 100 values), group by state:

    count(distinct age)   the small pair set: 51 x 100 pairs, almost every row meets its own entry
    count(distinct id)    the worst one: every row is a pair of its own, the set is as large as it gets (2^28 entries)

per run the clear of the set (event timing, kernel id 11), the select launch (0), the aggregation launch (4) and the mark pass (10),
then the whole statement on the wall clock: run + fetch of the 51 groups.  Every figure is checked against numpy.

--baseline measures the only way to the same figures WITHOUT the aggregate -- group by (state, age), respectively (state, id), fetch
every group, count on the host -- and is meant for a build of the commit before the aggregate existed (IMM3_LIB_PATH names its
library); both modes also time a plain count(id), max(age) group by state, to show that the general path was not slowed, and
--plain times that statement alone (alternate it between the two libraries: one process each, several times over).
Output: profiles/count_distinct.txt (every mode appends to the file it is given).

    python tools/count_distinct_bench.py [--baseline | --plain] [rows] [out.txt]"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

args = [a for a in sys.argv[1:] if a not in ("--baseline", "--plain")]
baseline, plain_only = "--baseline" in sys.argv[1:], "--plain" in sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 100_000_000
out_path = args[1] if len(args) > 1 else None
RUNS, ROUNDS = 10, 5
FORM = {0: "lanes", 1: "lanes-127", 2: "direct", 3: "tile", 4: "general"}
C, MX = native.AGG_COUNT, native.AGG_MAX
K_SELECT, K_AGG, K_MARK, K_CLEAR = 0, 4, native.KERNEL_DISTINCT_MARK, native.KERNEL_DISTINCT_CLEAR

ctx = native.Context(0)
ids = np.arange(n, dtype=np.int32)
age = synth.uniform_below(2, n, 100, np.int8)
st = synth.state_codes(3, n)
seg = native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids.view(np.uint8), n * 4, synth.block_offsets(n, 4)),
                                 (native.DENSE_STRING, 2, st.reshape(-1), n * 2, synth.block_offsets(n, 2)),
                                 (native.DENSE_TINYINT, 1, age.view(np.uint8), n, synth.block_offsets(n, 1))])
USED, ID, STATE, AGE = [0, 1, 2], 0, 1, 2
key = st[:, 0].astype(np.int64) | (st[:, 1].astype(np.int64) << 8)
rows_per_state = np.bincount(key, minlength=1 << 16)
present = np.bincount(key * 128 + age.astype(np.int64), minlength=(1 << 16) * 128).reshape(1 << 16, 128) > 0
WANT = {"age": present.sum(axis=1), "id": rows_per_state}       # (id is the row number: every row of a state is a value of its own)
del present
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def spread(xs):
    return f"{np.median(xs):10.1f} [{min(xs):.1f}, {max(xs):.1f}]"


def kernel_times(q, kernels):
    """{kernel id: [round medians, us]} of q.run() by event timing, each round the median of RUNS runs (a kernel that ran twice in
    one run -- two aggregates -- counts both)"""
    per = {k: [] for k in kernels}
    for _ in range(ROUNDS):
        ctx.timing_enable(8 * RUNS + 8)
        ctx.timing_mask(sum(1 << k for k in kernels))
        ctx.timing_reset()
        for _ in range(RUNS):
            q.run()
        ctx.sync()
        for k in kernels:
            t = ctx.timing_collect(k)
            per[k].append(float(np.median(t)) * 1e3 if t.size else 0.0)
        ctx.timing_enable(0)
    return per


def wall(fn, reps):
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def plain_count_max():
    q = native.DeviceQuery(ctx, seg, USED, [], (), 0, 1024, group_cols=[STATE], aggs=[(C, ID), (MX, AGE)])
    for _ in range(3):
        q.run()
    keys, first, counts, vals = q.fetch_groups()
    assert counts.tolist() == rows_per_state[keys.astype(np.int64)].tolist()
    per = kernel_times(q, [K_AGG])
    say(f"count(id), max(age) group by state: form {FORM.get(q.agg_form(), '?')}; aggregation launch, median [min, max] of {ROUNDS} round medians, us: {spread(per[K_AGG])}")
    q.close()


if not plain_only:
    say(f"==== {'BASELINE (two-column group-by, fetch, count on the host)' if baseline else 'count(distinct) as one query'}: {n} rows, 51 states ====")
plain_count_max()
for col, cidx, reps in (() if plain_only else (("age", AGE, 5), ("id", ID, 2 if baseline else 5))):
    if baseline:
        q = native.DeviceQuery(ctx, seg, USED, [], (), 0, 1024, group_cols=[STATE, cidx], aggs=[(C, ID)])

        def statement():
            q.run()
            keys, first, counts, vals = q.fetch_groups()           # every (state, value) group comes to the host ...
            statement.figure = np.bincount((keys & np.uint64(0xFFFF)).astype(np.int64), minlength=1 << 16)   # ... which counts them per state
        statement()
        assert statement.figure.tolist() == WANT[col].tolist()
        ms = wall(statement, reps)
        say(f"group by state, {col} + fetch + host count: form {FORM.get(q.agg_form(), '?')}; whole statement, ms, median [min, max] of {reps}: {spread(ms)}")
        q.close()
        continue
    CD = native.AGG_COUNT_DISTINCT
    q = native.DeviceQuery(ctx, seg, USED, [], (), 0, 1024, group_cols=[STATE], aggs=[(CD, cidx), (C, ID)])

    def statement():
        q.run()
        statement.groups = q.fetch_groups()
    statement()
    keys, first, counts, vals = statement.groups
    assert vals[:, 0].tolist() == WANT[col][keys.astype(np.int64)].tolist() and counts.tolist() == rows_per_state[keys.astype(np.int64)].tolist()
    entries = native.plan_distinct_capacity(n, 2, 1 if col == "age" else 4)
    per = kernel_times(q, [K_CLEAR, K_SELECT, K_AGG, K_MARK])
    ms = wall(statement, reps)
    say(f"count(distinct {col}), count(id) group by state: form {FORM.get(q.agg_form(), '?')}, pair set {entries} entries ({entries * 8 / 2 ** 20:.0f} MiB)")
    for k, name in ((K_CLEAR, "clear of the set"), (K_SELECT, "select launch"), (K_AGG, "aggregation launch"), (K_MARK, "mark pass")):
        say(f"    {name:20s} us, median [min, max] of {ROUNDS} round medians: {spread(per[k])}")
    say(f"    {'whole statement':20s} ms, run + fetch, median [min, max] of {reps}: {spread(ms)}")
    statement()
    assert statement.groups[3][:, 0].tolist() == WANT[col][statement.groups[0].astype(np.int64)].tolist()     # (after the timed runs too)
    q.close()
if out_path:
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
seg.close()
ctx.close()
