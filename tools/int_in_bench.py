#!/usr/bin/env python3
"""Development tool: what an integer IN-list costs.  Over `rows` rows (default 100 M), kernel time of the select launch by the
library's event timing (kernel id 0):
  (a) the list pass (k_filter_int_list): on an int32 column random ids with 1, 8, 9, 1 k, 64 k and 1 M values, over a SORTED and a
      SHUFFLED column; on an int8 column 4 and 64 values;
  (b) one conjunctive range over the same column through k_filter_tile, which reads the same bytes -- the floor;
  (c) the OR tree of IMM3_EQ leaves for 2 / 4 / 8 values (k_filter_expr): what a list cost before the pass existed.
All queries of one column are alternated round by round in one process; medians.  Every list's count is checked against numpy.

    python tools/int_in_bench.py [rows] [out.txt]"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import native, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS = 11
FORMS = {native.INT_LIST_I8: "I8", native.INT_LIST_ARGS: "ARGS", native.INT_LIST_LDS: "LDS", native.INT_LIST_GLOBAL: "GLOBAL"}

ctx = native.Context(0)
rng = np.random.default_rng(7)
lines = [f"# rows = {n}; kernel time of the select launch (us), median of {ROUNDS} alternated rounds; a/b: against the one-compare range over the same column"]


def measure(queries):
    for q in queries:
        q.run_select()
        q.sync()
    ctx.timing_enable(ROUNDS * len(queries) + 8)
    ctx.timing_mask(1)
    ctx.timing_reset()
    for _ in range(ROUNDS):
        for q in queries:
            q.run_select()
    ctx.sync()
    us = ctx.timing_collect(0).reshape(ROUNDS, len(queries)) * 1e3
    ctx.timing_enable(0)
    return [float(np.median(us[:, k])) for k in range(len(queries))]


CHECK = 1 << 20


def draw(domain, k):
    """k distinct values of the domain (an int: 0 .. domain - 1), without a permutation of the whole domain"""
    if not isinstance(domain, int):
        return [int(v) for v in rng.choice(domain, size=k, replace=False)]
    got = np.unique(rng.integers(0, domain, size=k + k // 8 + 8))
    return [int(v) for v in rng.permutation(got)[:k]]


def column(name, values, codec, width, sizes, domain):
    seg = native.DeviceSegment(ctx, [(codec, width, values.view(np.uint8), n * width, synth.block_offsets(n, width))])
    mid = int(np.median(values[:1_000_000]))
    names, queries, wants = ["(b) range"], [native.DeviceQuery(ctx, seg, [0], [(0, native.GT, float(mid))])], [int((values > mid).sum())]
    lists = {}
    for k in sizes:
        lists[k] = draw(domain, k)
        names.append(f"(a) list {k} [{FORMS[native.plan_int_list_form(width, k)]}]")
        queries.append(native.DeviceQuery(ctx, seg, [0], [(0, native.INT_IN, lists[k])]))
        wants.append(lists[k])
    if width == 4:
        for t in (2, 4, 8):
            prog = [0] + [x for i in range(1, t) for x in (i, native.EXPR_OR)]
            names.append(f"(c) OR of {t} EQ")
            queries.append(native.DeviceQuery(ctx, seg, [0], [(0, native.EQ, float(v)) for v in lists[8][:t]], expr=prog))
            wants.append(lists[8][:t])
    us = measure(queries)
    for q, w, nm in zip(queries, wants, names):   # short lists: the count over every row; long ones: the bitmap of the first CHECK rows
        if isinstance(w, int) or len(w) <= 9:
            assert q.count() == (w if isinstance(w, int) else int(np.isin(values, np.array(w, dtype=values.dtype)).sum())), (name, nm)
        else:
            m = np.isin(values[:CHECK], np.array(w, dtype=values.dtype))
            assert q.bitmap()[:CHECK // 64].tolist() == np.packbits(m, bitorder="little").view("<u8").tolist(), (name, nm)
    lines.append(f"## {name}")
    for nm, t in zip(names, us):
        lines.append(f"{nm:28s} {t:9.1f} us   a/b {t / us[0]:5.2f}")
        print(lines[-1], flush=True)
    if width == 4:
        by = dict(zip(names, us))
        lines.append("a/c: 8-value list / OR of 8 EQ = %.2f" % (by[f"(a) list 8 [{FORMS[native.plan_int_list_form(4, 8)]}]"] / by["(c) OR of 8 EQ"]))
    for q in queries:
        q.close()
    seg.close()


SIZES32 = (1, 8, 9, 1_000, 64_000, 1_000_000)
ids = rng.integers(0, 1 << 30, size=n, dtype=np.int32)
column("int32, shuffled", ids, native.DENSE_INT, 4, SIZES32, 1 << 30)
ids.sort()
column("int32, sorted", ids, native.DENSE_INT, 4, SIZES32, 1 << 30)
del ids
age = rng.integers(-128, 128, size=n).astype(np.int8)
column("int8", age, native.DENSE_TINYINT, 1, (4, 64), np.arange(-128, 128))
text = "\n".join(lines) + "\n"
print(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text)
