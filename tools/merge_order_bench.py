#!/usr/bin/env python3
"""Development tool: the merge of ordered results (imm3_comm_merge_ordered, DESIGN.md §21 "Merging ordered results") on one rank
against the host merge (operators.merge_ordered), eight segments of 1 M rows on one GPU, `select id, age order by id desc` with
`limit 1000` and without a limit.
  * the merge alone: the eight per-segment ordered queries have run and are settled; Comm.merge_ordered (pack, rank kernel, copy to the
    host, unpack) against operators.merge_ordered on the per-segment results -- on arrays already fetched, and with their fetch
    (what the host path has to do before it can merge);
  * the whole statement through the Python Engine, device_merge=True against device_merge=False (the yardstick): with the limit,
    list(Engine.execute(q)); without it the same up to the merged columns (boxing 8 M rows into Row objects is the same on both sides
    and would hide the merge).
Wall time of the synchronous calls, medians of ROUNDS interleaved rounds (device, host, device, host ...) after one warm-up round.
The two sides' rows are compared on the warm-up round.  Output: profiles/merge_ordered.txt.

    python tools/merge_order_bench.py [out.txt]"""
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from immutable3_amd import Project, Query, native  # noqa: E402
from immutable3_amd.operators import Engine, GpuSegmentManager, merge_ordered  # noqa: E402
from immutable3_amd.query import NoSelect, order_keys  # noqa: E402
from immutable3_amd.schema import CodecType, Column, Table, TableIO  # noqa: E402
from immutable3_amd.storage import SegmentManager, write_segment_arrays  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
ROUNDS, SEGS, ROWS = 7, 8, 1 << 20
ORDER = [("id", True)]

d = tempfile.mkdtemp(prefix="imm3_merge_order_")
t = Table("mo", [Column.make("id", CodecType.DENSE_INT), Column.make("age", CodecType.DENSE_TINYINT)], 1000)   # (blocks of 1000 rows: no one-table query)
TableIO.store(d, t)
rng = np.random.default_rng(11)
for s in range(SEGS):
    write_segment_arrays(d, t, s, {"id": rng.integers(-2 ** 31, 2 ** 31, size=ROWS, dtype=np.int64).astype(np.int32),
                                   "age": rng.integers(0, 100, size=ROWS).astype(np.int8)})
gsm = GpuSegmentManager(SegmentManager(d))
assert gsm.device_table("mo") is None


def interleaved(fns):
    """{name: median ms} of ROUNDS rounds that run every fn once, in turn, after one warm-up round"""
    for fn in fns.values():
        fn()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: float(np.median(v)) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


lines = [f"one rank, {SEGS} segments x {ROWS} rows, select id, age order by id desc; wall time, median of {ROUNDS} interleaved rounds (min .. max), ms"]
for limit in (1000, 0):
    q = Query("mo", NoSelect, Project(["id", "age"], limit, ORDER))
    okeys = order_keys(q.project.cols, q.project.order_by)
    dev_eng, host_eng = Engine(gsm, device_merge=True), Engine(gsm)
    # ---- the merge alone: the queries stay open and settled
    pipes = list(host_eng.pipelines(q))
    qs = [proj._open() for _, proj in pipes]
    idx = [s for s, _ in pipes]
    rows_in = sum(x.row_count() for x in qs)
    comm = native.Comm(gsm.ctxs[0], 1, 0, native.comm_unique_id())
    fetched = []

    def fetch():
        fetched.clear()
        for s, x in zip(idx, qs):
            ri, cols = x.fetch_rows()
            fetched.append((s, ri, pipes[0][1]._typed(cols, x.proj_codecs)))

    fetch()
    dseg, drow, dcols = comm.merge_ordered(qs, idx, limit)
    hseg, hrow, hcols = merge_ordered(fetched, okeys, limit)
    assert dseg.astype(np.int64).tolist() == hseg.tolist() and drow.astype(np.int64).tolist() == hrow.tolist()
    assert same(pipes[0][1]._typed(dcols, qs[0].proj_codecs), hcols)
    med, span = interleaved({"device": lambda: comm.merge_ordered(qs, idx, limit),
                             "host": lambda: merge_ordered(fetched, okeys, limit),
                             "host+fetch": lambda: (fetch(), merge_ordered(fetched, okeys, limit))})
    comm.close()
    for x in qs:
        x.close()
    # ---- the whole statement
    if limit:
        run_dev, run_host = (lambda: list(dev_eng.execute(q))), (lambda: list(host_eng.execute(q)))
        assert run_dev() == run_host()
        what = "list(Engine.execute(q))"
    else:
        run_dev = lambda: dev_eng._execute_ordered_device_merge(list(dev_eng.pipelines(q)), limit)                     # noqa: E731
        run_host = lambda: merge_ordered([(s, *p.run_columns()) for s, p in host_eng.pipelines(q)], okeys, limit)[2]  # noqa: E731
        assert same(run_dev(), run_host())
        what = "Engine.execute(q) up to the merged columns"
    smed, sspan = interleaved({"device": run_dev, "host": run_host})
    fmt = lambda k, m, sp: f"{m[k]:10.2f}  ({sp[k][0]:.2f} .. {sp[k][1]:.2f})"                                          # noqa: E731
    lines += [f"limit {limit}: {rows_in} rows enter the merge, {dseg.size} leave it" if limit else f"no limit: {rows_in} rows enter the merge, {dseg.size} leave it",
              f"  merge alone   Comm.merge_ordered (device)                     {fmt('device', med, span)}",
              f"                operators.merge_ordered, arrays already fetched  {fmt('host', med, span)}   x{med['host'] / med['device']:.2f} of the device merge",
              f"                fetch_rows per query + operators.merge_ordered   {fmt('host+fetch', med, span)}   x{med['host+fetch'] / med['device']:.2f}",
              f"  statement     {what}",
              f"                device_merge=True                                {fmt('device', smed, sspan)}",
              f"                device_merge=False (the yardstick)               {fmt('host', smed, sspan)}   x{smed['host'] / smed['device']:.2f} of device_merge=True"]

text = "\n".join(lines)
print(text, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
gsm.close()
shutil.rmtree(d, ignore_errors=True)
