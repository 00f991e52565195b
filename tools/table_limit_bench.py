#!/usr/bin/env python3
"""Development tool: what stopping a table query's scan at its `limit` buys, and what it costs when the scan cannot stop.  The
README-shaped table -- 98 segments of 1 024 001 rows (the loader's quirk: a trailing one-row block), id:int32 ascending, age:int8 --
and four projections with `limit 10`:
  readme    select id, age where (age > 18 and age < 30)            the reference's own README query
  id>5      select id where id > 5                                   survivors from the first tile on
  last      select id where id > <a row of the last segment>         the limit is met in the last segment: every tile is read
  none      select age where age > 100                               nothing survives: every tile is read
Kernel time of one run = the sum of ALL its launches (select, offsets scan, gather, count reduce) by the library's event timing;
median of RUNS runs per query.  One SESSION = one fresh process that builds the table and measures the four queries; the driver
alternates sessions of this checkout's library with sessions of another build of it (--other: the parent commit's libimm3.so), so
that both see the same machine state, and prints every session's medians, the median over the sessions and the spread between a
build's own sessions.  The rows of every query are checked against numpy in every session.

    python tools/table_limit_bench.py [--other /path/to/parent/libimm3.so] [--sessions 3] [out.txt]"""
import json
import os
import subprocess
import sys

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
RUNS = 15
SEGS, SEG_ROWS = 98, 1_024_001
NAMES = ["readme", "id>5", "last", "none"]


def session():
    import numpy as np
    from immutable3_amd import native, synth
    GT, LT = native.GT, native.LT
    ctx = native.Context(0)
    n = SEGS * SEG_ROWS
    ids = np.arange(n, dtype=np.int32)
    age = synth.uniform_below(2, n, 100, np.int8)
    segs = []
    for s in range(SEGS):
        lo, hi = s * SEG_ROWS, (s + 1) * SEG_ROWS
        blocks = [1024] * (SEG_ROWS // 1024) + [SEG_ROWS % 1024]
        o4 = np.concatenate([[0], np.cumsum(np.array(blocks, np.int64) * 4)]).astype(np.int32)
        o1 = np.concatenate([[0], np.cumsum(np.array(blocks, np.int64))]).astype(np.int32)
        segs.append(native.DeviceSegment(ctx, [(native.DENSE_INT, 4, ids[lo:hi].view(np.uint8), SEG_ROWS * 4, o4),
                                               (native.DENSE_TINYINT, 1, age[lo:hi].view(np.uint8), SEG_ROWS, o1)]))
    table = native.DeviceTable(ctx, segs)
    last = (SEGS - 1) * SEG_ROWS + 500_000
    specs = [([1, 0], [(0, GT, 18.0), (0, LT, 30.0)], [1, 0], (age > 18) & (age < 30)),
             ([0], [(0, GT, 5.0)], [0], ids > 5),
             ([0], [(0, GT, float(last))], [0], ids > last),
             ([1], [(0, GT, 100.0)], [0], np.zeros(n, bool))]
    out = {}
    for name, (used, sels, proj, keep) in zip(NAMES, specs):
        q = native.DeviceQuery(ctx, table, used, sels, proj, 10, 1024)
        want = np.flatnonzero(keep)[:10]
        for _ in range(3):
            q.run()
        idx, _ = q.fetch_rows()
        seg_of, row_of = q.locate_rows(idx)
        assert idx.size == want.size and (seg_of == want // SEG_ROWS).all() and (row_of == want % SEG_ROWS).all(), name
        head = np.zeros(16, np.uint64)
        import ctypes as C
        hip = C.CDLL("libamdhip64.so")
        ctx.sync()
        assert hip.hipMemcpy(C.c_void_p(head.ctypes.data), C.c_void_p(q.device_ptr(1)), C.c_size_t(head.nbytes), C.c_int(2)) == 0
        ctx.timing_enable(64)
        us, parts = [], []
        for _ in range(RUNS):
            ctx.timing_reset()
            q.run()
            ctx.sync()
            per = [float(ctx.timing_collect(k).sum()) * 1e3 for k in range(4)]   # select, offsets scan, gather, count reduce
            us.append(sum(per))
            parts.append(per)
        ctx.timing_enable(0)
        parts = np.median(np.array(parts), axis=0)
        out[name] = {"us": float(np.median(us)), "min_us": float(np.min(us)), "select_us": float(parts[0]), "scan_us": float(parts[1]),
                     "gather_us": float(parts[2]), "scanned_tiles": int(head[12])}
        q.close()
    print("SESSION " + json.dumps(out), flush=True)


def driver(argv):
    other, sessions, out_path = None, 3, None
    i = 0
    while i < len(argv):
        if argv[i] == "--other":
            other, i = argv[i + 1], i + 2
        elif argv[i] == "--sessions":
            sessions, i = int(argv[i + 1]), i + 2
        else:
            out_path, i = argv[i], i + 1
    import statistics
    builds = [("this", None)] + ([("other", other)] if other else [])
    res = {b: [] for b, _ in builds}
    lines = [f"# README-shaped table, {SEGS} x {SEG_ROWS} rows; `limit 10`; kernel time of one run (all launches), us, median of {RUNS} runs per session;",
             "# sessions alternate between the builds (this = this checkout, other = --other); tiles = the scanned-tile word after a run (0: nobody set it)",
             f"{'build':>6s} {'session':>7s} " + " ".join(f"{n:>9s} {'select':>7s} {'tiles':>6s}" for n in NAMES)]
    print("\n".join(lines), flush=True)
    for s in range(sessions):
        for b, path in builds:
            env = dict(os.environ)
            if path:
                env["IMM3_LIB_PATH"] = path
            else:
                env.pop("IMM3_LIB_PATH", None)
            p = subprocess.run([sys.executable, __file__, "--session"], env=env, capture_output=True, text=True, timeout=600)   # (a fresh process per session: one library per process)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("SESSION ")]
            if p.returncode != 0 or not got:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"session of build '{b}' failed with status {p.returncode}: measuring stops here")
            r = json.loads(got[0][len("SESSION "):])
            res[b].append(r)
            lines.append(f"{b:>6s} {s:7d} " + " ".join(f"{r[n]['us']:9.1f} {r[n]['select_us']:7.1f} {r[n]['scanned_tiles']:6d}" for n in NAMES))
            print(lines[-1], flush=True)
    lines.append("# per build: median over its sessions' medians, and (max - min) of them = the spread between a build's own repeated medians")
    for b, _ in builds:
        meds = {n: [r[n]["us"] for r in res[b]] for n in NAMES}
        lines.append(f"{b:>6s}  median " + " ".join(f"{statistics.median(meds[n]):9.1f} {'':7s} {'':6s}" for n in NAMES))
        lines.append(f"{b:>6s}  spread " + " ".join(f"{max(meds[n]) - min(meds[n]):9.1f} {'':7s} {'':6s}" for n in NAMES))
        print("\n".join(lines[-2:]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--session" in sys.argv[1:]:
        session()
    else:
        driver(sys.argv[1:])
