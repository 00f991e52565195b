"""Views of merged groups (imm3_comm_merge_groups_view) against what a caller did before: writes profiles/merge_view.txt.

Two segment queries `group by key` with MAX(age) and COUNT, merged to 51 / 2048 / 2^17 / 2^20 groups; the view `order by age_max desc
limit 10`, with and without `having count > 0`.  Per row: the path the view took, the device time of the view's launches (kernel id 9:
from its first kernel's start to its last one's end), the wall time of one merge_groups_view call, and the wall time of one
merge_groups_wide(..., max_groups=total) call plus the numpy filter and np.lexsort.  Medians of --rounds rounds.

    python tools/merge_view_bench.py [--rounds 5] [--out profiles/merge_view.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from immutable3_amd import native, synth  # noqa: E402

C, MX, A = native.AGG_COUNT, native.AGG_MAX, native.GROUP_ORDER_AGG
PATHS = {native.GROUP_ORDER_NONE: "none", native.GROUP_ORDER_SMALL: "small", native.GROUP_ORDER_RADIX_FULL: "radix full", native.GROUP_ORDER_RADIX_SELECT: "radix select"}


def case(ctx, comm, groups, rounds, out):
    rng = np.random.default_rng(groups)
    rows = max(groups // 2, 1 << 16)                     # per segment
    segs, queries = [], []
    for s in range(2):
        # many groups: the segments hold disjoint halves of the keys (every merged group comes from one query); few: both hold all
        keys = (rng.permutation(rows) + s * rows if groups >= 2 * rows else rng.integers(0, groups, size=rows)).astype(np.int32)
        age = rng.integers(-128, 128, size=rows).astype(np.int8)
        segs.append(native.DeviceSegment(ctx, [(native.DENSE_INT, 4, keys.view(np.uint8), rows * 4, synth.block_offsets(rows, 4)),
                                               (native.DENSE_TINYINT, 1, age.view(np.uint8), rows, synth.block_offsets(rows, 1))]))
        q = native.DeviceQuery(ctx, segs[-1], [0, 1], [], (), 0, 1024, group_cols=[0], aggs=[(MX, 1), (C, 0)])
        q.run()
        queries.append(q)
    seg_index = [0, 1]
    total = comm.merge_groups_wide(queries, seg_index, max_groups=0)[5]
    for having in (False, True):
        leaves, prog = ([(native.GROUP_FILTER_COUNT, 0, native.GT, 0)], [0]) if having else ([], [])
        view = dict(order=[(A, 0, True)], leaves=leaves, prog=prog, limit=10)
        comm.merge_groups_view(queries, seg_index, **view)
        ctx.timing_reset()
        new, old = [], []
        for _ in range(rounds):
            ctx.sync()
            t0 = time.perf_counter()
            keys, first, counts, vals, _, n = comm.merge_groups_wide(queries, seg_index, max_groups=total)
            kept = np.flatnonzero(counts > 0) if having else np.arange(n)
            top = kept[np.lexsort((first[kept], -vals[kept, 0]))[:10]]
            want = (keys[top].tolist(), first[top].tolist(), vals[top].tolist())
            old.append(time.perf_counter() - t0)
            ctx.sync()
            t0 = time.perf_counter()
            got = comm.merge_groups_view(queries, seg_index, **view)
            new.append(time.perf_counter() - t0)
            assert (got[0].tolist(), got[1].tolist(), got[3].tolist()) == want and got[5] == kept.size
        dev = ctx.timing_collect(9)
        assert dev.size == rounds
        new_ms, old_ms = float(np.median(new)) * 1e3, float(np.median(old)) * 1e3
        what = f"group by key{' having count > 0' if having else ''} order by age_max desc limit 10"
        out.write(f"{what:<62}{total:>9}{PATHS[comm.merge_view_path()]:>14}{float(np.median(dev)) * 1e3:>10.1f}{new_ms:>9.2f}   ({min(new) * 1e3:.2f} - {max(new) * 1e3:.2f})"
                  f"{old_ms:>9.2f}{new_ms / old_ms:>9.3f}\n")
    for q in queries:
        q.close()
    for s in segs:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_view.txt"))
    args = ap.parse_args()
    ctx = native.Context(0)
    comm = native.Comm(ctx, 1, 0, native.comm_unique_id())
    ctx.timing_enable(256)
    ctx.timing_mask(1 << 9)
    with open(args.out, "w") as out:
        out.write(f"# two segment queries merged on one rank; view = device time of the launches of one view (kernel id 9), us; new = wall time of one merge_groups_view\n"
                  f"# call, ms; old = wall time of merge_groups_wide(max_groups=total) + numpy filter + np.lexsort + cut, ms; medians of {args.rounds}\n")
        out.write(f"{'statement':<62}{'groups':>9}{'path':>14}{'view us':>10}{'new ms':>9}   (min - max)   {'old ms':>6}{'new/old':>9}\n")
        for groups in (51, 2048, 1 << 17, 1 << 20):
            case(ctx, comm, groups, args.rounds, out)
    comm.close()
    ctx.close()
    print(open(args.out).read())


if __name__ == "__main__":
    main()
