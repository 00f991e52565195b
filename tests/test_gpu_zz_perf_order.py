"""GPU suite, with the other assertions on a TIME (`zz`): the top-k path of ORDER BY.  `select id, age ... where age in (18, 30) order
by age desc limit 10` over 16 M rows (1.76 M survivors) through the radix select must cost no more than 1.25 x the same query with
every survivor sorted (tuning variant 23 pins the full sort); 1.25 is the bound the project's perf tests use for event noise at this
size.  An ordered run cannot be recorded into a graph, so both sides are timed with an event pair on the context's stream around ten
back-to-back runs of the settled query, each side twice, the better one kept."""
import numpy as np
import pytest

from immutable3_amd import native, synth

pytestmark = pytest.mark.gpu
TV_ORDER_FULL_SORT = 23


def runs_us(ctx, q, runs=10):
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    q.run()
    ctx.sync()
    a.record(stream)
    for _ in range(runs):
        q.run()
    b.record(stream)
    ctx.sync()
    return a.elapsed_time(b) / runs * 1e3


def test_top_k_select_is_not_slower_than_the_full_sort():
    N = 16_000_000
    ctx = native.Context(0)
    ids = np.arange(N, dtype=np.int32)
    age = synth.uniform_below(2, N, 100, np.int8)
    seg = native.DeviceSegment(ctx, [
        (native.DENSE_INT, 4, ids.view(np.uint8), N * 4, synth.block_offsets(N, 4)),
        (native.DENSE_TINYINT, 1, age.view(np.uint8), N, synth.block_offsets(N, 1))])
    t = {}
    try:
        for name, variant in (("select", 0), ("full sort", TV_ORDER_FULL_SORT)):
            ctx.set_tuning(variant, 0)
            q = native.DeviceQuery(ctx, seg, [1, 0], [(0, native.GT, 18.0), (0, native.LT, 30.0)], [1, 0], 0, 1024)
            q.set_order([(1, True)], 10)
            q.run()
            assert q.row_count() == 10                   # (settled: the arrays are sized, later runs do not wait for the device)
            rows = q.fetch_rows()
            t[name] = min(runs_us(ctx, q), runs_us(ctx, q))
            plan = q.plan()
            assert (plan["order_select_runs"] > 0) == (variant == 0) and (plan["order_full_runs"] > 0) == (variant != 0), (name, plan)
            t[name + " rows"] = (rows[0].tolist(), [v.tobytes() for v in rows[1]])
            q.close()
        ctx.set_tuning(0, 0)
    finally:
        ctx.set_tuning(0, 0)
        seg.close()
        ctx.close()
    assert t["select rows"] == t["full sort rows"]        # the select's result IS the full sort's first ten rows
    keep = np.flatnonzero((age > 18) & (age < 30))
    want = keep[np.lexsort((keep, -age[keep].astype(np.int64)))][:10]
    assert t["select rows"][0] == want.tolist()
    print(f"top-10 of {keep.size} survivors: select {t['select']:.1f} us, full sort {t['full sort']:.1f} us per query")
    assert t["select"] <= 1.25 * t["full sort"], t
