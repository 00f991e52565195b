"""GPU suite, with the other assertions on a TIME (`zz`): ORDER BY over groups.

1. The one-work-group launch on 51 groups (`group by state` over 1 M rows, `order by count desc limit 10`) must cost no more than 1.25 x
   the same ordered settle with the radix path pinned (tuning variant 25): the radix path is the projection's order kernels, i.e. what
   plain reuse would cost; 1.25 is the project's allowance for event noise.  Both sides are timed by the library's event pair around
   the ordered settle (kernel id 8: from the first order kernel's start to the last one's end), ten settles a batch, each side twice,
   the better batch kept.
2. The top 10 of ~1 M groups (`group by id` over 1 M distinct ids, `order by age_max desc limit 10`): wall time of set_group_order +
   fetch_groups must not exceed the wall time of what a caller did before on the same query -- fetch_groups of every group, unordered,
   plus np.lexsort.  No margin: the ordered path moves ten groups over PCIe instead of a million; if it is not faster the feature has
   not paid.  Each side twice, the better one kept."""
import time

import numpy as np
import pytest

from immutable3_amd import native, synth

pytestmark = pytest.mark.gpu
C, MX = native.AGG_COUNT, native.AGG_MAX
G, A = native.GROUP_ORDER_GROUP_COL, native.GROUP_ORDER_AGG
N = 1_000_000


def settle_us(ctx, q, order, limit, settles=10):
    """mean device time of one ordered settle's order launches (kernel id 8), over `settles` settles"""
    ctx.timing_reset()
    for _ in range(settles):
        q.set_group_order(order, limit)      # (a change of order: the next getter orders again)
        q.fetch_groups()
    t = ctx.timing_collect(8)
    assert t.size == settles
    return float(t.mean()) * 1e3


def test_small_launch_against_the_pinned_radix_path():
    rng = np.random.default_rng(8)
    ctx = native.Context(0)
    ids = np.arange(N, dtype=np.int32)
    states = np.array([list(b"%c%c" % (65 + i // 26, 65 + i % 26)) for i in range(51)], np.uint8)[rng.integers(0, 51, size=N)]
    seg = native.DeviceSegment(ctx, [
        (native.DENSE_INT, 4, ids.view(np.uint8), N * 4, synth.block_offsets(N, 4)),
        (native.DENSE_STRING, 2, states.reshape(-1), N * 2, synth.block_offsets(N, 2))])
    q = native.DeviceQuery(ctx, seg, [0, 1], [], (), 0, 1024, group_cols=[1], aggs=[(C, 0)])
    order, t, res = [(A, 0, True)], {}, {}
    try:
        q.run()
        ctx.timing_enable(64)
        ctx.timing_mask(1 << 8)
        for name, variant, paths in (("small", 0, (native.GROUP_ORDER_SMALL,)), ("radix", native.TV_GROUP_ORDER_RADIX, (native.GROUP_ORDER_RADIX_FULL, native.GROUP_ORDER_RADIX_SELECT))):
            ctx.set_tuning(variant, 0)
            q.set_group_order(order, 10)
            res[name] = [x.tolist() for x in q.fetch_groups()]
            assert q.group_order_path() in paths, name
            t[name] = min(settle_us(ctx, q, order, 10), settle_us(ctx, q, order, 10))
    finally:
        ctx.set_tuning(0, 0)
        q.close()
        seg.close()
        ctx.close()
    assert res["small"] == res["radix"] and len(res["small"][1]) == 10
    counts = np.bincount(np.unique(states.view(np.uint16).reshape(-1), return_inverse=True)[1].reshape(-1))
    assert res["small"][2] == sorted(counts.tolist(), reverse=True)[:10]
    print(f"top-10 of 51 groups by count: small launch {t['small']:.1f} us, radix path {t['radix']:.1f} us per ordered settle (ratio {t['small'] / t['radix']:.3f})")
    assert t["small"] <= 1.25 * t["radix"], t


def test_top_10_of_a_million_groups_beats_fetch_everything_and_lexsort():
    rng = np.random.default_rng(9)
    ctx = native.Context(0)
    ids = rng.permutation(N).astype(np.int32)
    age = rng.integers(-128, 128, size=N).astype(np.int8)
    seg = native.DeviceSegment(ctx, [
        (native.DENSE_INT, 4, ids.view(np.uint8), N * 4, synth.block_offsets(N, 4)),
        (native.DENSE_TINYINT, 1, age.view(np.uint8), N, synth.block_offsets(N, 1))])
    q = native.DeviceQuery(ctx, seg, [0, 1], [], (), 0, 1024, group_cols=[0], aggs=[(MX, 1)])
    order, t = [(A, 0, True)], {"ordered": [], "fetch all + lexsort": []}
    try:
        q.run()
        assert q.fetch_groups()[1].size == N             # (settled once: the dense arrays are sized)
        q.set_group_order(order, 10)
        q.fetch_groups()                                  # (and the order's buffers)
        for _ in range(2):
            q.set_group_order([], 0)
            ctx.sync()
            t0 = time.perf_counter()
            keys, first, counts, vals = q.fetch_groups()
            top = np.lexsort((first, -vals[:, 0]))[:10]
            old = (keys[top].tolist(), first[top].tolist(), counts[top].tolist(), vals[top].tolist())
            t["fetch all + lexsort"].append(time.perf_counter() - t0)
            ctx.sync()
            t0 = time.perf_counter()
            q.set_group_order(order, 10)
            new = tuple(x.tolist() for x in q.fetch_groups())
            t["ordered"].append(time.perf_counter() - t0)
            assert q.group_order_path() == native.GROUP_ORDER_RADIX_SELECT
            assert new == old
    finally:
        q.close()
        seg.close()
        ctx.close()
    want = np.lexsort((np.arange(N), -age.astype(np.int64)))[:10]
    assert new[1] == want.tolist() and new[0] == ids[want].astype(np.uint32).astype(np.uint64).tolist()
    new_ms, old_ms = min(t["ordered"]) * 1e3, min(t["fetch all + lexsort"]) * 1e3
    print(f"top-10 of {N} groups by age_max: ordered on the device {new_ms:.2f} ms, fetch every group + np.lexsort {old_ms:.2f} ms (ratio {new_ms / old_ms:.3f})")
    assert new_ms <= old_ms, t
