"""GPU timing (`zz`: with the other assertions on a time): IN (sub-query) through a device-built set must beat the only spelling it had
before -- fetch the inner rows, hand them back as an IMM3_INT_IN leaf.  16 M rows on either side, 10^5 distinct values in the inner
selection (about half the inner rows selected); wall-clock time of the whole route, host work included, in one process:
  new   imm3_int_set_create over the inner query + creation of the consumer with the IMM3_INT_IN_SET leaf + its run + its count
  old   imm3_query_fetch_rows of the inner projection + numpy.unique over those rows' values + creation of the consumer with IMM3_INT_IN
        over them (query creation builds the probe table on the CPU and uploads it) + its run + its count
Both inner queries have run before the clock starts; the routes are alternated round by round, median of 5 rounds, no margin -- the new
route must be STRICTLY faster; the old route in the same run is the yardstick, never a stored number.  Both counts are held against
numpy.  Figures on MI355X when this test was written: in the test's docstring below and profiles/int_set.txt."""
import time

import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_TINYINT, GT, RawColumn, blocks_of

pytestmark = pytest.mark.gpu


def test_device_built_set_beats_fetching_the_inner_rows():
    """measured on MI355X when written: device-built set 1.05 ms, fetched rows + numpy.unique + IMM3_INT_IN 45.9 ms (new / old = 0.023)"""
    from immutable3_amd import native
    n, distinct = 16 * 1024 * 1024, 100_000
    rng = np.random.default_rng(17)
    domain = rng.permutation(np.unique(rng.integers(0, 1 << 30, size=2 * distinct + distinct // 4)))[: 2 * distinct].astype(np.int32)
    assert domain.size == 2 * distinct
    inner_ids = domain[rng.integers(0, distinct, size=n)]                       # the inner column: the first 10^5 values of the domain
    flag = rng.integers(-1, 1, size=n).astype(np.int8)                          # ... of which the rows with flag > -1 are selected
    outer_ids = domain[rng.integers(0, 2 * distinct, size=n)]                   # the consumer's column: half its rows are members
    br = blocks_of(n, 1024)
    ctx = native.Context(0)
    inner = native.DeviceSegment(ctx, [RawColumn(DENSE_INT, 4, inner_ids, br).native(), RawColumn(DENSE_TINYINT, 1, flag, br).native()])
    outer = native.DeviceSegment(ctx, [RawColumn(DENSE_INT, 4, outer_ids, br).native()])
    members = np.unique(inner_ids[flag > -1])
    want = int(np.isin(outer_ids, members).sum())
    assert members.size == distinct and 0 < want < n
    src_select = native.DeviceQuery(ctx, inner, [1, 0], [(0, GT, -1.0)])
    src_project = native.DeviceQuery(ctx, inner, [1, 0], [(0, GT, -1.0)], [1], 0, 1024)
    src_select.run_select()
    src_project.run()
    src_select.sync(), src_project.sync()

    def new_route():
        s = native.IntSet(ctx, [(src_select, 1)])
        q = native.DeviceQuery(ctx, outer, [0], [(0, native.INT_IN_SET, s)])
        q.run_select()
        c = q.count()
        q.close(), s.close()
        return c

    def old_route():
        _, cols = src_project.fetch_rows()
        values = np.unique(cols[0].view("<i4").reshape(-1)).tolist()         # (deduplicated here: a list of the 8 M fetched values would cost the old route more)
        q = native.DeviceQuery(ctx, outer, [0], [(0, native.INT_IN, values)])
        q.run_select()
        c = q.count()
        q.close()
        return c

    assert new_route() == want and old_route() == want                          # warm-up (and the answer)
    rounds, t_new, t_old = 5, [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        new_route()
        t1 = time.perf_counter()
        old_route()
        t2 = time.perf_counter()
        t_new.append(t1 - t0)
        t_old.append(t2 - t1)
    new, old = float(np.median(t_new)) * 1e3, float(np.median(t_old)) * 1e3
    print(f"IN (sub-query), 16 M rows, 10^5 values: device-built set {new:.2f} ms; fetched rows + IMM3_INT_IN {old:.2f} ms; new / old = {new / old:.3f}")
    assert new < old
    for h in (src_select, src_project, inner, outer):
        h.close()
    ctx.close()
