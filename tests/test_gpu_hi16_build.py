"""GPU suite: k_hi16_build, the kernel that makes a DENSE_INT column's 16-bit high-half plane (SegCol::d_hi16) once,
when the first range query over the column is created.  It takes four grid strides per iteration (eight loads before the first
use), the strides that are left one at a time, and the rows behind the last whole group of eight one per thread; it also reduces the
smallest and largest half, by which the column keeps its plane or not (hi16_span_ok).  Plane and span against numpy, read back
through imm3_segment_hi16_plane."""
import numpy as np
import pytest

from conftest import DENSE_INT, GT, LT, RawColumn, blocks_of

pytestmark = pytest.mark.gpu
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
GROUP = 8 * 256 * 4  # rows one work-group takes per iteration: 8 per thread and stride, four strides


@pytest.fixture(scope="module")
def ctx():
    from immutable3_amd import native
    c = native.Context(0)
    yield c
    c.close()


def build_and_check(ctx, v, what):
    from immutable3_amd import native
    n = v.size
    seg = native.DeviceSegment(ctx, [RawColumn(DENSE_INT, 4, v, blocks_of(n, 1024)).native()])
    assert seg.hi16_plane(0, n)[0] == 0, what                       # nobody has asked yet
    q = native.DeviceQuery(ctx, seg, [0], [(0, GT, -5.0), (0, LT, 5.0)])  # creation builds the plane
    half = (v.astype(np.int64) >> 16).astype(np.int16)
    state, span, plane = seg.hi16_plane(0, n)
    assert span == (int(half.min()), int(half.max())), (what, span)
    keeps = native.plan_hi16_span_ok(int(half.min()), int(half.max()))
    assert state == (1 if keeps else -1), (what, state)
    if keeps:
        assert plane.shape == (n,) and np.array_equal(plane, half), (what, np.flatnonzero(plane != half)[:8])
    q.run()
    assert q.count() == int(((v > -5) & (v < 5)).sum()) and q.plan()["hi16_plane"] == keeps, what
    q.close()
    seg.close()


# 1 .. 9: the tail alone, one whole group of eight, one group and a tail; GROUP - 1: one work-group whose last thread falls out of the
# four-stride loop; 5 GROUP + 3: five work-groups, every thread exactly one four-stride iteration, and a tail
@pytest.mark.parametrize("n", [1, 7, 8, 9, GROUP - 1, 5 * GROUP + 3])
def test_plane_and_span(ctx, n):
    rng = np.random.default_rng(n)
    v = rng.integers(INT_MIN, INT_MAX + 1, size=n, dtype=np.int64).astype(np.int32)
    if n >= 2:
        at = rng.permutation(n)[:2]
        v[at[0]], v[at[1]] = INT_MIN, INT_MAX
    build_and_check(ctx, v, ("random", n))
    if n >= 7:  # the extremes in the tail rows and in the first group, zeros elsewhere; and a span too small for a plane
        w = np.zeros(n, np.int32)
        w[n - 1], w[0] = INT_MIN, INT_MAX
        build_and_check(ctx, w, ("extremes at the ends", n))
        build_and_check(ctx, rng.integers(-70000, 70000, size=n).astype(np.int32), ("four halves", n))


def test_a_column_past_the_grid_cap(ctx):
    """2048 work-groups at most: from 16.8 M rows on a thread takes more than one iteration -- here one of four strides, one single
    stride, and part of the threads one more"""
    rng = np.random.default_rng(2048)
    n = 2048 * GROUP + 2048 * 256 * 8 + 8 * 100_000 + 5
    v = rng.integers(INT_MIN, INT_MAX + 1, size=n, dtype=np.int64).astype(np.int32)
    v[n - 2], v[n // 2] = INT_MIN, INT_MAX
    build_and_check(ctx, v, ("past the cap", n))
