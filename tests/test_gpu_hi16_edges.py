"""GPU suite: the plane scan's tiles with and without rows on an EDGE half (ColRegs<TK_H16>, refine_undecided).  An edge
half is a boundary half of the interval that does not decide itself; only a tile that holds a row with such a half (and that no other
column has failed) compares full values, and only such tiles stop their wave for the loads -- what the launch's work-groups are sized
for.  Here: columns without any edge half, one edge row at every in-lane position of the first, a middle and the last lane, edge rows
in every tile, columns full of a boundary half that decides itself, the int8 + int32 instance with edge rows the int8 column fails or
passes, plane passes that AND into earlier words -- against numpy, with the default grid and with the grid pinned to 1 and 2
work-groups (each wave then walks several tiles: prologue, steady state, last iteration, parked lines, the partial tile)."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_TINYINT, GT, LT, RawColumn, blocks_of

pytestmark = pytest.mark.gpu
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
H = 0x10000
# intervals by what their two boundary halves do: a boundary half decides itself when every value of it lies inside the interval
# (lo & 0xFFFF == 0, hi & 0xFFFF == 0xFFFF); the others are the interval's EDGE halves, the only ones whose rows need their full value
CLASSES = {
    "both edges": [(2 ** 28 + 1, 3 * 2 ** 28 - 2), (5 * H + 1, 9 * H + 0xFFFE), (-7 * H + 0x8000, -3 * H + 0x8000)],
    "lower edge only": [(2 ** 28 + 1, 3 * 2 ** 28 - 1), (5 * H + 0xFFFF, 9 * H + 0xFFFF), (-7 * H + 1, -3 * H - 1)],
    "upper edge only": [(2 ** 28, 3 * 2 ** 28 - 2), (5 * H, 9 * H), (-7 * H, -3 * H + 0xFFFE)],
    "no edge": [(2 ** 28, 3 * 2 ** 28 - 1), (5 * H, 5 * H + 0xFFFF), (-7 * H, -3 * H - 1), (-H, H - 1)],
    "one half": [(5 * H + 3, 5 * H + 9), (5 * H, 5 * H + 9), (5 * H + 3, 5 * H + 0xFFFF), (-2 * H + 7, -2 * H + 7), (-1, -1), (0, 0)],
    "adjacent halves": [(5 * H + 3, 6 * H + 9), (5 * H, 6 * H + 9), (5 * H + 3, 6 * H + 0xFFFF), (5 * H, 6 * H + 0xFFFF), (-H + 5, 5), (-1, 0)],
    "lo < 0 <= hi": [(-1, 0), (-5 * H + 1, 4 * H + 2), (-5 * H, 4 * H + 2), (-5 * H + 1, 4 * H + 0xFFFF), (-0x8000, 0x8000), (-2 ** 30 - 1, 2 ** 30 + 1)],
    "ends of the range": [(INT_MIN, INT_MAX), (INT_MIN, 5), (INT_MIN + 1, 5), (-5, INT_MAX), (-5, INT_MAX - 1), (INT_MIN, INT_MIN), (INT_MAX, INT_MAX),
                          (INT_MIN, INT_MIN + 5), (INT_MAX - 5, INT_MAX), (INT_MIN + 1, INT_MAX - 1), (INT_MIN + 1, INT_MAX), (INT_MIN, INT_MAX - 1)],
    # possible_count 65 535: the window leaves one half out; 65 536: every half is possible
    "count 65535": [(INT_MIN + H, INT_MAX), (INT_MIN + H + 1, INT_MAX - 1), (INT_MIN, INT_MAX - H), (INT_MIN + 1, INT_MAX - H), (INT_MIN + H + 1, INT_MAX)],
    "count 65536": [(INT_MIN, INT_MAX), (INT_MIN + 1, INT_MAX - 1), (INT_MIN + 0xFFFF, INT_MAX - 0xFFFF), (INT_MIN, INT_MAX - 1), (INT_MIN + 1, INT_MAX)],
}
SHAPES = (3 * 1024 + 517, 12 * 1024 + 1)
GRIDS = (0, 1, 2)
# the lane layout of the plane's tile: lane l holds rows 8 l .. + 7 and 512 + 8 l .. + 7
LANE_ROWS = [8 * lane + k + 512 * run for lane in (0, 7, 8, 63) for run in (0, 1) for k in range(8)]


@pytest.fixture(scope="module")
def ctx():
    from immutable3_amd import native
    c = native.Context(0)
    yield c
    c.set_tuning(0, 0)
    c.close()


def words_of(keep):
    bits = np.packbits(keep, bitorder="little")
    return np.concatenate([bits, np.zeros((-bits.size) % 8, np.uint8)]).view("<u8")


def int_col(v):
    return RawColumn(DENSE_INT, 4, np.asarray(v, np.int32), blocks_of(len(v), 1024))


def range_sels(col, lo, hi):
    """lo <= v <= hi; a bound at the end of the int32 range is left out (the other folds to the same closed interval)"""
    return ([(col, GT, float(lo - 1))] if lo > INT_MIN else []) + ([(col, LT, float(hi + 1))] if hi < INT_MAX else [])


def gpu_intervals(name):
    """the intervals of one class that are a predicate at all (two per class: the runs add up)"""
    return [(lo, hi) for lo, hi in CLASSES[name] if (lo, hi) != (INT_MIN, INT_MAX)][:2]


def edge_halves(lo, hi):
    """the undecided halves of [lo, hi] by the library's two windows (at most two), signed, as the plane holds them"""
    from immutable3_amd import native
    pf, pn, cf, cn = native.plan_hi16_bounds(lo, hi)
    h = np.arange(65536, dtype=np.int64)
    und = h[(((h - pf) & 0xFFFF) < pn) & ~(((h - cf) & 0xFFFF) < cn)]
    want = sorted({x >> 16 for x, open_ in ((lo, (lo & 0xFFFF) != 0), (hi, (hi & 0xFFFF) != 0xFFFF)) if open_})
    got = sorted(int(e) - 65536 if e >= 32768 else int(e) for e in und)
    assert got == want, (lo, hi, got, want)
    for e in got:
        assert native.plan_hi16_class(lo, hi, e) == native.HI16_UNDECIDED
    return got


def column_without(rng, n, lo, hi, avoid):
    """n values over the whole range, a third of them within three halves of a boundary, none with a half in `avoid`"""
    near = np.array([(x >> 16) + d for x in (lo, hi) for d in (-3, -2, -1, 0, 1, 2, 3)], np.int64).clip(-32768, 32767)
    half = np.where(rng.integers(0, 3, size=n) == 0, near[rng.integers(0, near.size, size=n)], rng.integers(-32768, 32768, size=n))
    for _ in range(64):
        bad = np.isin(half, avoid)
        if not bad.any():
            break
        half[bad] = rng.integers(-32768, 32768, size=int(bad.sum()))
    assert not np.isin(half, avoid).any()
    v = (half << 16) + rng.integers(0, H, size=n)
    v[0], v[n - 1] = (-32768 << 16) + 5 if -32768 not in avoid else (-32767 << 16), (32767 << 16) + 5 if 32767 not in avoid else (32766 << 16)
    return v.astype(np.int32)


def check(ctx, q, keep, what, grids=GRIDS, refined=None):
    """every grid: a bitmap run and a count-only run, each exact, each over the plane, and -- refined given -- each saying whether a
    tile took the refine (q.hi16_refined(): set on the device by such a tile, read and cleared by the call)"""
    want = words_of(keep)
    total = int(keep.sum())
    try:
        for grid in grids:
            ctx.set_tuning(0, grid)
            q.run()
            got = q.bitmap()
            plan = q.plan()
            assert plan["hi16_plane"], (what, grid, plan)
            assert refined is None or q.hi16_refined() == refined, (what, grid, plan)
            assert q.count() == total, (what, grid)
            assert got[: want.size].tolist() == want.tolist() and not got[want.size:].any(), (what, grid)
            q.run_count()
            plan = q.plan()
            assert q.count() == total and plan["hi16_plane"], (what, grid, "count-only")
            assert refined is None or q.hi16_refined() == refined, (what, grid, "count-only", plan)
    finally:
        ctx.set_tuning(0, 0)


def one_query(ctx, v, lo, hi, what, refined, grids=GRIDS):
    from immutable3_amd import native
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
    check(ctx, q, (v >= lo) & (v <= hi), what, grids, refined)
    q.close()
    seg.close()


@pytest.mark.parametrize("name", list(CLASSES))
def test_columns_without_an_edge_half(ctx, name):
    """no tile has an undecided row: the launch never reads the column itself"""
    rng = np.random.default_rng(sorted(CLASSES).index(name))
    for lo, hi in gpu_intervals(name):
        edges = edge_halves(lo, hi)
        for n in SHAPES:
            v = column_without(rng, n, lo, hi, edges)
            one_query(ctx, v, lo, hi, (name, lo, hi, n), refined=False)


def walk(ctx, rng, lo, hi, n, what):
    """One edge-half row per full tile of an otherwise edge-free column, at every position of LANE_ROWS, its full value just inside and
    just outside the interval, for each edge: as many columns as it takes to place them all, one row per tile."""
    edges = edge_halves(lo, hi)
    plants = []  # (position in the tile, value)
    for e in edges:
        inside_outside = []
        if e == lo >> 16 and (lo & 0xFFFF) != 0:
            inside_outside += [lo, lo - 1]
        if e == hi >> 16 and (hi & 0xFFFF) != 0xFFFF:
            inside_outside += [hi, hi + 1]
        assert inside_outside and all(x >> 16 == e for x in inside_outside), (lo, hi, e)
        plants += [(pos, x) for x in inside_outside for pos in LANE_ROWS]
    full = n // 1024
    for first in range(0, len(plants), full):
        v = column_without(rng, n, lo, hi, edges)
        for tile, (pos, x) in enumerate(plants[first: first + full]):
            v[1024 * tile + pos] = x
        one_query(ctx, v, lo, hi, what + (first,), refined=True)


WALKED = [name for name in CLASSES if name != "no edge"]


@pytest.mark.parametrize("name", WALKED)
def test_one_edge_row_at_every_lane_position(ctx, name):
    rng = np.random.default_rng(100 + WALKED.index(name))
    walked = 0
    for lo, hi in gpu_intervals(name):
        if not edge_halves(lo, hi):
            continue
        walk(ctx, rng, lo, hi, SHAPES[1] if walked else SHAPES[0], (name, lo, hi))  # (the first interval over the short shape, the second over the long one)
        walked += 1
    assert walked, name


def test_the_same_walk_over_negative_halves(ctx):
    rng = np.random.default_rng(7)
    walk(ctx, rng, -7 * H + 0x1234, -3 * H + 0x4321, SHAPES[1], ("negative",))
    walk(ctx, rng, -0x8000, 0x8000, SHAPES[0], ("around zero",))


@pytest.mark.parametrize("name", WALKED)
def test_edge_rows_in_every_tile(ctx, name):
    rng = np.random.default_rng(200 + WALKED.index(name))
    for lo, hi in gpu_intervals(name):
        edges = edge_halves(lo, hi)
        if not edges:
            continue
        for n in SHAPES:
            v = column_without(rng, n, lo, hi, edges).astype(np.int64)
            at = rng.integers(1, n - 1, size=n // 16)
            near = np.array([lo - 1, lo, lo + 1, hi - 1, hi, hi + 1], np.int64).clip(INT_MIN, INT_MAX)
            planted = np.where(rng.integers(0, 2, size=at.size) == 0, near[rng.integers(0, near.size, size=at.size)],
                               (np.array(edges, np.int64)[rng.integers(0, len(edges), size=at.size)] << 16) + rng.integers(0, H, size=at.size))
            v[at] = planted
            v = v.astype(np.int32)
            assert all(np.isin((v[1024 * t: 1024 * (t + 1)].astype(np.int64) >> 16), edges).any() for t in range(n // 1024)), (name, n)
            one_query(ctx, v, lo, hi, (name, lo, hi, n), refined=True)


def test_a_boundary_half_that_decides_itself_sends_no_tile_to_the_refine(ctx):
    """every tile is full of both boundary halves, both decide themselves: no half is undecided, the result is exact and no tile refines"""
    rng = np.random.default_rng(11)
    for lo, hi in CLASSES["no edge"]:
        for n in SHAPES:
            v = column_without(rng, n, lo, hi, []).astype(np.int64)
            at = rng.integers(1, n - 1, size=n // 2)
            v[at] = (np.array([lo >> 16, hi >> 16, (lo >> 16) - 1, (hi >> 16) + 1], np.int64)[rng.integers(0, 4, size=at.size)] << 16) + rng.integers(0, H, size=at.size)
            v = v.astype(np.int32)
            assert not edge_halves(lo, hi)
            one_query(ctx, v, lo, hi, ("no edge", lo, hi, n), refined=False)


def pair_segment(ctx, age, ids):
    from immutable3_amd import native
    n = age.size
    return native.DeviceSegment(ctx, [RawColumn(DENSE_TINYINT, 1, age, blocks_of(n, 1024)).native(), int_col(ids).native()])


@pytest.mark.parametrize("n", SHAPES)
def test_int8_beside_the_plane_false_alarms_and_refines(ctx, n):
    """<I8, H16>: tile 0 holds one edge row that the int8 column FAILS (nothing is left undecided), tile 1 one that it passes, inside
    the interval, tile 2 one that it passes, outside; the other tiles hold no edge half.  First with tile 0's row alone -- a false
    alarm: no tile refines -- then with all three."""
    from immutable3_amd import native
    rng = np.random.default_rng(n)
    lo, hi = 5 * H + 0x1000, 9000 * H + 0x2000
    edges = edge_halves(lo, hi)
    assert len(edges) == 2
    for pos in (0, 63, 64, 511, 512, 519, 1016, 1023):
        ids = column_without(rng, n, lo, hi, edges)
        age = rng.integers(-128, 128, size=n).astype(np.int8)
        ids[pos], age[pos] = lo + 5, -100                # passes the range, fails the int8 test
        for refined in (False, True):
            if refined:
                ids[1024 + pos], age[1024 + pos] = hi - 5, 7     # passes both
                ids[2048 + pos], age[2048 + pos] = hi + 5, 7     # on the edge half, outside the range
            keep = (age > -20) & (age < 90) & (ids >= lo) & (ids <= hi)
            assert not keep[pos] and (not refined or (keep[1024 + pos] and not keep[2048 + pos]))
            seg = pair_segment(ctx, age, ids)
            for used, sels in (([0, 1], [(0, GT, -20.0), (0, LT, 90.0)] + range_sels(1, lo, hi)), ([1, 0], range_sels(0, lo, hi) + [(1, GT, -20.0), (1, LT, 90.0)])):
                q = native.DeviceQuery(ctx, seg, used, sels)
                check(ctx, q, keep, ("pair", n, pos, used, refined), refined=refined)
                q.close()
            seg.close()


@pytest.mark.parametrize("n", SHAPES)
def test_plane_passes_that_and_into_earlier_words(ctx, n):
    """Four int32 ranges and an int8 one: the first three int32 columns go through one int32 launch, the int8 column and the fourth
    int32 column through <I8, H16>, which ANDs into that launch's words; and four int32 ranges alone: the last one, <H16>, does.  Edge rows
    of the plane's column in every tile, some failed and some passed by the earlier pass."""
    from immutable3_amd import native
    rng = np.random.default_rng(3 * n)
    lo, hi = -40 * H + 0x7777, 11000 * H + 0x0101
    edges = edge_halves(lo, hi)
    three = [rng.integers(0, 2 ** 30, size=n).astype(np.int32) for _ in range(3)]
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    ids = column_without(rng, n, lo, hi, edges).astype(np.int64)
    at = rng.integers(1, n - 1, size=n // 8)
    ids[at] = np.array([lo - 1, lo, hi, hi + 1], np.int64)[rng.integers(0, 4, size=at.size)]
    ids = ids.astype(np.int32)
    keep3 = np.ones(n, bool)
    sels3 = []
    for k, x in enumerate(three):
        lo_k, hi_k = 2 ** 26 + 1000 * k + 1, 2 ** 30 - 2 ** 26 - 17 * k
        sels3 += range_sels(k, lo_k, hi_k)
        keep3 &= (x >= lo_k) & (x <= hi_k)
    in_range = (ids >= lo) & (ids <= hi)
    cols = [int_col(x).native() for x in three] + [RawColumn(DENSE_TINYINT, 1, age, blocks_of(n, 1024)).native(), int_col(ids).native()]
    seg = native.DeviceSegment(ctx, cols)
    q = native.DeviceQuery(ctx, seg, [0, 1, 2, 3, 4], sels3 + [(3, GT, -20.0), (3, LT, 90.0)] + range_sels(4, lo, hi))
    check(ctx, q, keep3 & (age > -20) & (age < 90) & in_range, ("three int32, then int8 + plane", n), refined=True)
    q.close()
    q = native.DeviceQuery(ctx, seg, [0, 1, 2, 4], sels3 + range_sels(3, lo, hi))
    check(ctx, q, keep3 & in_range, ("three int32, then the plane", n), refined=True)
    q.close()
    seg.close()


def test_a_column_large_enough_for_the_plane_s_own_grid(ctx):
    """12.6 M rows: 12 293 tiles, more than the 6144 waves of the lone plane's 1536 work-groups (twice the 768 of a 2-byte column), so
    that the default launch runs that grid with two or three tiles per wave, the last iteration's prefetch of the shared group 0
    included; the headline's interval shape (one edge) and a two-edge one, edge rows scattered at the uniform column's rate"""
    from immutable3_amd import native
    rng = np.random.default_rng(1536)
    n = 2 * 1536 * 4 * 1024 + 5 * 1024 + 3
    v = rng.integers(0, 2 ** 30, size=n, dtype=np.int64).astype(np.int32)
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    for lo, hi in ((2 ** 28 + 1, 3 * 2 ** 28 - 1), (1000001, 790000000)):
        q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
        check(ctx, q, (v >= lo) & (v <= hi), ("large", lo, hi), grids=(0,), refined=True)
        q.close()
    seg.close()
