"""GPU suite: int32 range filters over the 16-bit high-half plane (SegCol::d_hi16, the TK_H16 kind of k_filter_tile).
A DENSE_INT column that a segment query range-filters gets, once, a plane of (int16)(v >> 16); the scan reads the plane, decides every
row whose half lies strictly between (or outside) the interval's boundary halves, and compares the full value of the others in the
same launch.  Bitmap and count are bit-exact against numpy and the oracle everywhere; plan()["hi16_plane"] says which path ran."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, EQ, GT, LT, MATCH, RawColumn, blocks_of

pytestmark = pytest.mark.gpu
PAD = 16384  # the slack behind every device column (and behind its plane)


@pytest.fixture(scope="module")
def ctx():
    from immutable3_amd import native
    c = native.Context(0)
    yield c
    c.close()


def words_of(keep):
    bits = np.packbits(keep, bitorder="little")
    return np.concatenate([bits, np.zeros((-bits.size) % 8, np.uint8)]).view("<u8")


def int_col(v):
    return RawColumn(DENSE_INT, 4, np.asarray(v, np.int32), blocks_of(len(v), 1024))


def between(v, lo, hi):
    """[(0, GT, lo - 1), (0, LT, hi + 1)] selects lo <= v <= hi (INT_MIN < lo, hi < INT_MAX: the doubles hold them exactly)"""
    return (v >= lo) & (v <= hi)


def range_sels(col, lo, hi):
    return [(col, GT, float(lo - 1)), (col, LT, float(hi + 1))]


def check_select(q, keep, plane, what):
    """one run: count, every bitmap word, zero padding, the count-only instance, and which path ran"""
    q.run()
    want = words_of(keep)
    got = q.bitmap()
    assert q.count() == int(keep.sum()), what
    assert got[: want.size].tolist() == want.tolist(), what
    assert not got[want.size:].any(), what
    if plane is not None:
        assert q.plan()["hi16_plane"] == plane, (what, q.plan())


def undecided_full_tiles(v, lo, hi):
    """tiles (full ones: the rolled last tile reads the column itself) that hold a row the halves cannot decide -- the host's rule"""
    from immutable3_amd import native
    pf, pn, cf, cn = native.plan_hi16_bounds(lo, hi)
    h = (v.astype(np.int64) >> 16) & 0xFFFF
    und = (((h - pf) & 0xFFFF) < pn) & ~(((h - cf) & 0xFFFF) < cn)
    full = (v.size // 1024) * 1024
    return np.unique(np.flatnonzero(und[:full]) // 1024)


SIZES = [1024 * k + r for k, r in ((1, 0), (3, 1), (17, 63), (64, 777), (0, 777))]


def test_threshold_sweep_over_uniform_int30(ctx, oracle):
    """Both boundaries at every alignment around a half's edge; values planted on and beside every threshold so that each alignment
    has rows on both sides in several tiles.  EQ, and GT / LT from doubles -- NaN and +-1e12 among them (they fold to a bound, to
    every row or to none) -- against the oracle."""
    from immutable3_amd import native, synth
    n = 64 * 1024 + 777
    v = synth.uniform_int30(16, n).copy()
    lo_edge, hi_edge = 2 ** 28, 3 * 2 ** 28
    aligns = (0, 1, 0x7FFF, 0xFFFF, 0x10000)
    rng = np.random.default_rng(1)
    for edge in (lo_edge, hi_edge):
        for a in aligns:
            for d in (-1, 0, 1):
                v[rng.integers(0, n, size=6)] = edge + a + d
    col = int_col(v)
    seg = native.DeviceSegment(ctx, [col.native()])
    b0 = seg.device_bytes
    cases = [[(0, EQ, float(lo_edge + a))] for a in aligns]
    cases += [[(0, GT, float(lo_edge + a)), (0, LT, float(hi_edge + b))] for a in aligns for b in aligns]
    cases += [[(0, GT, float("nan"))], [(0, LT, float("nan"))], [(0, GT, 1e12)], [(0, LT, 1e12)], [(0, GT, -1e12)], [(0, LT, -1e12)],
              [(0, GT, -1e12), (0, LT, 1e12)], [(0, GT, float(lo_edge)), (0, LT, 1e12)], [(0, GT, -1e12), (0, LT, float(hi_edge + 1))]]
    planes = 0
    for sels in cases:
        ow, oc = oracle.scan_select([col.ocol()], sels, 1024, 1)
        q = native.DeviceQuery(ctx, seg, [0], sels)
        q.run()
        assert q.count() == oc and q.bitmap().tolist() == ow.tolist(), sels
        planes += q.plan()["hi16_plane"]
        if oc:  # (a query that selects nothing by construction launches nothing)
            assert q.plan()["hi16_plane"], sels
        q.run_count()
        assert q.count() == oc, (sels, "count-only")
        q.close()
    assert planes >= len(cases) - 3
    assert seg.device_bytes == b0 + 2 * n + PAD
    seg.close()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_ragged_ends(ctx, n):
    from immutable3_amd import native, synth
    v = synth.uniform_int30(n, n)
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    for lo, hi in ((2 ** 28 + 1, 3 * 2 ** 28 - 1), (2 ** 28 + 0x8000, 2 ** 28 + 0x9000), (0x10000, 2 ** 30)):
        q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
        check_select(q, between(v, lo, hi), True, (n, lo, hi))
        q.close()
    seg.close()


def test_sorted_columns(ctx):
    """id = i over 200 000 rows spans four halves: it gets NO plane (fewer than 64) and runs as before.  id = 64 i is the same sorted
    shape with one half per tile: the tiles of the two boundary halves are undecided in every row, the others in none.  And the same
    straddling zero."""
    from immutable3_amd import native
    n = 200_000
    i = np.arange(n, dtype=np.int64)
    for name, v, plane in (("id = i", i, False), ("id = 64 i", 64 * i, True), ("signed", 64 * (i - n // 2) - 7, True)):
        v = v.astype(np.int32)
        seg = native.DeviceSegment(ctx, [int_col(v).native()])
        for lo, hi in ((int(v[70_000]) + 5, int(v[150_000]) + 9), (int(v[1000]), int(v[1000])), (int(v[3]) - 1, int(v[n - 2])),
                       (int(v[65_536 + 512]), int(v[131_072 - 1]))):
            q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
            check_select(q, between(v, lo, hi), plane, (name, lo, hi))
            q.run_count()
            assert q.count() == int(between(v, lo, hi).sum()), (name, lo, hi)
            q.close()
        if plane:
            t = undecided_full_tiles(v, int(v[70_000]) + 5, int(v[150_000]) + 9)
            assert t.size == (2 if name == "id = 64 i" else 4), t  # one whole tile per boundary half (two where a half straddles tiles)
        seg.close()


def test_every_tile_takes_the_refine(ctx):
    """every row shares its half with both thresholds; two far outliers give the column the span a plane needs"""
    from immutable3_amd import native
    rng = np.random.default_rng(3)
    for n in (20 * 1024 + 63, 5 * 1024):
        for half in (0x1234, -0x0042):
            v = ((half << 16) + rng.integers(0, 1 << 16, size=n)).astype(np.int64)
            v[7], v[n - 9] = -(2 ** 31) + 5, 2 ** 31 - 5
            v = v.astype(np.int32)
            lo, hi = (half << 16) + 0x4000, (half << 16) + 0xC000
            assert undecided_full_tiles(v, lo, hi).size == n // 1024
            seg = native.DeviceSegment(ctx, [int_col(v).native()])
            q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
            check_select(q, between(v, lo, hi), True, (n, half))
            q.run_count()
            assert q.count() == int(between(v, lo, hi).sum())
            q.close()
            seg.close()


def test_a_small_span_column_gets_no_plane(ctx):
    from immutable3_amd import native
    rng = np.random.default_rng(4)
    n = 33 * 1024 + 1
    v = rng.integers(0, 50_000, size=n).astype(np.int32)
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    b0 = seg.device_bytes
    for _ in range(2):
        q = native.DeviceQuery(ctx, seg, [0], range_sels(0, 10_000, 30_000))
        check_select(q, between(v, 10_000, 30_000), False, "small span")
        q.close()
    assert seg.device_bytes == b0
    seg.close()


def pair_columns(rng, n):
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    ids = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    ids[rng.integers(0, n, size=64)] = 0x00420000 + rng.integers(0, 1 << 16, size=64)  # rows on a boundary half
    return age, ids


@pytest.mark.parametrize("n", [2 * 1024 + 1, 64 * 1024 + 63])
def test_int8_and_int32_pair(ctx, n):
    """the I8 + H16 instance, as a bitmap run and count-only"""
    from immutable3_amd import native
    rng = np.random.default_rng(n)
    age, ids = pair_columns(rng, n)
    cols = [RawColumn(DENSE_TINYINT, 1, age, blocks_of(n, 1024)), int_col(ids)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    lo, hi = 0x00420000 + 0x1000, 2 ** 30 + 12345
    keep = (age > -20) & (age < 90) & between(ids, lo, hi)
    for used, sels in (([0, 1], [(0, GT, -20.0), (0, LT, 90.0)] + range_sels(1, lo, hi)), ([1, 0], range_sels(0, lo, hi) + [(1, GT, -20.0), (1, LT, 90.0)])):
        q = native.DeviceQuery(ctx, seg, used, sels)
        check_select(q, keep, True, (n, used))
        q.run_count()
        assert q.count() == int(keep.sum()) and q.plan()["hi16_plane"]
        q.close()
    seg.close()


def test_count_only_runs(ctx):
    from immutable3_amd import native, synth
    n = 40 * 1024 + 777
    v = synth.uniform_int30(6, n)
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    for lo, hi in ((2 ** 28 + 1, 3 * 2 ** 28 - 1), (2 ** 29 + 77, 2 ** 29 + 0x20000)):
        q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
        q.run_count()  # (the first run of the handle: no bitmap has ever been stored)
        assert q.count() == int(between(v, lo, hi).sum()) and q.plan()["hi16_plane"]
        assert undecided_full_tiles(v, lo, hi).size > 0
        q.close()
    seg.close()


def test_chains_and_into_earlier_words(ctx):
    """A 4-byte string match beside the int32 range (the string pass ANDs into the plane pass's words), and four int32 ranges: three go
    through one int32 launch and the fourth, alone, scans its plane and ANDs into that launch's words."""
    from immutable3_amd import native, synth
    n = 48 * 1024 + 63
    rng = np.random.default_rng(7)
    v = synth.uniform_int30(7, n)
    names = np.array([list(b"anna"), list(b"bert"), list(b"cleo")], np.uint8)[rng.integers(0, 3, size=n)]
    cols = [int_col(v), RawColumn(DENSE_STRING, 4, names, blocks_of(n, 1024))]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    lo, hi = 2 ** 28 + 1, 3 * 2 ** 28 - 1
    keep = between(v, lo, hi) & (names == np.frombuffer(b"bert", np.uint8)).all(axis=1)
    q = native.DeviceQuery(ctx, seg, [0, 1], range_sels(0, lo, hi) + [(1, MATCH, [b"bert"])])
    check_select(q, keep, True, "string beside the range")
    q.close()
    seg.close()
    four = [synth.uniform_int30(70 + k, n) for k in range(4)]
    seg = native.DeviceSegment(ctx, [int_col(x).native() for x in four])
    sels, keep = [], np.ones(n, bool)
    for k, x in enumerate(four):
        lo_k, hi_k = 2 ** 26 + 1000 * k + 1, 2 ** 30 - 2 ** 26 - 17 * k
        sels += range_sels(k, lo_k, hi_k)
        keep &= between(x, lo_k, hi_k)
    q = native.DeviceQuery(ctx, seg, [0, 1, 2, 3], sels)
    check_select(q, keep, True, "four int32 ranges")
    q.close()
    seg.close()


def test_projection_and_limit_keep_their_rows(ctx):
    """the same range with a projection of the filtered column (whatever plan the projection takes) and with a limit (chunks of a limit
    scan read the column itself): the rows are the ones numpy selects"""
    from immutable3_amd import native, synth
    n = 64 * 1024 + 777
    v = synth.uniform_int30(8, n)
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    lo, hi = 2 ** 28 + 1, 3 * 2 ** 28 - 1
    rows = np.flatnonzero(between(v, lo, hi))
    q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi), [0])
    q.run()
    idx, vals = q.fetch_rows()
    assert idx.tolist() == rows.tolist() and vals[0].view("<i4").reshape(-1).tolist() == v[rows].tolist()
    assert q.count() == rows.size and q.bitmap()[: (n + 63) // 64].tolist() == words_of(between(v, lo, hi)).tolist()
    q.close()
    b0 = seg.device_bytes
    q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi), [0], 10)
    q.run()
    assert not q.plan()["hi16_plane"]
    idx, vals = q.fetch_rows()
    assert idx.tolist() == rows[:10].tolist() and vals[0].view("<i4").reshape(-1).tolist() == v[rows[:10]].tolist()
    assert q.count() == rows.size
    q.close()
    assert seg.device_bytes == b0
    seg.close()


def test_a_limit_query_alone_makes_no_plane(ctx):
    from immutable3_amd import native, synth
    n = 16 * 1024
    v = synth.uniform_int30(9, n)
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    b0 = seg.device_bytes
    q = native.DeviceQuery(ctx, seg, [0], range_sels(0, 2 ** 28, 2 ** 29), [0], 5)
    q.run()
    idx, _ = q.fetch_rows()
    assert idx.tolist() == np.flatnonzero(between(v, 2 ** 28, 2 ** 29))[:5].tolist() and not q.plan()["hi16_plane"]
    assert seg.device_bytes == b0
    q.close()
    seg.close()


def test_async_segment_query_created_and_run_at_once(ctx):
    from immutable3_amd import native, synth
    n = 64 * 1024 + 1
    v = synth.uniform_int30(10, n)
    col = int_col(v)
    seg = native.DeviceSegment(ctx, [col.native()], async_copy=True)
    lo, hi = 2 ** 28 + 1, 3 * 2 ** 28 - 1
    q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
    check_select(q, between(v, lo, hi), True, "async")
    seg.wait()
    q.close()
    seg.close()


def test_captured_graph_replays(ctx):
    from immutable3_amd import native, synth
    n = 32 * 1024 + 63
    v = synth.uniform_int30(11, n)
    seg = native.DeviceSegment(ctx, [int_col(v).native()])
    lo, hi = 2 ** 28 + 1, 3 * 2 ** 28 - 1
    keep = between(v, lo, hi)
    q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
    with ctx.capture() as cap:
        q.run()
    for _ in range(3):
        cap.graph.launch()
        assert q.count() == int(keep.sum()) and q.bitmap()[: (n + 63) // 64].tolist() == words_of(keep).tolist()
        assert q.plan()["hi16_plane"]
    cap.graph.close()
    q.close()
    seg.close()


def test_segment_bytes_grow_once(ctx):
    from immutable3_amd import native, synth
    n = 10 * 1024 + 777
    v = synth.uniform_int30(12, n)
    age = np.zeros(n, np.int8)
    seg = native.DeviceSegment(ctx, [int_col(v).native(), RawColumn(DENSE_TINYINT, 1, age, blocks_of(n, 1024)).native()])
    b0 = seg.device_bytes
    q0 = native.DeviceQuery(ctx, seg, [1], [(0, GT, -1.0)])  # no int32 predicate: no plane
    assert seg.device_bytes == b0
    qs = [native.DeviceQuery(ctx, seg, [0], range_sels(0, 2 ** 20 * (k + 1), 2 ** 29 + k)) for k in range(4)]
    assert seg.device_bytes == b0 + 2 * n + PAD
    qs.append(native.DeviceQuery(ctx, seg, [1, 0], [(0, GT, -1.0)] + range_sels(1, 5, 2 ** 29)))
    assert seg.device_bytes == b0 + 2 * n + PAD
    for q in qs:
        q.run()
        assert q.plan()["hi16_plane"]
    for q in qs + [q0]:
        q.close()
    seg.close()


FUZZ_SEED, FUZZ_CASES = 20261, 200


def fuzz_case(rng):
    n = int(rng.integers(1, 70_001))
    dist = int(rng.integers(0, 4))
    if dist == 0:      # uniform
        v = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    elif dist == 1:    # sorted
        v = np.sort(rng.integers(-2 ** 27, 2 ** 27, size=n, dtype=np.int64))
    elif dist == 2:    # clustered: a few halves hold most rows
        centres = rng.integers(-2 ** 30, 2 ** 30, size=4, dtype=np.int64)
        v = centres[rng.integers(0, 4, size=n)] + rng.integers(-40_000, 40_000, size=n)
        far = rng.integers(0, n, size=max(1, n // 50))
        v[far] = rng.integers(-2 ** 31, 2 ** 31, size=far.size, dtype=np.int64)
    else:              # few distinct halves: no plane
        v = rng.integers(0, 1 << 16, size=n) + (rng.integers(0, 8, size=n) << 16) - (3 << 16)
    v = v.astype(np.int32)
    pick = lambda: int(np.clip(int(v[rng.integers(0, n)]) + int(rng.integers(-70_000, 70_001)), -2 ** 31 + 1, 2 ** 31 - 2))
    lo, hi = pick(), pick()
    if rng.integers(0, 8):  # (mostly a proper interval; sometimes lo > hi: nothing selected)
        lo, hi = min(lo, hi), max(lo, hi)
    return dist, v, lo, hi


def expects_plane(v, lo, hi):
    h = v.astype(np.int64) >> 16
    return lo <= hi and int(h.max()) - int(h.min()) + 1 >= 64


def test_the_fuzz_seed_meets_its_conditions_on_the_host():
    """the seed was chosen from the host logic alone: at least half the cases scan a plane, at least 20 have a tile to refine"""
    rng = np.random.default_rng(FUZZ_SEED)
    planes = refines = 0
    for _ in range(FUZZ_CASES):
        _, v, lo, hi = fuzz_case(rng)
        if expects_plane(v, lo, hi):
            planes += 1
            refines += undecided_full_tiles(v, lo, hi).size > 0
    assert planes >= FUZZ_CASES // 2 and refines >= 20, (planes, refines)


def test_fuzz(ctx):
    from immutable3_amd import native
    rng = np.random.default_rng(FUZZ_SEED)
    planes = refines = 0
    for case in range(FUZZ_CASES):
        dist, v, lo, hi = fuzz_case(rng)
        what = ("seed", FUZZ_SEED, "case", case, "dist", dist, "n", v.size, "lo", lo, "hi", hi)
        keep = between(v, lo, hi)
        seg = native.DeviceSegment(ctx, [int_col(v).native()])
        q = native.DeviceQuery(ctx, seg, [0], range_sels(0, lo, hi))
        q.run()
        want = words_of(keep)
        got = q.bitmap()
        assert q.count() == int(keep.sum()), what
        assert got[: want.size].tolist() == want.tolist() and not got[want.size:].any(), what
        ran = q.plan()["hi16_plane"]
        assert ran == expects_plane(v, lo, hi), what
        planes += ran
        refines += ran and undecided_full_tiles(v, lo, hi).size > 0
        q.close()
        seg.close()
    assert planes >= FUZZ_CASES // 2 and refines >= 20, (planes, refines)
