"""GPU suite: IMM3_STR_RANGE -- a closed byte-order range on a string column -- over ONE segment: k_filter_str_range
(csrc/imm3_strmatch.hip) under the default plan and the word-at-a-time kernel's range form under tuning variant 1.  Expected bitmaps
and counts are tests/str_range_util.py's (rows compared as Python bytes); an equality is also held against Match through the C oracle."""
import numpy as np
import pytest

from conftest import DENSE_INT, DENSE_STRING, DENSE_TINYINT, GT, LT, MATCH, RawColumn, blocks_of
from immutable3_amd import native
import str_range_util as U

pytestmark = pytest.mark.gpu
STR_RANGE = native.STR_RANGE
TV_GENERIC_ONLY = 1
WIDTHS = [4, 8, 12, 16, 20, 24, 32, 256]      # every instance of the string pass
GENERIC_WIDTHS = [2, 3, 5]                      # the word-at-a-time kernel only
TAIL_WIDTHS = [20, 24, 32, 256]
# test_gpu_str_rows.py's SHAPES
SHAPES = [(0, []), (1, [1]), (63, [63]), (64, [64]), (65, [65]), (1023, [1023]), (1024, [1024]), (1025, blocks_of(1025, 1024)),
          (2 * 1024 + 1, [1024, 1024, 1]), (4 * 64 + 5, [64, 128, 64, 5])]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def select_both_ways(ctx, seg, used, sels, expr=None):
    """(words, count) of run_select under the default plan and under the word-at-a-time kernel"""
    out = []
    for variant in (0, TV_GENERIC_ONLY):
        ctx.set_tuning(variant, 0)
        try:
            q = native.DeviceQuery(ctx, seg, used, sels, expr=expr)
            q.run_select()
            out.append((q.bitmap(), q.count()))
            q.close()
        finally:
            ctx.set_tuning(0, 0)
    return out


def check(ctx, seg, used, sels, mask, block_rows, what, expr=None):
    want = U.bitmap_words(mask, block_rows)
    for (w, c), plan in zip(select_both_ways(ctx, seg, used, sels, expr), ("default", "generic")):
        assert c == int(mask.sum()), (what, plan, c, int(mask.sum()))
        assert w.tolist() == want.tolist(), (what, plan)


def bounds_for(rng, width):
    """(lo', hi') of full width with lo' < hi', bytes on both sides of 0x80 so that a signed compare orders rows wrongly"""
    lo = bytes([0x41]) + bytes(rng.integers(0x30, 0xD0, size=width - 1).astype(np.uint8))
    hi = bytes([0xC1]) + bytes(rng.integers(0x30, 0xD0, size=width - 1).astype(np.uint8))
    return lo, hi


def pool_for(rng, width, bounds):
    rows = []
    for b in bounds:
        rows += U.neighbours(b, width)
    for _ in range(40):
        rows.append(bytes(rng.integers(0, 256, size=width).astype(np.uint8)))
    return U.rows_array(rows, width)


def ranges_for(width, lo, hi):
    """(lo, hi, what): the full-width pair, short bounds, a prefix, everything, nothing, an equality, and the carry bounds"""
    out = [(lo, hi, "full width"), (lo[:1], hi[:1], "one byte"), (lo[: width // 2], hi[: width - 1], "short"), (lo[: max(1, width // 2)], lo[: max(1, width // 2)], "prefix"),
           (b"", b"", "every row"), (hi, lo, "lo' > hi'"), (lo, lo, "lo' == hi'"), (lo, b"", "from lo on"), (b"", hi, "up to hi")]
    for cb in U.carry_bounds(width):
        out += [(cb, b"", "from a carry bound on"), (b"", cb, "up to a carry bound"), (cb, cb, "a carry bound alone")]
    return out


@pytest.mark.parametrize("width", WIDTHS + GENERIC_WIDTHS)
def test_byte_order_every_shape(ctx, oracle, width):
    """rows that differ from a bound in one byte alone (0x7F / 0x80, 0x00 / 0xFF) at every byte position, the bounds themselves (in),
    their predecessors and successors with carries (out), short bounds, the special ranges -- on every shape"""
    rng = np.random.default_rng(4000 + width)
    lo, hi = bounds_for(rng, width)
    pool = pool_for(rng, width, [lo, hi] + U.carry_bounds(width))
    ranges = ranges_for(width, lo, hi)
    for n, block_rows in SHAPES:
        v = pool[rng.integers(0, pool.shape[0], size=n)].reshape(n, width).copy()
        if n >= pool.shape[0]:
            v[: pool.shape[0]] = pool                     # every neighbour of every bound is a row
        elif n:
            v[:] = pool[rng.permutation(pool.shape[0])[:n]]
        col = RawColumn(DENSE_STRING, width, v, block_rows)
        seg = native.DeviceSegment(ctx, [col.native()])
        for (a, b, what) in ranges:
            mask = U.in_range(v, a, b)
            check(ctx, seg, [0], [(0, STR_RANGE, (a, b))], mask, block_rows, (width, n, what))
            if what == "lo' > hi'":
                assert not mask.any()
            if what == "every row":
                assert mask.all()
            if what == "lo' == hi'" and n:                 # an equality: also Match, through the oracle
                ow, oc = oracle.scan_select([col.ocol()], [(0, MATCH, [a])], 1024, 1)
                assert oc == int(mask.sum()) and ow.tolist() == U.bitmap_words(mask, block_rows).tolist()
        seg.close()
    # the rows next to the bounds are where they belong
    plo, phi = U.pad(lo, hi, width)
    near = U.rows_array([plo, phi, U.predecessor(plo), U.successor(phi)], width)
    assert U.in_range(near, lo, hi).tolist() == [True, True, False, False]


@pytest.mark.parametrize("width", TAIL_WIDTHS)
def test_tail_ties(ctx, width):
    """tiles of rows that share their first 16 bytes with a bound and lie above or below it later: a tile that is all ties with lo', ties
    with hi', bounds that share their prefix (rows tie with both), rows that differ from a bound in the last byte only"""
    rng = np.random.default_rng(5000 + width)
    lo, hi = bounds_for(rng, width)
    shared_hi = lo[:16] + bytes([0xE0]) + hi[17:]        # shares lo's first 16 bytes, above it at byte 16
    n, block_rows = 3 * 1024 + 1, [1024, 1024, 1024, 1]

    def tied(with_bound, count):
        rows = []
        for k in range(count):
            r = bytearray(with_bound)
            if k % 4 == 0:
                r[-1] = (r[-1] + (1 if k % 8 else -1)) & 0xFF       # the last byte only
            elif k % 4 == 1:
                pass                                                 # the bound itself
            else:
                at = 16 + int(rng.integers(0, width - 16))
                r[at:] = bytes(rng.integers(0, 256, size=width - at).astype(np.uint8))
            rows.append(bytes(r))
        return U.rows_array(rows, width)

    v = rng.integers(0, 256, size=(n, width)).astype(np.uint8)
    v[1024:2048] = tied(lo, 1024)                        # one tile is all ties with lo'
    v[2048:2048 + 300] = tied(hi, 300)
    v[2048 + 300:2048 + 600] = tied(shared_hi, 300)
    v[[3, 1023, 3072]] = np.frombuffer(lo, dtype=np.uint8)
    col = RawColumn(DENSE_STRING, width, v, block_rows)
    seg = native.DeviceSegment(ctx, [col.native()])
    last_lo = lo[:-1] + bytes([(lo[-1] + 1) & 0xFF]) if lo[-1] != 0xFF else lo
    for (a, b, what) in [(lo, hi, "ties with lo' and hi'"), (lo, shared_hi, "bounds share their prefix"), (lo, lo, "equality"), (lo, last_lo, "last byte"),
                         (lo[:16], lo[:16], "the prefix of all ties"), (hi, b"", "from hi on"), (b"", lo, "up to lo"), (shared_hi, hi, "from the shared bound")]:
        mask = U.in_range(v, a, b)
        check(ctx, seg, [0], [(0, STR_RANGE, (a, b))], mask, block_rows, (width, what))
    assert U.in_range(v, lo[:16], lo[:16])[1024:2048].all() and 0 < U.in_range(v, lo, hi)[1024:2048].sum() < 1024
    seg.close()


def mixed_segment(ctx, rng, n, block_rows, w_a=16, w_b=8):
    lo, hi = bounds_for(rng, w_a)
    pool_a = pool_for(rng, w_a, [lo, hi])
    pool_b = rng.integers(97, 101, size=(12, w_b)).astype(np.uint8)
    ids = rng.integers(-50, 50, size=n).astype(np.int32)
    age = rng.integers(-128, 128, size=n).astype(np.int8)
    a = pool_a[rng.integers(0, pool_a.shape[0], size=n)].copy()
    b = pool_b[rng.integers(0, 12, size=n)].copy()
    cols = [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows),
            RawColumn(DENSE_STRING, w_a, a, block_rows), RawColumn(DENSE_STRING, w_b, b, block_rows)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    return seg, cols, (ids, age, a, b), (lo, hi, pool_a, pool_b)


@pytest.mark.parametrize("n,block_rows", [(3 * 1024 + 700, [1024] * 3 + [700]), (4 * 64 + 5, [64, 128, 64, 5])])
def test_composition(ctx, oracle, n, block_rows):
    """a range beside int32 and int8 predicates, beside a Match on a second string column, two ranges on one column, a range and a
    Match on one column, an AND-only program through the _expr entry point, and the refusal of OR / NOT"""
    rng = np.random.default_rng(n)
    seg, cols, (ids, age, a, b), (lo, hi, pool_a, pool_b) = mixed_segment(ctx, rng, n, block_rows)
    ra = U.in_range(a, lo, hi)
    num = (ids > -20) & (ids < 40) & (age > -100)
    check(ctx, seg, [2, 0, 1], [(0, STR_RANGE, (lo, hi)), (1, GT, -20.0), (1, LT, 40.0), (2, GT, -100.0)], ra & num, block_rows, "range first")
    check(ctx, seg, [0, 1, 2], [(0, GT, -20.0), (0, LT, 40.0), (1, GT, -100.0), (2, STR_RANGE, (lo, hi))], ra & num, block_rows, "range last")
    lb = [bytes(pool_b[0]), bytes(pool_b[5])]
    mb = (b == pool_b[0]).all(1) | (b == pool_b[5]).all(1)
    check(ctx, seg, [2, 3], [(0, STR_RANGE, (lo, hi)), (1, MATCH, lb)], ra & mb, block_rows, "beside a Match")
    check(ctx, seg, [3, 2], [(0, STR_RANGE, (b"a", b"b")), (1, STR_RANGE, (lo, hi))], ra & U.in_range(b, b"a", b"b"), block_rows, "two string passes")
    # two ranges on one column: their intersection
    mid = bytes([0x80]) * 3
    check(ctx, seg, [2], [(0, STR_RANGE, (lo, hi)), (0, STR_RANGE, (mid, b""))], U.in_range(a, mid, hi), block_rows, "two ranges")
    check(ctx, seg, [2], [(0, STR_RANGE, (lo, mid)), (0, STR_RANGE, (hi, b""))], np.zeros(n, bool), block_rows, "two ranges that do not meet")
    # a range and a Match on one column: the IN-list's values inside the range -- an ordinary Match (same plan, same result)
    inside = [bytes(r) for r in pool_a if U.pad(lo, hi, 16)[0] <= bytes(r) <= U.pad(lo, hi, 16)[1]][:3]
    outside = [bytes(r) for r in pool_a if bytes(r) > U.pad(lo, hi, 16)[1]][:3]
    assert inside and outside
    sels = [(0, MATCH, inside + outside), (0, STR_RANGE, (lo, hi))]
    ow, oc = oracle.scan_select([cols[2].ocol()], [(0, MATCH, inside)], 1024, 1)
    mask = np.array([bytes(r) in set(inside) for r in a], dtype=bool)
    assert oc == int(mask.sum()) and ow.tolist() == U.bitmap_words(mask, block_rows).tolist()
    check(ctx, seg, [2], sels, mask, block_rows, "range and Match")
    check(ctx, seg, [2], sels[::-1], mask, block_rows, "Match and range")
    q, qm = native.DeviceQuery(ctx, seg, [2], sels, [0]), native.DeviceQuery(ctx, seg, [2], [(0, MATCH, inside)], [0])
    assert q.plan() == qm.plan()
    q.close()
    qm.close()
    # an AND-only program is the flat list
    check(ctx, seg, [2, 0], [(0, STR_RANGE, (lo, hi)), (1, GT, -20.0)], ra & (ids > -20), block_rows, "AND program", expr=[0, 1, native.EXPR_AND])
    for prog in ([0, 1, native.EXPR_OR], [0, native.EXPR_NOT], [0, 1, native.EXPR_AND, native.EXPR_NOT]):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, [2, 0], [(0, STR_RANGE, (lo, hi)), (1, GT, -20.0)], expr=prog)
        assert e.value.code == native.ERR_ARG and "IMM3_STR_RANGE" in e.value.msg and not e.value.msg.startswith(native.TABLE_TREE_REFUSED)
    seg.close()


def test_leaf_checks(ctx):
    rng = np.random.default_rng(9)
    seg, cols, _, (lo, hi, _, _) = mixed_segment(ctx, rng, 100, [100])
    for operand, word in (([lo], "n_match"), ([lo, hi, hi], "n_match"), ([], "n_match"), ([lo + b"x", hi], "longer"), ([lo, hi + b"xy"], "longer")):
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, [2], [(0, STR_RANGE, operand)])
        assert e.value.code == native.ERR_ARG and word in e.value.msg, e.value.msg
    for used in ([0], [1]):                                 # int32 / int8 columns
        with pytest.raises(native.Imm3Error) as e:
            native.DeviceQuery(ctx, seg, used, [(0, STR_RANGE, (b"a", b"b"))])
        assert e.value.code == native.ERR_UNSUPPORTED_VECTOR and e.value.msg == "Unsupported column vector"
    seg.close()
    empty = native.DeviceSegment(ctx, [RawColumn(DENSE_INT, 4, np.zeros(0, np.int32), []).native()])
    q = native.DeviceQuery(ctx, empty, [0], [(0, STR_RANGE, (b"a", b"b"))])   # no batch: no vector to be of the wrong type
    q.close()
    empty.close()


@pytest.mark.parametrize("width", [16, 32])
def test_behind_the_select(ctx, width):
    """projection with limit 0, 7 and all; group-by count + max; set_order by the string column"""
    rng = np.random.default_rng(6000 + width)
    n, block_rows = 5 * 1024 + 321, [1024] * 5 + [321]
    lo, hi = bounds_for(rng, width)
    pool = pool_for(rng, width, [lo, hi])
    ids = rng.integers(-50, 50, size=n).astype(np.int32)
    age = rng.integers(-4, 4, size=n).astype(np.int8)
    s = pool[rng.integers(0, pool.shape[0], size=n)].copy()
    cols = [RawColumn(DENSE_INT, 4, ids, block_rows), RawColumn(DENSE_TINYINT, 1, age, block_rows), RawColumn(DENSE_STRING, width, s, block_rows)]
    seg = native.DeviceSegment(ctx, [c.native() for c in cols])
    used, sels = [2, 0, 1], [(0, STR_RANGE, (lo, hi)), (2, GT, -3.0)]
    mask = U.in_range(s, lo, hi) & (age > -3)
    keep = np.flatnonzero(mask)
    assert 0 < keep.size < n
    for limit in (0, 7, keep.size):
        q = native.DeviceQuery(ctx, seg, used, sels, [1, 0, 2], limit, 1024)
        q.run()
        idx, vals = q.fetch_rows()
        assert q.count() == keep.size and q.bitmap().tolist() == U.bitmap_words(mask, block_rows).tolist()
        q.close()
        want = keep[:limit] if limit else keep
        assert idx.tolist() == want.tolist()
        assert vals[0].view("<i4").reshape(-1).tolist() == ids[want].tolist() and vals[1].tobytes() == s[want].tobytes()
        assert vals[2].view(np.int8).reshape(-1).tolist() == age[want].tolist()
    q = native.DeviceQuery(ctx, seg, used, sels, (), 0, 1024, group_cols=[2], aggs=[(native.AGG_COUNT, 1), (native.AGG_MAX, 1)])
    q.run()
    keys, first, counts, gvals = q.fetch_groups()
    q.close()
    want = {}
    for r in keep:
        k = int(age[r])
        c, m = want.get(k, (0, -1 << 40))
        want[k] = (c + 1, max(m, int(ids[r])))
    key_of = lambda k: int.from_bytes(bytes([int(k) & 0xFF]), "little", signed=True)
    got = {key_of(k): (int(c), int(v[1])) for k, c, v in zip(keys, counts, gvals)}
    assert got == want and [key_of(k) for k in keys] == list(dict.fromkeys(int(x) for x in age[keep]))
    if width <= 16:                                        # (an order key is at most 16 bytes wide)
        for desc, limit in ((False, 0), (True, 5)):
            q = native.DeviceQuery(ctx, seg, used, sels, [0, 1], 0, 1024)
            q.set_order([(0, desc)], limit)
            q.run()
            idx, vals = q.fetch_rows()
            q.close()
            order = sorted(keep.tolist(), key=lambda r: (tuple(255 - x for x in s[r]) if desc else tuple(s[r]), r))
            order = order[:limit] if limit else order
            assert idx.tolist() == order and vals[0].tobytes() == s[order].tobytes()
    seg.close()
