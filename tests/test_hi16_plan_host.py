"""CPU suite for the 16-bit high-half plane of DENSE_INT columns (csrc/imm3_hi16_plan.{h,cpp}): what a closed int32 interval becomes
over the halves v >> 16 -- a row whose half lies outside the boundary halves fails, one strictly inside passes, one ON a boundary half
that does not decide itself needs its full value -- and the rule that says which tile pass scans the plane.  No device is touched."""
import numpy as np
import pytest

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def native():
    from immutable3_amd import native as n
    from immutable3_amd.build import build_native
    build_native()
    return n


def classify(bounds, halves):
    """numpy restatement of hi16_class over an array of halves (int64 in -32768 .. 32767)"""
    pf, pn, cf, cn = bounds
    h = halves & 0xFFFF
    possible = ((h - pf) & 0xFFFF) < pn
    certain = ((h - cf) & 0xFFFF) < cn
    return np.where(~possible, 0, np.where(certain, 1, 2))


EDGE_VALUES = sorted({INT_MIN, INT_MIN + 1, INT_MIN + 0xFFFF, INT_MIN + 0x10000, -0x10001, -0x10000, -0xFFFF, -2, -1, 0, 1, 0x7FFF, 0xFFFF,
                      0x10000, 0x10001, 0x1FFFF, 0x20000, 2 ** 28, 2 ** 28 + 1, 3 * 2 ** 28 - 1, INT_MAX - 0x10000, INT_MAX - 0xFFFF, INT_MAX - 1,
                      INT_MAX})


def intervals(rng):
    out = [(lo, hi) for lo in EDGE_VALUES for hi in EDGE_VALUES]                                    # lo > hi among them
    for base in (0, -0x30000, 0x7FFF0000 - 0x10000, INT_MIN):
        for dlo in (0, 1, 0x7FFF, 0xFFFF):
            for dhi in (0, 1, 0x7FFF, 0xFFFF):
                out.append((base + dlo, base + dhi))                                                # both boundaries in one half
                out.append((base + dlo, base + 0x10000 + dhi))                                      # adjacent halves
                out.append((base + dlo, base + 0x20000 + dhi))
    for _ in range(300):
        lo, hi = (int(x) for x in rng.integers(INT_MIN, INT_MAX + 1, size=2))
        out.append((lo, hi))
        out.append((lo, min(INT_MAX, lo + int(rng.integers(0, 1 << 18)))))
    return [(lo, hi) for lo, hi in out if INT_MIN <= lo <= INT_MAX and INT_MIN <= hi <= INT_MAX]


def test_the_classification_never_contradicts_the_interval(native):
    rng = np.random.default_rng(16)
    for lo, hi in intervals(rng):
        b = native.plan_hi16_bounds(lo, hi)
        near = np.array([x + d for x in (lo, hi) for d in (-0x10001, -0x10000, -0xFFFF, -1, 0, 1, 0xFFFF, 0x10000, 0x10001)], np.int64)
        v = np.concatenate([near, np.array(EDGE_VALUES, np.int64), rng.integers(INT_MIN, INT_MAX + 1, size=200)])
        v = v[(v >= INT_MIN) & (v <= INT_MAX)]
        half = v >> 16
        cls = classify(b, half)
        truth = (v >= lo) & (v <= hi)
        assert not (cls[truth] == 0).any(), (lo, hi, v[truth & (cls == 0)][:3])
        assert not (cls[~truth] == 1).any(), (lo, hi, v[~truth & (cls == 1)][:3])
        # undecided only on a boundary half that does not decide itself
        lo_h, hi_h = lo >> 16, hi >> 16
        lo_open, hi_open = (lo & 0xFFFF) != 0, (hi & 0xFFFF) != 0xFFFF
        und = cls == 2
        if lo <= hi:
            allowed = ((half == lo_h) & lo_open) | ((half == hi_h) & hi_open)
            assert not (und & ~allowed).any(), (lo, hi, v[und & ~allowed][:3])
            assert (cls[allowed] == 2).all(), (lo, hi)
        else:
            assert (cls == 0).all(), (lo, hi)
        for x, c in zip(v[:6].tolist(), cls[:6].tolist()):                                         # the library's own classifier agrees
            assert native.plan_hi16_class(lo, hi, x >> 16) == c, (lo, hi, x)


def test_every_half_of_small_windows(native):
    """All 65 536 halves against intervals whose windows wrap, touch the ends of the int32 range, or are empty."""
    all_halves = np.arange(-32768, 32768, dtype=np.int64)
    for lo, hi in [(INT_MIN, INT_MAX), (INT_MIN, INT_MIN), (INT_MAX, INT_MAX), (-1, 0), (-0x10000, 0xFFFF), (-0x8000, 0x8000), (0x10000, 0x1FFFF),
                   (0x10001, 0x1FFFE), (4, 5), (INT_MAX - 5, INT_MAX), (INT_MIN, INT_MIN + 5), (2 ** 28 + 1, 3 * 2 ** 28 - 1)]:
        cls = classify(native.plan_hi16_bounds(lo, hi), all_halves)
        lo_v, hi_v = all_halves << 16, (all_halves << 16) + 0xFFFF                                   # the values a half holds
        must_fail = (hi_v < lo) | (lo_v > hi)
        must_pass = (lo_v >= lo) & (hi_v <= hi)
        assert (cls[must_fail] == 0).all() and (cls[must_pass] == 1).all() and (cls[~must_fail & ~must_pass] == 2).all(), (lo, hi)
    assert native.plan_hi16_class(0, 10, 40000) == -1 and native.plan_hi16_class(0, 10, -32769) == -1


def test_which_columns_keep_a_plane(native):
    assert native.HI16_MIN_SPAN == 64
    assert not native.plan_hi16_span_ok(0, 0)                  # values in [0, 65536)
    assert not native.plan_hi16_span_ok(0, 62) and native.plan_hi16_span_ok(0, 63)
    assert native.plan_hi16_span_ok(-32768, 32767) and native.plan_hi16_span_ok(-32, 31) and not native.plan_hi16_span_ok(-31, 31)
    assert not native.plan_hi16_span_ok(32767, -32768)         # (an empty column: what the build's reduction starts from)


def test_the_eligibility_rule_case_by_case(native):
    ok = dict(dense_int=True, has_plane=True)
    e = native.plan_hi16_eligible
    assert e(1, 0, 0, **ok) and e(1, 1, 0, **ok)                                                   # the two instances
    for n_i32, n_i8, n_s2 in ((0, 1, 0), (2, 0, 0), (1, 2, 0), (1, 0, 1), (1, 1, 1), (2, 1, 0), (0, 0, 0)):
        assert not e(n_i32, n_i8, n_s2, **ok), (n_i32, n_i8, n_s2)
    for fact in ("table", "tree", "ragged", "has_list", "stages", "chunked", "pinned_i32"):
        assert not e(1, 0, 0, **ok, **{fact: True}), fact
        assert not e(1, 1, 0, **ok, **{fact: True}), fact
    assert not e(1, 0, 0, dense_int=True) and not e(1, 0, 0, has_plane=True)                        # no plane / a PFOR or snappy column
