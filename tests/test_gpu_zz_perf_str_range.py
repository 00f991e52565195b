"""GPU suite, with the other assertions on a TIME (`zz`): k_filter_str_range against two launches this change does not touch, over 16 M
rows of a 16-byte column.  Yardstick 1 is Match with two values on the same column (k_filter_str_rows): both kernels read the same
256 MB, so a range or a prefix must come within 1.25 x of it -- the bound the project's perf tests give HIP-event noise on launches
of this length.  Yardstick 2 is the same range under the word-at-a-time kernel (tuning variant 1), which the string pass has to beat.
All launches are timed interleaved, round after round, by an event pair around ten back-to-back select runs; medians over the rounds.
A range whose bounds tie with a tenth of the rows is reported, not asserted (at 16 bytes a tie is decided without a tail)."""
import numpy as np
import pytest

from immutable3_amd import native
import str_range_util as U

pytestmark = pytest.mark.gpu
TV_GENERIC_ONLY = 1
N, WIDTH, ROUNDS, RUNS = 16_000_000, 16, 7, 10


def runs_us(ctx, q, runs=RUNS):
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    q.run_select()
    ctx.sync()
    a.record(stream)
    for _ in range(runs):
        q.run_select()
    b.record(stream)
    ctx.sync()
    return a.elapsed_time(b) / runs * 1e3


def test_range_and_prefix_against_match_and_the_generic_kernel():
    rng = np.random.default_rng(16)
    v = rng.integers(0, 256, size=(N, WIDTH), dtype=np.uint8)
    tie = bytes(rng.integers(0x30, 0x70, size=WIDTH).astype(np.uint8))
    v[::10] = np.frombuffer(tie, dtype=np.uint8)                   # a tenth of the rows equal the tie case's lower bound
    offs = np.concatenate([np.arange(0, N, 1024, dtype=np.int64), [N]]) * WIDTH
    assert offs[-1] < 2 ** 31
    ctx = native.Context(0)
    seg = native.DeviceSegment(ctx, [(native.DENSE_STRING, WIDTH, v.reshape(-1), v.size, offs.astype(np.int32))])
    cases = {
        "match2": (0, (0, native.MATCH, [bytes(v[1]), bytes(v[2])])),
        "wide": (0, (0, native.STR_RANGE, (b"\x20", b"\xdf"))),
        "prefix": (0, (0, native.STR_RANGE, (b"\x41\x42", b"\x41\x42"))),
        "tie": (0, (0, native.STR_RANGE, (tie, b"\xdf"))),
        "wide generic": (TV_GENERIC_ONLY, (0, native.STR_RANGE, (b"\x20", b"\xdf"))),
        "prefix generic": (TV_GENERIC_ONLY, (0, native.STR_RANGE, (b"\x41\x42", b"\x41\x42"))),
    }
    first = v[:, 0]
    want = {"wide": int(((first >= 0x20) & (first <= 0xDF)).sum()), "prefix": int(((first == 0x41) & (v[:, 1] == 0x42)).sum())}
    times = {k: [] for k in cases}
    try:
        queries = {}
        for name, (variant, sel) in cases.items():
            ctx.set_tuning(variant, 0)
            q = native.DeviceQuery(ctx, seg, [0], [sel])
            q.run_select()
            if name.split()[0] in want:
                assert q.count() == want[name.split()[0]], name
            queries[name] = q
        sample = slice(0, 4096)
        assert queries["tie"].count() >= N // 10 and queries["tie"].bitmap()[:64].tolist() == U.bitmap_words(U.in_range(v[sample], tie, b"\xdf"), [1024] * 4).tolist()
        for _ in range(ROUNDS):                                    # interleaved: every round times every launch once
            for name, (variant, _) in cases.items():
                ctx.set_tuning(variant, 0)                         # (the chain is planned on every run)
                times[name].append(runs_us(ctx, queries[name]))
        for q in queries.values():
            q.close()
    finally:
        ctx.set_tuning(0, 0)
        seg.close()
        ctx.close()
    t = {k: float(np.median(x)) for k, x in times.items()}
    print("str_range perf, 16 M rows x 16 bytes, us per select run (median of %d rounds): " % ROUNDS + ", ".join(f"{k} {x:.1f}" for k, x in t.items()))
    print("ratios to match2: " + ", ".join(f"{k} {t[k] / t['match2']:.3f}" for k in ("wide", "prefix", "tie")) +
          f"; generic / string pass: wide {t['wide generic'] / t['wide']:.2f}, prefix {t['prefix generic'] / t['prefix']:.2f}")
    for k in ("wide", "prefix"):
        assert t[k] <= 1.25 * t["match2"], (k, t)
        assert t[k] < t[k + " generic"], (k, t)
