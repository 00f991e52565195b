"""CPU suite: the host-only units of a view of merged groups (imm3_comm_merge_groups_view; DESIGN.md section 21, "Views of merged
groups").  The plan -- tie width, refusal, the hash the ranks vote on -- through the diag call that needs no device
(imm3_merge_view_plan_json); the plan and the host view function (imm3_merge_view_host.cpp) alone under AddressSanitizer + UBSan in a
stand-alone program, tests/native/merge_view_asan.cpp: nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import pytest

from immutable3_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

C, MN, MX, S = native.AGG_COUNT, native.AGG_MIN, native.AGG_MAX, native.AGG_SUM
GCOL, AGG = native.GROUP_ORDER_GROUP_COL, native.GROUP_ORDER_AGG
# group by (int8, int32, 12-byte string); COUNT, SUM, MIN(int32), MAX(12-byte string)
SHAPE = dict(group_kinds=[1, 0, 2], group_widths=[1, 4, 12], agg_kinds=[C, S, MN, MX], agg_col_kinds=[0, 0, 0, 2], agg_col_widths=[4, 4, 4, 12])


def plan(largest, **view):
    return native.merge_view_plan(largest_segment_index=largest, **SHAPE, **view)


@pytest.mark.parametrize("largest,s", [(0, 0), (255, 1), (256, 2), (65535, 2), (65536, 3), (2 ** 24, 4), (2 ** 31 - 1, 4)])
def test_the_tie_takes_the_bytes_of_the_largest_segment_index(largest, s):
    p = plan(largest, order=[(AGG, 0, 1)])
    assert p["seg_bytes"] == s and p["user_bytes"] == 5 and p["key_bytes"] == 5 + s + 4
    assert plan(largest)["key_bytes"] == s + 4                                     # no order: first arrival as the whole key


def test_sixteen_key_bytes_are_accepted_and_seventeen_refused_with_the_prefix():
    assert plan(0, order=[(GCOL, 2, 0)])["key_bytes"] == 16                        # 12 + 0 + 4
    assert plan(0, order=[(AGG, 3, 1)])["key_bytes"] == 16                         # a 12-byte string MAX
    p = plan(255, order=[(AGG, 1, 0), (GCOL, 0, 0)])                               # SUM 8 + int8 1, one byte of segment, the row
    assert p["user_bytes"] == 9 and p["key_bytes"] == 9 + 1 + 4
    assert plan(65535, order=[(AGG, 0, 0), (AGG, 2, 0), (GCOL, 0, 0)])["key_bytes"] == 16      # 10 + 2 + 4
    for largest, order in ((1, [(GCOL, 2, 0)]), (255, [(AGG, 3, 0)]), (65536, [(AGG, 0, 0), (AGG, 2, 0), (GCOL, 0, 0)]), (256, [(AGG, 1, 0), (GCOL, 1, 0)])):
        with pytest.raises(native.Imm3Error) as e:
            plan(largest, order=order)
        assert e.value.code == native.ERR_ARG and e.value.msg.startswith(native.MERGE_VIEW_REFUSED), e.value.msg
    # a bad key or leaf is a plain argument error, never the refusal
    for view in (dict(order=[(GCOL, 3, 0)]), dict(order=[(AGG, 1, 0), (AGG, 0, 0)]), dict(leaves=[(3, 0, native.GT, 0)], prog=[0]),
                 dict(leaves=[(0, 1, native.GT, 0)], prog=[0]), dict(leaves=[(1, 0, native.GT, 0)], prog=[0, 0])):
        with pytest.raises(native.Imm3Error) as e:
            plan(0, **view)
        assert e.value.code == native.ERR_ARG and not e.value.msg.startswith(native.MERGE_VIEW_REFUSED), (view, e.value.msg)


def test_the_hash_tells_views_apart_and_ignores_the_tie():
    base = dict(order=[(AGG, 1, 1), (GCOL, 0, 0)], leaves=[(1, 0, native.GT, 1000), (native.GROUP_FILTER_COUNT, 0, native.LT, 9)], prog=[0, 1, native.EXPR_AND], limit=10)
    h = plan(3, **base)["hash"]
    assert len(h) == 16 and plan(3, **base)["hash"] == h and plan(300, **base)["hash"] == h
    others = [dict(base, order=[(AGG, 1, 0), (GCOL, 0, 0)]),                                                            # one descending flag
              dict(base, leaves=[(1, 0, native.GT, 1001), base["leaves"][1]]),                                           # one threshold
              dict(base, limit=11), dict(base, limit=0),                                                                 # the limit
              dict(base, prog=[0, 1, native.EXPR_OR]), dict(base, order=[(GCOL, 0, 0), (AGG, 1, 1)])]
    hashes = [plan(3, **v)["hash"] for v in others]
    assert h not in hashes and len(set(hashes)) == len(hashes), hashes
    assert plan(3, **dict(base, limit=-4))["hash"] == plan(3, **dict(base, limit=0))["hash"]   # <= 0: no limit


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_and_host_view_under_asan_ubsan(tmp_path):
    """A stand-alone program (its own main) linked with the host-only translation units, built with -fsanitize=address,undefined and run
    as a child process: the tie and its refusal, the hash, directed views on synthetic records (ties across segments under descending
    keys, a filter that keeps none and one that keeps all, limit 1 / = kept / > kept, an average at a count of 2^39 against thresholds
    at the edges of int32, decided where int64 would wrap) and 300 random views against a sort on the values."""
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    exe = str(tmp_path / "merge_view_asan")
    csrc = os.path.join(ROOT, "immutable3_amd", "csrc")
    units = ["imm3_merge_view_plan.cpp", "imm3_merge_view_host.cpp", "imm3_group_order_plan.cpp", "imm3_group_filter_plan.cpp", "imm3_expr_norm.cpp"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-D__HIP_PLATFORM_AMD__", "-I", hip_inc,                      # (imm3_expr_norm.cpp reads the handles' header)
                           os.path.join(HERE, "native", "merge_view_asan.cpp")] + [os.path.join(csrc, u) for u in units] + ["-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    assert r.stdout.splitlines() == ["tie ok", "hash ok", "directed views ok", "300 random views ok"], r.stdout
