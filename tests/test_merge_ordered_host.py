"""The host-only unit of imm3_comm_merge_ordered (csrc/imm3_merge_order_host.cpp: record geometry, vote words, argument rules, the
host k-way merge of the single-process flavour) alone under AddressSanitizer + UBSan: tests/native/merge_order_asan.cpp is a
stand-alone program with its own main.  No GPU, nothing loaded into python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHECKS = 32


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_merge_order_host_unit_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "merge_order_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "merge_order_asan.cpp"), os.path.join(ROOT, "immutable3_amd", "csrc", "imm3_merge_order_host.cpp"),
                           "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == CHECKS and all(line.endswith(" ok") for line in lines), r.stdout


def test_the_entry_points_are_declared_and_bound():
    """include/imm3.h declares both entry points, native.py binds them, and ORDER BY's header text points at the merge."""
    from immutable3_amd import native
    header = open(os.path.join(ROOT, "include", "imm3.h")).read()
    for name in ("imm3_comm_merge_ordered", "imm3_comm_merge_ordered_all"):
        assert f"int {name}(" in header and name in native.EXPORTS
    assert "OUT OF SCOPE: merging ordered results" not in header
    assert callable(native.Comm.merge_ordered) and callable(native.Comm.merge_ordered_all)
