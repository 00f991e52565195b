"""The arithmetic of the merges' shape vote (csrc/imm3_merge_vote.h: the five words a rank sends, the zeros of a failed rank, the
verdict read from the reduced words) alone under AddressSanitizer + UBSan: tests/native/merge_vote_asan.cpp is a stand-alone program
with its own main that simulates the all-reduce(max) over 2 and 3 ranks.  No GPU, nothing loaded into python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKS = 24


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_merge_vote_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "merge_vote_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "native", "merge_vote_asan.cpp"), "-o", exe])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == CHECKS and all(line.endswith(" ok") for line in lines), r.stdout
