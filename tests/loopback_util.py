"""The test side of the two-rank loopback tests (test_gpu_comm_loopback.py says what the transport is): build
tests/native/loopback_rccl.cpp, then run a worker script in a process of its own with IMM3_RCCL_LIB pointing at it.  The workers
take their ranks from loopback_ranks.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "loopback_rccl.cpp")


def build_transport(tmp_path):
    lib = tmp_path / "libloopback_rccl.so"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "hip", "--offload-arch=gfx950", SRC, "-o", str(lib)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(lib)


def run_worker(tmp_path, name, source, marker):
    """Write `source` as tmp_path/name, run it (argv[1]: the repository) over the loopback transport; it must exit 0 and print `marker`."""
    script = tmp_path / name
    script.write_text(source)
    env = dict(os.environ, IMM3_RCCL_LIB=build_transport(tmp_path))
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=900)
    sys.stdout.write(r.stdout[-4000:])
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0 and marker in r.stdout
