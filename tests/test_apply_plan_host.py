"""What an apply call does (csrc/apply_plan.hpp) checked on the host, no GPU: the flag verdict, the scratch step (first call, kept, regrown,
invalidated, the generation's wrap past 0), per rank the passes of each phase with their grids and per call the all-gathers, for every
combination of flags 0 .. 15, communicator, 1 and 3 ranks, 0 / 1 / 1024 / 1025 nodes, 0 / 1 / 1025 rows, status_out and index, against the
five functions that decided it before the header: tests/cpp/apply_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "apply_plan_tests")


def test_apply_plan_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/apply_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
