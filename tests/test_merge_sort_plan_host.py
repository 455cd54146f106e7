"""The device merge sort's plan (csrc/merge_sort_plan.hpp) checked on the host, no GPU: pass count, grids, run lengths and buffers of every
step at the sizes around each pass boundary up to 2^31 records (one more is refused), every plan up to 4097 records executed on the CPU over
an emulation of the two kernels' contracts with the stale set poisoned, against std::sort, and step by step against the two drivers
ksched_api.hip had before the header: tests/cpp/merge_sort_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "merge_sort_plan_tests")


def test_merge_sort_plan_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/merge_sort_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
