"""The chunk walk of KSCHED_APPLY_WHILE_FIT (csrc/apply_admit.hpp) checked on the host, no GPU: a 64-lane emulation of k_apply_admit over
the shared arithmetic -- split-half prefix sums, the per-lane test, the first failing lane, the carry -- against the serial rule, over
every segment of up to 4 pods with requests and `available` from {-1, 0, 1, 2, INT64_MAX, INT64_MIN}, random segments of 63 to 1000 pods,
and the step counts the shortcut for chunks without a negative request promises: tests/cpp/apply_admit_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "apply_admit_tests")


def test_chunk_walk_equals_the_serial_rule_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/apply_admit_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
    assert "62209186 segments" in r.stdout  # 36 * (1 + 36 + 36^2 + 36^3 + 36^4) exhaustive ones, 15 400 random ones, 6 counted
