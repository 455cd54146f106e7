"""The numbers the best-fit structures and launches are sized by (csrc/bestfit_layout.hpp) checked on the host, no GPU: the sample and
level arrays of the two orders at every level boundary, the merge passes, the row bitmaps, the hand-over buffer's offsets, the
rotation of its counter sets, the debug bits, and a sweep against the expressions the launcher had written inline:
tests/cpp/bestfit_layout_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "bestfit_layout_tests")


def test_bestfit_layout_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/bestfit_layout_tests"])  # (plain g++: the header includes neither HIP nor the ctx)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
    assert " 0 differences" in r.stdout
