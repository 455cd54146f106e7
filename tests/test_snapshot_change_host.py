"""The pure parts of a node-snapshot change (csrc/snapshot_change.hpp) checked on the host, no GPU: which rows of an update count
(the last of every node, and the tiles they touch), whether the planned index layout survives a label update, where the fields of the
three staging blocks lie, and what each change makes stale -- every rule at its boundary: tests/cpp/snapshot_change_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "snapshot_change_tests")


def test_snapshot_change_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/snapshot_change_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
