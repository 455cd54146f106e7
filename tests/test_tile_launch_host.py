"""The description of a tile-kernel launch (csrc/tile_launch.hpp) checked on the host, no GPU: the LDS carve-up against the byte
counts the fused and the summary kernel have always been launched with, the launch geometry with every measured rule at its boundary
(the chunk-count rule: C3's 49 chunks against 51), the argument fill both kernels share and the predicate dispatcher:
tests/cpp/tile_launch_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "tile_launch_tests")


def test_tile_launch_description_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/tile_launch_tests"])  # (g++; the HIP headers are read for their types only)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
