"""The plan of a pipe submit (csrc/pipe_plan.hpp) checked on the host, no GPU: which streams carry a slot's mask kernel and its pick, which
of the slot's two events they first wait for, and what the slot remembers -- over a happens-before model of every sequence of four submits
on one slot (slots 0 to 8, every KSCHED_OPT_PIPE_MODE, picks that read the mask and picks that do not, with and without
ksched_pipe_wait_mask), the hole the rules had before, the waits of the steady state and the transitions the GPU tests state:
tests/cpp/pipe_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "pipe_plan_tests")


def test_pipe_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/pipe_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
