"""The plan of a KSCHED_PICK_PACK request (csrc/eval_plan.hpp) and the pipe's waits for it (csrc/pipe_plan.hpp) checked on the host, no
GPU: the mask kernel always runs (fused or direct as for a mask-only request, into the scratch mask exactly when the caller gave none),
the pack pick follows it, last_pick is "pack", a forced fused kernel that does not apply is KSCHED_E_UNSUPPORTED, pick_reads_mask is true
under every option, and every sequence of pipe submits plans the waits the same sequence with the spread pick plans:
tests/cpp/pack_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "pack_plan_tests")


def test_pack_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/pack_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
