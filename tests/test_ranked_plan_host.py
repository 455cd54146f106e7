"""The plan of a ranked-pick request -- KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD, KSCHED_PICK_PACK (csrc/eval_plan.hpp) -- and the pipe's
waits for it (csrc/pipe_plan.hpp) checked on the host, no GPU, every rule for every member: the mask kernel always runs (fused or direct
as for a mask-only request, into the scratch mask exactly when the caller gave none), the member's pick follows it, no other pick is
planned and nothing rides, last_pick is the member's name, a forced fused kernel that does not apply is KSCHED_E_UNSUPPORTED,
pick_reads_mask is true under every option, every sequence of pipe submits plans the waits the same sequence with another member plans,
and today's requests keep today's plans: tests/cpp/ranked_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "ranked_plan_tests")


def test_ranked_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/ranked_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
