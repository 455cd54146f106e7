"""The plan of a KSCHED_PICK_UNIFORM request (csrc/eval_plan.hpp) checked on the host, no GPU: the mask kernel always runs (fused or
direct by applicability and option, into the scratch mask when the caller gave none), the uniform pick follows it, no other pick is
planned and nothing rides; today's requests keep today's plans: tests/cpp/uniform_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "uniform_plan_tests")


def test_uniform_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/uniform_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
