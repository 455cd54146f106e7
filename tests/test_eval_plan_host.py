"""The evaluation plan (csrc/eval_plan.hpp) checked on the host, no GPU: which mask kernel a request runs, how its sampled pick
runs (own launch, riding as waves of the fill or as tile tests, from the mask), how its best fit runs (one stage, two, two plus the
listed kernel, from the mask), and which requests are unsupported -- every rule at its boundary: tests/cpp/plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "plan_tests")


def test_eval_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
