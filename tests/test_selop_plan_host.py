"""The rules of an operator call -- KSCHED_SELOP_EXISTS / _GT / _LT (csrc/sel_ops.hpp, csrc/eval_plan.hpp) -- checked on the host, no GPU:
the constants, single bits outside every other flag set; every refusal and every accepted combination (one operator, KSCHED_SEL, no fit,
taint or fit mask; a combine op, the modifier and a pick beside it); the rule for one (entry, id) pair by hand and one pod's row against
a loop over single bits; the launch plan at its boundaries and walked on the CPU as the kernel walks it (every word below W by exactly one
lane, no padding word, every key by exactly one pass); the plan of an operator call with and without combine, soft and each pick, with
KSCHED_OPT_KERNEL forced either way; and a request without an operator against the plan as it was: tests/cpp/selop_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "selop_plan_tests")


def test_selop_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/selop_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
