"""The rules of a tagged call -- KSCHED_SELOP_TAGGED (csrc/sel_tags.hpp, csrc/eval_plan.hpp) -- checked on the host, no GPU: the constants;
every refusal and every accepted combination of check_seltag_args (the flag beside each KSCHED_SELOP_* flag, without KSCHED_SEL, with fit,
taint or a fit mask; a combine op, the modifier and a pick beside it); the rule for one (entry, id) pair by the hand table of
tests/test_seltag_restatement.py, and the one compare form the kernel decodes every tag into against it; one pod's row against a loop over
single bits, padding bits under NE and ABSENT included; the launch plan walked on the CPU as the kernel walks it (every word below W by
exactly one lane, every key by exactly one pass); the plan of a tagged call plain, combining, soft and with each pick, with
KSCHED_OPT_KERNEL forced each way; and a request without the flag against the plan as it was: tests/cpp/seltag_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "seltag_plan_tests")


def test_seltag_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/seltag_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
