"""The rules of a tagged call with a term count -- KSCHED_SEL_TERMS (csrc/sel_terms.hpp, csrc/eval_plan.hpp) -- checked on the host, no GPU:
the constants; every refusal and every accepted combination of check_selterms_args at its boundary (the field without KSCHED_SELOP_TAGGED,
without KSCHED_SEL, beside each operator flag, with fit, taint or a fit mask, where it is not accepted); where entry (term, key, pod) lies;
one pod's row against seltag_row, with the case in which an AND of ORs differs from the OR of ANDs; the launch geometry walked on the CPU
as the two kernels walk it (every (word, pod) written exactly once by one launch, for W on each side of a wave's and a block's columns
and keys 8, 9 and 32); the plan with the field against the tagged call's; and a request without the field against the plan as it was:
tests/cpp/selterms_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "selterms_plan_tests")


def test_selterms_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/selterms_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
