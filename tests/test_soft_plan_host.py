"""The rules of a soft combining evaluation -- KSCHED_COMBINE_SOFT (csrc/mask_combine_soft.hpp, csrc/eval_plan.hpp) -- checked on the host,
no GPU: the constant, a single bit outside every other flag set, which changes no word's op; every refusal, for the entry points that accept
combining calls and for those that refuse them (no op, OR, two ops, no mask, a fit mask); the row rule on hand-written rows; the launch
plan at each side of every switch (the group sizes 1 .. 64, registers against two reads) for both unit widths, and the launch walked on the
CPU as the kernel walks it (every word below W by exactly one lane of exactly one group, no padding word); the plan with the bit against
the plain combining plan: tests/cpp/soft_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "soft_plan_tests")


def test_soft_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/soft_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
