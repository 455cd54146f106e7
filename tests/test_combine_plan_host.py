"""The rules of a combining evaluation -- KSCHED_COMBINE_AND / _OR / _ANDNOT (csrc/mask_combine.hpp, csrc/eval_plan.hpp) -- checked on the
host, no GPU: the op of a flag word; the argument rules for the entry points that accept the flags and for those that refuse them; the
valid-bits word for n % 64 in {0, 1, 63}; the access width for aligned and unaligned bases and pitches; the launch geometry for one word,
one wave's worth and one unit more than a full grid pass, walked on the CPU (every word below W exactly once, no padding word); the plan
with an op (the mask kernel of a mask-only request into the scratch mask, nothing rides, the sampled and the best-fit pick from the mask,
the ranked picks as they are, a forced fused kernel that does not apply unsupported); and, over a sweep of today's requests, that the plan
without an op is the plan as it was: tests/cpp/combine_plan_tests.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "combine_plan_tests")


def test_combine_plan_rules_on_host():
    subprocess.check_call(["make", "-C", ROOT, "-s", "tests/cpp/combine_plan_tests"])  # (g++ alone: no ROCm header is needed)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed check(s)" in r.stdout
