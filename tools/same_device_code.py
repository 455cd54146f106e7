#!/usr/bin/env python3
"""Is the device code of the work tree the same as revision REV's?

    tools/same_device_code.py HEAD~1

Compiles kube_scheduler_rs_reference_amd/csrc/ksched_api.hip to device assembly (the Makefile's HIPCC and HIPFLAGS plus
--offload-device-only -S), once from the work tree and once from `git archive REV` in a temporary directory, and compares the
two files line by line.  Lines that name __hip_cuid_ are left out: that symbol carries a hash of the whole translation unit, so
it changes with any edit, host code included.  Exit status 0: identical; 1: they differ (the first differing lines are printed).

When the files differ the functions are compared one by one as well, by name, with the function's ordinal masked in its local labels
(.LBB<n>_<block>, .Lfunc_end<n>, "Header=BB<n>_<block>" comments): a change that ADDS a kernel moves the ordinals of the functions
emitted after it and nothing else of them -- except the blanks in front of a label's trailing comment, which the assembly printer pads to a
column and which therefore move when an ordinal gains a digit (.LBB99_4 -> .LBB100_4); they are squeezed to one.  The last line then names the functions added, removed and changed; exit status 2 when none
was removed or changed (every function of REV is in the work tree with the same instructions), 1 otherwise.

What it is for: a refactor of the host side (the dispatch, the ABI functions) must leave every kernel as it was; with this
check passing, any difference in results or speed is in the host path.  No GPU is needed; each compile takes about 45 s, the two
run side by side."""
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join("kube_scheduler_rs_reference_amd", "csrc", "ksched_api.hip")


def compile_command():
    """[hipcc, flags...] as the work tree's Makefile has them"""
    out = subprocess.check_output(["make", "-s", "-C", ROOT, "--no-print-directory", "--eval", "print-hipcc: ; @echo $(HIPCC) $(HIPFLAGS)", "print-hipcc"],
                                  text=True)
    return out.split() + ["--offload-device-only", "-S"]


def device_lines(path):
    with open(path) as f:
        return [ln for ln in f if "__hip_cuid_" not in ln]


def functions(lines):
    """{name: its lines between "Begin function" and "End function", the function's ordinal masked in local labels}"""
    out, cur = {}, None
    for ln in lines:
        m = re.search(r"; -- Begin function (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif "; -- End function" in ln:
            cur = None
        elif cur is not None:
            ln = re.sub(r"(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end|\.Ltmp)\d+(?=_|\b)", r"\1N", ln)
            cur.append(re.sub(r"^(\.LBBN_\d+:)[ \t]+;", r"\1 ;", ln))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    cmd = compile_command()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.mkdir(old)
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", rev, "kube_scheduler_rs_reference_amd/csrc", "include"])
        with tarfile.open(fileobj=io.BytesIO(tar)) as t:
            t.extractall(old)
        outs = [os.path.join(tmp, "new.s"), os.path.join(tmp, "old.s")]
        procs = [subprocess.Popen(cmd + ["-o", out, SRC], cwd=cwd) for out, cwd in zip(outs, (ROOT, old))]
        if any(p.wait() for p in procs):
            sys.exit("the compile failed: " + " ".join(cmd))
        new_s, old_s = (device_lines(o) for o in outs)
    kernels = sum(1 for ln in new_s if ".amdhsa_kernel " in ln)
    if new_s == old_s:
        print(f"identical device code: {len(new_s)} lines, {kernels} kernels (work tree against {rev})")
        return 0
    shown = 0
    for i, (a, b) in enumerate(zip(new_s, old_s)):
        if a != b and shown < 10:
            print(f"line {i + 1}:\n  {rev}: {b.rstrip()}\n  work tree: {a.rstrip()}")
            shown += 1
    print(f"device code DIFFERS: {len(new_s)} lines in the work tree, {len(old_s)} in {rev}")
    new_f, old_f = functions(new_s), functions(old_s)
    added = sorted(set(new_f) - set(old_f))
    removed = sorted(set(old_f) - set(new_f))
    changed = sorted(k for k in old_f if k in new_f and old_f[k] != new_f[k])
    print(f"function by function (local label ordinals masked): {len(old_f) - len(removed) - len(changed)} of {rev}'s {len(old_f)} functions have the same "
          f"instructions in the work tree; added {added}; removed {removed}; changed {changed}")
    return 1 if removed or changed else 2


if __name__ == "__main__":
    sys.exit(main())
