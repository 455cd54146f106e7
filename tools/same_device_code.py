#!/usr/bin/env python3
"""Is the device code of the work tree the same as revision REV's?

    tools/same_device_code.py HEAD~1

Compiles kube_scheduler_rs_reference_amd/csrc/ksched_api.hip to device assembly (the Makefile's HIPCC and HIPFLAGS plus
--offload-device-only -S), once from the work tree and once from `git archive REV` in a temporary directory, and compares the
two files line by line.  Lines that name __hip_cuid_ are left out: that symbol carries a hash of the whole translation unit, so
it changes with any edit, host code included.  Exit status 0: identical; 1: they differ (the first differing lines are printed).

What it is for: a refactor of the host side (the dispatch, the ABI functions) must leave every kernel as it was; with this
check passing, any difference in results or speed is in the host path.  No GPU is needed; each compile takes about 45 s, the two
run side by side."""
import io
import os
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
    return 1


if __name__ == "__main__":
    sys.exit(main())
