"""KSCHED_APPLY_WHILE_FIT at ksched_apply_bindings_sharded_local on the MI355X: KSCHED_E_UNSUPPORTED with nothing changed and the clique
usable afterwards (tests/admit_sharded_worker.py: two ctxs on the one GPU in one child process, the test build of the library with the RCCL
stand-in, as tests/test_gpu_apply_sharded.py runs its cases)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = {"KSCHED_TEST_HOOKS": "1", "KSCHED_LIB": os.path.join(ROOT, "tests", "cpp", "hooks", "libksched_hip.so"),
         "KSCHED_RCCL_LIB": os.path.join(ROOT, "tests", "cpp", "libfake_rccl.so")}


def test_the_sharded_apply_refuses_the_flag_and_stays_usable(built):
    for k in ("KSCHED_LIB", "KSCHED_RCCL_LIB"):
        assert os.path.exists(HOOKS[k]), f"{HOOKS[k]} has not been built (make test-lib host)"
    r = subprocess.run([sys.executable, "-m", "tests.admit_sharded_worker", "refused", json.dumps({"n": 2})], cwd=ROOT, capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, **HOOKS))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-6000:]
    assert r.stdout.rstrip().endswith("ok refused")
