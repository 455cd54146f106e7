"""ksched_apply_bindings_sharded / ksched_apply_bindings_sharded_local on the MI355X: every replica of a row-sharded batch ends where ONE
ctx's ksched_apply_bindings_device over the concatenated rows ends (columns, index checksum, statuses).

n > 1 ranks run as n ctxs on the one GPU in ONE child process (tests/apply_sharded_worker.py) against the test build of the library with
the RCCL stand-in; n = 1 runs the shipped library over the real RCCL.  Only the per-process test starts two children at once.
The "paths" case runs tests/apply_paths_worker.check_matrix in its reduced form on every replica after each sharded apply: with it the
pack pick's legs (tests/pack_ref.py on the columns the gathered commit wrote) and the combining chains (KSCHED_COMBINE_AND / _OR / _ANDNOT
and KSCHED_COMBINE_SOFT against tests/combine_ref.py / tests/soft_ref.py, a pick in the soft chain's last link), and the operator and
tagged selector calls (KSCHED_SELOP_EXISTS / _GT / _LT, KSCHED_SELOP_TAGGED): their bare masks against tests/selop_ref.py /
tests/seltag_ref.py, the plain table under the tagged call against the oracle, and a chain of them on one mask whose last link carries
each of the five picks in turn on the columns the gathered commit wrote -- the first operator and tagged calls on a replica after a
sharded apply; and the terms call (KSCHED_SEL_TERMS) beside them: its bare mask against tests/selterms_ref.py, one term against the tagged
mask, the padded plain table against the oracle and the terms chain with each of the five picks in its last link."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = {"KSCHED_TEST_HOOKS": "1", "KSCHED_LIB": os.path.join(ROOT, "tests", "cpp", "hooks", "libksched_hip.so"),
         "KSCHED_RCCL_LIB": os.path.join(ROOT, "tests", "cpp", "libfake_rccl.so")}
NODES = [1, 1023, 1025, 5000, 50_000]
PATHS_NODES = [63, 4097, 50_000]  # of the "paths" case (tests/test_apply_paths_host.py walks the same without a GPU)


def _cmd(case, spec):
    return [sys.executable, "-m", "tests.apply_sharded_worker", case, json.dumps(spec)]


def _env(hooks, extra=None):
    env = dict(os.environ, **(HOOKS if hooks else {}), **(extra or {}))
    if not hooks:
        for k in HOOKS:
            env.pop(k, None)
    return env


def run(case, spec, hooks=True, timeout=600, extra=None):
    for k in ("KSCHED_LIB", "KSCHED_RCCL_LIB"):
        assert not hooks or os.path.exists(HOOKS[k]), f"{HOOKS[k]} has not been built (make test-lib host)"
    r = subprocess.run(_cmd(case, spec), cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=_env(hooks, extra))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-6000:]
    assert r.stdout.rstrip().endswith(f"ok {case}")
    return r.stdout


def test_one_rank_over_the_real_rccl_equals_the_single_ctx_apply(built):
    run("equal", {"n": 1, "nodes": NODES}, hooks=False)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_replicas_equal_the_single_ctx_apply(built, n):
    run("equal", {"n": n, "nodes": NODES})


def test_chain_sampled_pick_at_c3(built):
    run("chain", {"n": 3, "mode": "sampled"}, timeout=900)


def test_chain_bestfit_at_c5_shard(built):
    run("chain", {"n": 2, "mode": "bestfit"}, timeout=900)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_every_replica_evaluates_right_after_a_sharded_apply(built, n):
    """the select pick, the waves-form riding pick, ksched_explain, the direct kernel, list-key best fit, the uniform and the spread pick on
    every replica, against the oracle (the spread pick: tests/spread_ref.py on the columns the gathered commit must have left on that
    replica); n = 1 over the real RCCL"""
    out = run("paths", {"n": n, "nodes": PATHS_NODES}, hooks=n > 1, timeout=900)
    reached = out.rsplit("picks reached", 1)[-1]
    assert "'spread'" in reached, "the spread pick is not among the picks reached"
    for pick in ("pack", "spread", "uniform", "sampled", "bestfit"):
        assert f"'selchain-{pick}'" in reached, f"no selector chain carried the {pick} pick in its last link"
        assert f"'termchain-{pick}'" in reached, f"no terms chain carried the {pick} pick in its last link"


def test_shards_longer_than_one_stride_of_the_pod_kernels(built):
    run("large", {}, timeout=600)


def test_apply_to_an_empty_snapshot(built):
    run("empty", {"n": 2})


def test_scratch_is_idle_after_either_apply(built):
    run("scratch", {"n": 3})


def test_failed_collective_invalidates_every_replica(built):
    run("failure", {}, extra={"FAKE_RCCL_FAIL_ALLGATHER": "2"}, timeout=300)


def test_argument_errors(built):
    run("errors", {}, timeout=300)


def test_per_process_form_through_abicomm(built, tmp_path):
    """two processes on the one GPU, each one rank of dist.AbiComm over the stand-in's clique of processes"""
    world = 2
    procs = [subprocess.Popen(_cmd("rank", {"rank": r, "world": world, "dir": str(tmp_path)}), cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=_env(True)) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, o[-3000:] + e[-5000:]
    res = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ref = res[0]
    for k in range(3):
        for r in range(world):
            x = res[r]
            assert np.array_equal(x[f"cpu{k}"], ref[f"ref_cpu{k}"]) and np.array_equal(x[f"mem{k}"], ref[f"ref_mem{k}"]), (k, r)
            assert np.array_equal(x[f"sum{k}"], ref[f"ref_sum{k}"]), (k, r)
            lo, hi = x[f"lo{k}"]
            assert np.array_equal(x[f"st{k}"], ref[f"ref_st{k}"][lo:hi]), (k, r)
    assert res[1]["lo2"][0] == res[1]["lo2"][1], "the third batch gives rank 1 an empty shard"
