"""The input conditions of the spread legs in tests/apply_paths_worker.py, without a GPU: the worker's own sequences (walk_single, and
walk_paths of tests/apply_sharded_worker.py) walked with the oracle, tests/uniform_ref.py, tests/spread_ref.py and the exact-integer apply
in place of the device, over the specs the GPU tests pass.  The walks assert what the GPU cases assert of their inputs: (a) before any
apply at 1025 nodes or more, the d = 5 spread restatement binds 35 % of the pods or more to another node than their candidate 0 (and the
uniform legs' condition holds); (b) at every such node count the columns from before an apply of real bindings would change at least one
spread binding, summed over its rounds; and the sampled, the uniform and the spread pick each hand their bindings on.  A change of the
shapes, the seeds or the rotation that would let the GPU legs pass with stale columns fails here first."""
import numpy as np
import pytest

from oracle.oracle_ref import apply_bindings_exact
from tests import apply_paths_worker as W
from tests.test_gpu_apply_paths import SINGLE
from tests.test_gpu_apply_sharded import PATHS_NODES


def exact_apply(S, cpu, mem, b, ok, flags, what):
    P = len(b)
    return apply_bindings_exact(cpu, mem, b, S["rc"][:P], S["rm"][:P], ok, flags)


def restated(S, cpu, mem, what, rng, **kw):
    return W.restated_matrix(S, cpu, mem, None, what, rng, **kw)


@pytest.mark.parametrize("kind", W.KINDS)
def test_single_ctx_matrix_inputs(kind, capsys):
    handed = W.walk_single(dict(SINGLE, kind=kind), lambda S, cpu, mem, what: None, restated, exact_apply)
    assert set(handed) == {False, True} and all(set(p) == set(W.PICKS) for p in handed.values()), handed  # all three picks in both classes
    out = capsys.readouterr().out
    print(out)
    assert out.count("the spread pick (d = 5) binds") >= 3 and out.count("would change") >= 8


@pytest.mark.parametrize("n", [1, 2, 3])
def test_replicated_matrix_inputs(n, capsys):
    from tests import apply_sharded_worker as SW
    from tests.test_gpu_apply_bindings import restate
    handed = []

    def matrix(q, S, cpu, mem, what, rng, **kw):
        if kw.get("hand_on"):
            handed.append((S["N"] >= 1025, kw["hand_on"]))
        return W.restated_matrix(S, cpu, mem, None, what, rng, reduced=True, **kw)

    def apply(S, cpu, mem, bounds, b, ok, flags, use_ok, what):
        return restate(cpu, mem, b, S["rc"], S["rm"], ok if use_ok else None, flags)

    k = SW.walk_paths({"n": n, "nodes": PATHS_NODES}, lambda S, what: None, matrix, apply, lambda: None)
    out = capsys.readouterr().out
    print(out)
    assert k == 12 and out.count("would change") == 6
    assert {p for big, p in handed if big} == set(W.PICKS), handed  # at 1025 nodes or more: all three within one run
    # (below 1025 a run has two snapshots: the three picks over the runs with n = 1, 2, 3)
    assert len({p for big, p in handed if not big}) == 2, handed
    assert {W.PICKS[(ki + m) % 3] for ki in (0, 1) for m in (1, 2, 3)} == set(W.PICKS)


@pytest.mark.parametrize("change", ["negated", "permuted", "apply"])
def test_pipe_snapshot_change_inputs(change):
    """tests/test_gpu_spread_pick.py::test_pipe_submits_around_a_snapshot_change can tell the old snapshot from the new one"""
    from tests.test_gpu_spread_pick import assert_old_and_new_can_be_told_apart
    assert_old_and_new_can_be_told_apart(change)


def test_restated_matrix_draws_what_check_matrix_draws():
    """the walk without a device is the walk with one only if both advance the generator alike: per predicate set one call of
    explain_pairs (check_matrix draws its pairs through it too)"""
    S = W.snapshot("taints", 63, 50, 1)
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    W.restated_matrix(S, S["cpu"], S["mem"], None, "x", a, hand_on=None)
    for _ in S["preds"]:
        W.explain_pairs(b, S["P"], S["N"])
    assert a.integers(0, 1 << 60) == b.integers(0, 1 << 60)
