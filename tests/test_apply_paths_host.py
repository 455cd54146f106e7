"""The input conditions of the spread, the pack and the combining legs in tests/apply_paths_worker.py, without a GPU: the worker's own sequences (walk_single, and
walk_paths of tests/apply_sharded_worker.py) walked with the oracle, tests/uniform_ref.py, tests/spread_ref.py and the exact-integer apply
in place of the device, over the specs the GPU tests pass.  The walks assert what the GPU cases assert of their inputs: (a) before any
apply at 1025 nodes or more, the d = 5 spread restatement binds 35 % of the pods or more to another node than their candidate 0 (and the
uniform legs' condition holds); (b) at every such node count the columns from before an apply of real bindings would change at least one
spread binding, summed over its rounds; and the sampled, the uniform and the spread pick each hand their bindings on.  A change of the
shapes, the seeds or the rotation that would let the GPU legs pass with stale columns fails here first.  Likewise the admit legs
(KSCHED_APPLY_WHILE_FIT): the admit round of every node count with admit_round_conditions' floors, the sizes and the large case's plans
(sizes_step, large_plan) and the pipe's admit -- an admit that defers nobody where a floor says it must fails here, not on a GPU.
Likewise the pack legs (KSCHED_PICK_PACK) and the combining chains (KSCHED_COMBINE_*, KSCHED_COMBINE_SOFT): at 1025 nodes or more the d = 5
pack restatement binds 35 % of the pods or more to another node than their candidate 0 and than the spread restatement; either soft tier
narrows 20 %, is dropped for 10 %, finds 1 % empty and changes 10 % of the rows or more; the pack pick on the tier-2 mask differs from the
hard mask's for 15 % of the pods or more; fit & ~feasible has a set bit in 30 % of the rows or more; a stale column would change a pack
binding of the matrix's legs; and the sizes plan's chain meets the same floors at its three large snapshots.
Likewise the operator and the tagged selector legs (KSCHED_SELOP_EXISTS / _GT / _LT, KSCHED_SELOP_TAGGED; assert_selector_input_conditions, on
tests/selop_ref.py and tests/seltag_ref.py alone): at 1025 nodes or more, under each operator and under the tagged table half of the
constrained rows or more are neither full nor empty; a tenth of the pods or more are constrained through NE / ABSENT entries only; all six
tags and SEL_NEVER occur; on the nine- and ten-key snapshots a tenth of the pods or more constrain a key below 8 and a key at 8 or above;
every link of the selector chain changes 5 % of the rows or more -- in the single walks, the sizes plan and the replicated walk.
Likewise the legs of the terms call (KSCHED_SEL_TERMS; assert_terms_input_conditions, on tests/selterms_ref.py alone), from 63 nodes on: a
quarter of the rows or more are neither empty nor full; 5 % or more differ from every single term's row; a tenth or more are full although
term 0's row is not; on the nine- and ten-key snapshots a fifth or more differ from the and-of-ors formula; each term count occurs in a
fifth of the pods or more; every link of the terms chain changes 5 % of the rows or more."""
import numpy as np
import pytest

from tests import apply_paths_worker as W
from tests.admit_ref import apply_exact
from tests.test_gpu_apply_paths import LARGE, NODES, SINGLE, SIZES
from tests.test_gpu_apply_sharded import PATHS_NODES


def exact_apply(S, cpu, mem, b, ok, flags, what):
    P = len(b)
    return apply_exact(cpu, mem, b, S["rc"][:P], S["rm"][:P], ok, flags)


def restated(S, cpu, mem, what, rng, **kw):
    return W.restated_matrix(S, cpu, mem, None, what, rng, **kw)


@pytest.mark.parametrize("kind", W.KINDS)
def test_single_ctx_matrix_inputs(kind, capsys):
    handed = W.walk_single(dict(SINGLE, kind=kind), lambda S, cpu, mem, what: None, restated, exact_apply)
    assert set(handed) == {False, True} and all(set(p) == set(W.PICKS) for p in handed.values()), handed  # all three picks in both classes
    out = capsys.readouterr().out
    print(out)
    assert out.count("the spread pick (d = 5) binds") >= 3 and out.count("would change") >= 8
    # the pack and the combining legs' conditions, per predicate set of the three node counts from 1025 on: asserted by restated_matrix
    # (assert_pack_input_condition, assert_chain_input_conditions), printed in words of their own; and the stale-column count of the pack
    # restatement beside the spread one's, asserted by walk_single
    sets = 3 * len(W.snapshot(kind, 63, 8, 1)["preds"])
    assert out.count("the pack pick (d = 5) binds") == sets and out.count("to another node than the spread pick") == sets
    assert [out.count(f"soft tier {tier} (") for tier in (1, 2)] == [sets, sets]
    assert out.count("on the tier-2 mask binds") == sets and out.count("of the rows of fit & ~feasible have a set bit") == sets
    assert out.count("pack bindings") == out.count("would change")
    # the operator and the tagged legs' conditions, per predicate set of the same node counts (every predicate set has SEL)
    assert out.count("are neither full nor empty") == out.count("through NE / ABSENT entries only") == out.count("the selector chain's links change") == sets
    assert out.count("constrain a key below 8 and a key at 8 or above") == (sets if kind in ("many-keys", "list-key") else 0)
    # the terms call's conditions (assert_terms_input_conditions), per predicate set of the same node counts
    # -- these from 63 nodes on: four node counts
    tsets = sets // 3 * 4
    assert out.count("of the rows of the terms call") == out.count("term counts 1 .. 3 occur in") == out.count("the terms chain's links change") == tsets
    assert out.count("the terms ORed pass by pass and the passes ANDed differ") == (tsets if kind in ("many-keys", "list-key") else 0)
    # the admit round of every node count, with the floors walk_single sets on it (admit_round_conditions), printed in words of its own
    assert [out.count(f"{kind} N={N} admit round (") > 0 for N in NODES] == [True] * len(NODES)
    assert out.count("statuses (applied, unbound, not ok, deferred, overflow, bad node)") == len(NODES)
    assert out.count("the columns from before this admit move") == 2  # the two on real bindings


def test_sizes_case_inputs(capsys):
    """tests/apply_paths_worker.py case_sizes without a device: every WHILE_FIT apply of the committed spec meets sizes_step's floors, and
    exactly one step has the admit that outgrows the admit scratch"""
    plans = [W.sizes_step(step, N) for step, N in enumerate(SIZES["nodes"])]
    assert [len(q["applies"]) for q in plans] == [4 if N == 4097 else 3 for N in SIZES["nodes"]]
    big = plans[SIZES["nodes"].index(4097)]["applies"]
    assert len(big[3][0]) > len(big[2][0]) + len(big[2][0]) // 4 and all(a[2] == 0x08 for a in big[2:])  # past the 25 % headroom
    assert all((q["updates"][0][0].size, q["updates"][1][0].size) == (min(50, q["S"]["N"]),) * 2 for q in plans)
    out = capsys.readouterr().out
    print(out)
    assert out.count(": admit of ") == len(SIZES["nodes"]) + 1
    # the soft chain behind the queued changes: expected masks and bindings for every step, the floors where a floor can hold
    big_steps = sum(N >= 1025 for N in SIZES["nodes"])
    assert big_steps == 3 and [out.count(f"chain: soft tier {tier} (") for tier in (1, 2)] == [big_steps, big_steps]
    assert out.count("chain: the pack pick (d = 5) on the tier-2 mask binds") == big_steps
    # the selector chain behind it: the floors at the same three snapshots, expected masks and spread bindings for every step
    assert out.count("selchain: of the constrained rows") == out.count("selchain: the tagged table constrains") == big_steps
    assert out.count("selchain: the selector chain's links change") == big_steps
    # and the terms chain behind that: the floors at the same three snapshots, expected masks and pack bindings for every step
    assert out.count("termchain: of the rows of the terms call") == out.count("termchain: term counts 1 .. 3 occur in") == big_steps
    assert out.count("termchain: the terms chain's links change") == big_steps
    for q in plans:
        S, c = q["S"], q["chain"]
        assert [m.shape for m in c["links"]] == [(S["P"], (S["N"] + 63) // 64)] * 3 and c["bind"].shape == (S["P"],)
        assert ((c["bind"] >= 0) == c["links"][2].any(axis=1)).all() and (c["links"][2].any(axis=1) == c["links"][0].any(axis=1)).all()
        sc = q["selchain"]
        assert sc["first"] == W.FIT | W.TAINT and [m.shape for m in sc["links"]] == [(S["P"], (S["N"] + 63) // 64)] * 5 and sc["bind"].shape == (S["P"],)
        assert ((sc["bind"] >= 0) == sc["links"][4].any(axis=1)).all() and (sc["links"][4].any(axis=1) == sc["links"][3].any(axis=1)).all()  # the last link is soft
        tc = q["termchain"]
        assert tc["first"] == W.FIT | W.TAINT and [m.shape for m in tc["links"]] == [(S["P"], (S["N"] + 63) // 64)] * 3 and tc["bind"].shape == (S["P"],)
        assert ((tc["bind"] >= 0) == tc["links"][2].any(axis=1)).all() and (tc["links"][2].any(axis=1) == tc["links"][1].any(axis=1)).all()  # the last link is soft
        assert S["terms"].shape == (W.TERMS, S["sel"].shape[0], S["P"]) and np.array_equal(S["terms"][0], S["tsel"])


def test_large_case_inputs(capsys):
    """case_large without a device: the 600 000-pod admit meets large_plan's floors, and the four applies behind it still meet theirs on
    the columns it leaves"""
    S, plan = W.large_plan(LARGE["pods"])
    assert [f for f, *_ in plan] == [0x08, 0, W.FPN, W.REL, W.FPN | W.REL] and LARGE["pods"] > W.LARGE_FAR + 64
    assert all(len(b) == LARGE["pods"] for _, b, _, _ in plan)
    out = capsys.readouterr().out
    print(out)
    assert "admit: statuses" in out


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
    sets = 2 * (2 + 1)  # the two node counts from 1025 on, the taints snapshot's two predicate sets and the list-key snapshot's one
    assert out.count("the pack pick (d = 5) binds") == out.count("the spread pick (d = 5) binds") == sets
    assert out.count("soft tier 1 (") == out.count("soft tier 2 (") == out.count("on the tier-2 mask binds") == out.count("the pack pick (d = 5) binds")
    assert out.count("are neither full nor empty") == out.count("through NE / ABSENT entries only") == out.count("the selector chain's links change") == sets
    assert out.count("constrain a key below 8 and a key at 8 or above") == 2  # the list-key snapshot's nine keys, at either node count
    # (the terms call's floors from 63 nodes on: all three node counts)
    assert out.count("of the rows of the terms call") == out.count("term counts 1 .. 3 occur in") == out.count("the terms chain's links change") == 3 * (2 + 1)
    assert out.count("the terms ORed pass by pass and the passes ANDed differ") == 3  # the list-key snapshot's nine keys, at every node count
    assert {p for big, p in handed if big} == set(W.PICKS), handed  # at 1025 nodes or more: all three within one run
    # (below 1025 a run has two snapshots: the three picks over the runs with n = 1, 2, 3)
    assert len({p for big, p in handed if not big}) == 2, handed
    assert {W.PICKS[(ki + m) % 3] for ki in (0, 1) for m in (1, 2, 3)} == set(W.PICKS)


@pytest.mark.parametrize("change", ["negated", "permuted", "apply", "admit"])
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
