"""The yardstick of the summary tests, pinned on the CPU: tests/summary_ref.py (three single-predicate oracle masks F, S, T and four
popcounts) against oracle.capi.check_node_validity pair by pair on one object-level golden, and hand-worked cases at the tile and word
edges, at the int64 ends, and for the precedence (a node that fails every predicate counts once, under resources)."""
import json
import os

import numpy as np
import pytest

from oracle import capi
from tests import summary_ref as ref
from tests.conftest import ROOT

FIT, SEL, TAINT = ref.FIT, ref.SEL, ref.TAINT
SEL_NEVER = 0xFFFFFFFF
GOLD = os.path.join(ROOT, "tests", "golden")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module", autouse=True)
def oracle_built():
    capi.build()


def test_restatement_equals_check_node_validity_pair_by_pair():
    """ragged_70x130_taints: the encoded columns (.npz) through the restatement == the objects (.json) through check_node_validity
    (src/predicates.rs:63-77) for every one of the 9 100 pairs, tallied by reason; with the taint extension a pair the reference
    accepts is rejected when tolerates_node_taints says so"""
    g = np.load(os.path.join(GOLD, "ragged_70x130_taints.npz"))
    obj = json.load(open(os.path.join(GOLD, "ragged_70x130_taints_objects.json")))
    pods, nodes, bound = obj["pods"], obj["nodes"], obj["bound"]
    P, N = len(pods), len(nodes)
    assert (P, N) == (70, 130)
    plain = np.zeros((P, 4), dtype=np.uint32)
    tainted = np.zeros((P, 4), dtype=np.uint32)
    for i, pod in enumerate(pods):
        for node in nodes:
            r = capi.check_node_validity(pod, node, bound)
            assert r in (0, 1, 2)
            plain[i, r] += 1
            if r == 0 and not capi.tolerates_node_taints(pod, node):
                r = 3
            tainted[i, r] += 1
    cols = (g["avail_cpu"], g["avail_mem"], g["node_labels"], g["node_taints"], g["req_cpu"], g["req_mem"], g["pod_sel"], g["pod_tol"])
    assert np.array_equal(ref.expected_counts(*cols, FIT | SEL), plain)
    assert np.array_equal(ref.expected_counts(*cols, FIT | SEL | TAINT), tainted)
    assert (tainted[:, 3] > 0).any() and (plain[:, 2] > 0).any() and (plain[:, 1] > 0).any()
    # row blocks do not change the answer
    assert np.array_equal(ref.expected_counts(*cols, FIT | SEL | TAINT, block=7), tainted)
    # a predicate that is not selected rejects nothing
    only_sel = ref.expected_counts(*cols, SEL)
    assert (only_sel[:, 1] == 0).all() and (only_sel[:, 3] == 0).all() and (only_sel.sum(axis=1) == N).all()


def one(avail_cpu, avail_mem, lab, tnt, rc, rm, sel, tol, flags):
    i64 = lambda a: np.array(a, dtype=np.int64)  # noqa: E731
    return ref.expected_counts(i64(avail_cpu), i64(avail_mem), None if lab is None else np.array(lab, dtype=np.uint32),
                               None if tnt is None else np.array(tnt, dtype=np.uint64), i64(rc), i64(rm),
                               None if sel is None else np.array(sel, dtype=np.uint32), None if tol is None else np.array(tol, dtype=np.uint64), flags)


@pytest.mark.parametrize("N", [1, 64, 65, 1023, 1024, 1025])
def test_hand_worked_counts_at_tile_and_word_edges(N):
    """node j has j units of both resources, label id 1 + j % 2 and taint bit 0 when j % 3 == 0; the pod asks for 2 units, label id 1
    (even nodes) and tolerates nothing"""
    j = np.arange(N)
    got = one(j, j, [1 + j % 2], np.where(j % 3 == 0, 1, 0), [2], [2], [[1]], [0], FIT | SEL | TAINT)
    fit = j >= 2
    sel = j % 2 == 0
    tnt = j % 3 != 0
    want = [int((fit & sel & tnt).sum()), int((~fit).sum()), int((fit & ~sel).sum()), int((fit & sel & ~tnt).sum())]
    assert got.tolist() == [want] and sum(want) == N
    # the closed forms, worked by hand: nodes 0 and 1 are short of resources whatever else they fail
    assert want[1] == min(N, 2)
    assert want[2] == max(0, N - 2) // 2  # the odd nodes from 3 on
    assert want[3] == len([x for x in range(2, N) if x % 2 == 0 and x % 3 == 0])


def test_a_node_that_fails_every_predicate_counts_once_under_resources():
    got = one([0, 5], [0, 5], [[2, 2]], [1, 1], [1], [1], [[1]], [0], FIT | SEL | TAINT)
    assert got.tolist() == [[0, 1, 1, 0]]  # node 0: resources (not selector, not taint); node 1 fits, misses the selector: selector, not taint
    got = one([5, 5], [5, 5], [[1, 1]], [1, 0], [1], [1], [[1]], [0], FIT | SEL | TAINT)
    assert got.tolist() == [[1, 0, 0, 1]]
    # without FIT the same node 0 is booked under the selector, without FIT and SEL under the taint
    assert one([0, 5], [0, 5], [[2, 2]], [1, 1], [1], [1], [[1]], [0], SEL | TAINT).tolist() == [[0, 0, 2, 0]]
    assert one([0, 5], [0, 5], [[2, 2]], [1, 1], [1], [1], [[1]], [0], TAINT).tolist() == [[0, 0, 0, 2]]


def test_int64_extremes():
    avail = [I64_MIN, -1, 0, I64_MAX]
    got = one(avail, avail, None, None, [I64_MIN, 0, I64_MAX, 1], [I64_MIN, 0, I64_MAX, I64_MIN], None, None, FIT)
    assert got.tolist() == [[4, 0, 0, 0], [2, 2, 0, 0], [1, 3, 0, 0], [1, 3, 0, 0]]
    # one resource alone decides
    got = one([I64_MAX] * 3, [I64_MIN, 0, I64_MAX], None, None, [I64_MAX], [0], None, None, FIT)
    assert got.tolist() == [[2, 1, 0, 0]]


def test_sel_never_and_a_pod_without_a_selector():
    lab = [[1, 2, 0, 1], [3, 3, 3, 0]]
    sel = [[SEL_NEVER, 0, 1, 0], [0, 0, 3, 0]]  # pod 0: a value no node carries; pod 1: no selector; pod 2: both keys; pod 3: no selector
    got = one([9] * 4, [9] * 4, lab, None, [1] * 4, [1] * 4, sel, None, FIT | SEL)
    assert got.tolist() == [[0, 0, 4, 0], [4, 0, 0, 0], [1, 0, 3, 0], [4, 0, 0, 0]]
    # sel_val_ids None = no pod has a selector; tolerations None = tolerate nothing
    got = one([9] * 4, [9] * 4, lab, [0, 1, 2, 0], [1], [1], None, None, FIT | SEL | TAINT)
    assert got.tolist() == [[2, 0, 0, 2]]


def test_restatement_columns_are_the_abi_reason_codes():
    """column r of the restatement is KSCHED_REASON_r of include/ksched.h, as the binding carries it, and a row has KSCHED_SUMMARY_WORDS words"""
    from kube_scheduler_rs_reference_amd import _lib
    assert ref.WORDS == _lib.SUMMARY_WORDS == 4
    assert (_lib.REASON_OK, _lib.REASON_NOT_ENOUGH_RESOURCES, _lib.REASON_NODE_SELECTOR_MISMATCH, _lib.REASON_TAINT_NOT_TOLERATED) == (0, 1, 2, 3)
    assert (ref.FIT, ref.SEL, ref.TAINT) == (_lib.FIT, _lib.SEL, _lib.TAINT)
    got = one([0, 5, 5, 5], [5] * 4, [[1, 2, 1, 1]], [0, 0, 1, 0], [1], [1], [[1]], [0], FIT | SEL | TAINT)[0]
    assert got[_lib.REASON_OK] == 1 and got[_lib.REASON_NOT_ENOUGH_RESOURCES] == 1 and got[_lib.REASON_NODE_SELECTOR_MISMATCH] == 1 and \
        got[_lib.REASON_TAINT_NOT_TOLERATED] == 1
