"""tests/admit_ref.py (KSCHED_APPLY_WHILE_FIT restated) against answers worked by hand from the header's contract, and against the two
older rules' restatement (oracle_ref.apply_bindings_exact) where the three must agree.  No GPU."""
import numpy as np
import pytest

from oracle.oracle_ref import APPLY_FIRST_PER_NODE, APPLY_RELEASE, apply_bindings_exact
from tests.admit_ref import (APPLIED, BAD_NODE, DEFERRED, I64_MAX, I64_MIN, NOT_OK, OVERFLOW, UNBOUND, WHILE_FIT, admitted_behind_deferred,
                             apply_exact, apply_while_fit_exact, longest_segment)

A, D, O = APPLIED, DEFERRED, OVERFLOW


def run(cpu, mem, b, rc, rm, ok=None):
    c, m, st = apply_while_fit_exact(np.array(cpu, dtype=np.int64), np.array(mem, dtype=np.int64), np.array(b, dtype=np.int32),
                                     np.array(rc, dtype=np.int64), np.array(rm, dtype=np.int64), None if ok is None else np.array(ok, dtype=np.uint8))
    assert c.dtype == np.int64 and m.dtype == np.int64 and st.dtype == np.int32
    return c.tolist(), m.tolist(), st.tolist()


def test_every_status_in_one_call():
    #            unbound  bad  not-ok  applied  deferred  overflow (fits, R - req passes INT64_MAX)
    b = [-1, 2, 0, 0, 0, 1]
    rc = [1, 1, 1, 4, 7, -2]
    rm = [1, 1, 1, 4, 1, 0]
    ok = [1, 1, 0, 1, 1, 1]
    c, m, st = run([10, I64_MAX - 1], [10, 5], b, rc, rm, ok)
    assert st == [UNBOUND, BAD_NODE, NOT_OK, A, D, O]
    assert c == [6, I64_MAX - 1] and m == [6, 5]


def test_status_precedence_unbound_bad_node_not_ok():
    _, _, st = run([5], [5], [-3, 1, 7, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0])
    assert st == [UNBOUND, BAD_NODE, BAD_NODE, NOT_OK]


def test_skip_not_stop():
    c, m, st = run([10], [100], [0, 0, 0], [5, 9, 3], [1, 1, 1])
    assert st == [A, D, A] and c == [2] and m == [98]
    assert admitted_behind_deferred([0, 0, 0], st) == 1
    where = set()
    assert admitted_behind_deferred([1, 0, 1, 0, 1, 2, 2], [A, D, D, A, A, A, D], where) == 2 and where == {0, 1}


def test_exact_fill():
    k, r = 7, 13
    c, m, st = run([k * r], [k * r * 2], [0] * 12, [r] * 12, [2 * r] * 12)
    assert st == [A] * k + [D] * (12 - k) and c == [0] and m == [0]


def test_zero_request_on_zero_and_on_minus_one():
    c, m, st = run([0, -1, 0], [0, 0, -1], [0, 1, 2], [0, 0, 0], [0, 0, 0])
    assert st == [A, D, D] and c == [0, -1, 0] and m == [0, 0, -1]


def test_one_resource_fits_and_the_other_does_not():
    c, m, st = run([10, 10], [10, 10], [0, 1, 0, 1], [5, 11, 5, 1], [11, 5, 10, 1])
    assert st == [D, D, A, A] and c == [5, 9] and m == [0, 9]


def test_negative_request_grows_what_is_left_but_revives_nobody():
    c, m, st = run([4], [4], [0, 0, 0], [6, -3, 6], [1, 0, 1])
    assert st == [D, A, A] and c == [1] and m == [3]  # pod 0 stays deferred although 6 <= 7 after pod 1


def test_overflow_just_inside_and_one_past():
    # R - req == INT64_MAX exactly: admitted; one past: OVERFLOW, nothing changes, and the node goes on
    c, m, st = run([I64_MAX - 2], [0], [0], [-2], [0])
    assert st == [A] and c == [I64_MAX] and m == [0]
    c, m, st = run([I64_MAX - 2, 5], [7, I64_MAX], [0, 0, 1, 1, 1], [-3, 4, 1, 1, 5], [1, 1, -1, 2, 0])
    assert st == [O, A, O, A, D]
    assert c == [I64_MAX - 6, 4] and m == [6, I64_MAX - 2]
    c, m, st = run([0], [0], [0, 0], [I64_MIN, I64_MIN], [0, 0])  # 0 - INT64_MIN is one past INT64_MAX
    assert st == [O, O] and c == [0]
    c, m, st = run([I64_MIN], [0], [0, 0], [I64_MIN, I64_MAX], [0, 0])  # INT64_MIN fits INT64_MIN and leaves 0
    assert st == [A, D] and c == [0]


def test_a_lower_ineligible_pod_takes_no_place():
    c, m, st = run([5], [5], [0, 0, 0], [5, 5, 5], [5, 5, 5], [0, 1, 1])
    assert st == [NOT_OK, A, D] and c == [0] and m == [0]


def test_no_nodes():
    c, m, st = run([], [], [0, -1, 3], [1, 1, 1], [1, 1, 1])
    assert st == [BAD_NODE, UNBOUND, BAD_NODE] and c == [] and m == []
    c, m, st = run([3], [3], [], [], [])
    assert st == [] and c == [3]


def random_case(rng, n, p):
    b = rng.integers(-2, n + 2, p).astype(np.int32)
    return b, rng.integers(0, 5000, p).astype(np.int64), rng.integers(0, 1 << 33, p).astype(np.int64), (rng.random(p) > 0.1).astype(np.uint8)


def test_with_room_for_everything_it_is_the_summed_rule():
    rng = np.random.default_rng(1)
    for n, p in ((1, 50), (7, 300), (100, 2000)):
        b, rc, rm, ok = random_case(rng, n, p)
        cpu, mem = np.full(n, 1 << 50, dtype=np.int64), np.full(n, 1 << 60, dtype=np.int64)
        got, want = apply_while_fit_exact(cpu, mem, b, rc, rm, ok), apply_bindings_exact(cpu, mem, b, rc, rm, ok, 0)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert (want[2] == APPLIED).sum() >= 10  # (n = 1: a fifth of the draws name the node)
        assert longest_segment(b, n, ok) >= 2


def test_with_one_fitting_pod_per_node_it_is_first_per_node():
    rng = np.random.default_rng(2)
    n, p = 500, 400
    b = rng.permutation(n)[:p].astype(np.int32)  # every node at most once
    b[rng.random(p) < 0.1] = -1
    b[rng.random(p) < 0.05] = n + 3
    _, rc, rm, ok = random_case(rng, n, p)
    cpu, mem = rng.integers(5000, 1 << 20, n).astype(np.int64), rng.integers(1 << 33, 1 << 40, n).astype(np.int64)
    got, want = apply_while_fit_exact(cpu, mem, b, rc, rm, ok), apply_bindings_exact(cpu, mem, b, rc, rm, ok, APPLY_FIRST_PER_NODE)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert set(want[2].tolist()) == {APPLIED, UNBOUND, NOT_OK, BAD_NODE}


def tight_case():
    """three pods onto one node of which the middle one does not fit: the three rules leave three different columns"""
    return (np.array([10], dtype=np.int64), np.array([100], dtype=np.int64), np.array([0, 0, 0], dtype=np.int32),
            np.array([5, 9, 3], dtype=np.int64), np.array([1, 1, 1], dtype=np.int64), np.array([1, 1, 1], dtype=np.uint8))


def test_apply_exact_picks_the_rule_by_the_flags():
    args = tight_case()
    c, m, st = apply_exact(*args, WHILE_FIT)
    assert c.tolist() == [2] and m.tolist() == [98] and st.tolist() == [A, D, A]
    for g, w in zip(apply_exact(*args, WHILE_FIT), apply_while_fit_exact(*args)):
        assert np.array_equal(g, w)
    left = {WHILE_FIT: 2}
    for flags in (0, APPLY_FIRST_PER_NODE, APPLY_RELEASE, APPLY_FIRST_PER_NODE | APPLY_RELEASE):
        got, want = apply_exact(*args, flags), apply_bindings_exact(*args, flags)
        for g, w in zip(got, want):
            assert np.array_equal(g, w) and g.dtype == w.dtype
        left[flags] = int(got[0][0])
    assert left == {WHILE_FIT: 2, 0: -7, APPLY_FIRST_PER_NODE: 5, APPLY_RELEASE: 27, APPLY_FIRST_PER_NODE | APPLY_RELEASE: 15}  # no two rules alike
    assert apply_exact(*args[:5], None, WHILE_FIT)[2].tolist() == [A, D, A]  # ok=None passes through


@pytest.mark.parametrize("flags", [WHILE_FIT | APPLY_FIRST_PER_NODE, WHILE_FIT | APPLY_RELEASE, WHILE_FIT | 3, 0x04, 0x10, 0x0C, 1 << 31, -1])
def test_apply_exact_refuses_every_other_flag_set(flags):
    with pytest.raises(ValueError):
        apply_exact(*tight_case(), flags)


@pytest.mark.parametrize("flags", [WHILE_FIT, WHILE_FIT | APPLY_FIRST_PER_NODE, WHILE_FIT | APPLY_RELEASE, 0x04, 0x10, 1 << 31])
def test_the_summed_restatement_refuses_flags_it_does_not_restate(flags):
    """it used to ignore them: flags = 0x08 gave the flags = 0 rule, which agrees with the admission rule wherever everything fits"""
    with pytest.raises(ValueError):
        apply_bindings_exact(*tight_case(), flags)
    assert apply_bindings_exact(*tight_case(), flags & 3)[2].shape == (3,)  # the same call without the foreign bits is restated
