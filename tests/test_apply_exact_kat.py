"""Known answers, worked out by hand, for oracle/oracle_ref.py apply_bindings_exact: the exact-integer restatement every GPU test of
ksched_apply_bindings_device / ksched_apply_bindings_sharded* (and tools/fuzz_parity.py) takes its expected columns and statuses from.
No GPU."""
import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import _lib
from oracle import oracle_ref as R
from oracle.oracle_ref import apply_bindings_exact as exact

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
A, U, NO, D, O, BAD = R.APPLY_APPLIED, R.APPLY_UNBOUND, R.APPLY_NOT_OK, R.APPLY_DEFERRED, R.APPLY_OVERFLOW, R.APPLY_BAD_NODE
FPN, REL = R.APPLY_FIRST_PER_NODE, R.APPLY_RELEASE


def run(cpu, mem, b, rc, rm, ok=None, flags=0):
    c, m, st = exact(np.array(cpu, np.int64), np.array(mem, np.int64), np.array(b, np.int32), np.array(rc, np.int64), np.array(rm, np.int64),
                     None if ok is None else np.array(ok, np.uint8), flags)
    assert c.dtype == np.int64 and m.dtype == np.int64 and st.dtype == np.int32
    return c.tolist(), m.tolist(), st.tolist()


def test_constants_are_the_headers():
    assert (A, U, NO, D, O, BAD) == (_lib.APPLY_APPLIED, _lib.APPLY_UNBOUND, _lib.APPLY_NOT_OK, _lib.APPLY_DEFERRED, _lib.APPLY_OVERFLOW,
                                     _lib.APPLY_BAD_NODE)
    assert (FPN, REL) == (_lib.APPLY_FIRST_PER_NODE, _lib.APPLY_RELEASE)


def test_every_status():
    # node 0: pods 0 and 5 (10 + 1, 100 + 2); node 1: pod 4 overflows mem; pod 1 unbound, pod 2 past the last node, pod 3 not ok
    c, m, st = run([50, 60], [500, I64_MIN + 3], [0, -1, 2, 0, 1, 0], [10, 7, 7, 7, 1, 1], [100, 7, 7, 7, 4, 2], ok=[1, 1, 1, 0, 1, 1])
    assert st == [A, U, BAD, NO, O, A]
    assert c == [39, 60] and m == [398, I64_MIN + 3]
    # DEFERRED: with FIRST_PER_NODE only pod 0 lands on node 0
    c, m, st = run([50, 60], [500, 600], [0, 0, 1, 0], [10, 20, 30, 40], [1, 2, 3, 4], flags=FPN)
    assert st == [A, D, A, D]
    assert c == [40, 30] and m == [499, 597]


@pytest.mark.parametrize("why", ["unbound", "bad node", "not ok"])
def test_first_per_node_skips_a_lower_ineligible_pod(why):
    """pod 0 is ineligible (as `why` says) but names node 0 or not at all; the lowest ELIGIBLE pod on node 0 is pod 1"""
    b = {"unbound": [-1, 0, 0], "bad node": [2, 0, 0], "not ok": [0, 0, 0]}[why]
    ok = [0, 1, 1] if why == "not ok" else None
    c, m, st = run([100, 100], [100, 100], b, [5, 6, 7], [50, 60, 70], ok=ok, flags=FPN)
    assert st == [{"unbound": U, "bad node": BAD, "not ok": NO}[why], A, D]
    assert c == [94, 100] and m == [40, 100]


def test_release_adds_back():
    c, m, st = run([1, -5], [0, 0], [1, 1, 0], [3, 4, 2], [-10, 20, 1], flags=REL)
    assert st == [A, A, A]
    assert c == [3, 2] and m == [1, 10]
    c, m, st = run([1, 2], [3, 4], [0, 0, 1], [5, 6, 7], [8, 9, 10], flags=FPN | REL)
    assert st == [A, D, A]
    assert c == [6, 9] and m == [11, 14]


def test_the_int64_ends_are_inside_and_one_past_is_outside():
    # node 0: -1 - INT64_MAX = INT64_MIN exactly; node 1: -2 - INT64_MAX = INT64_MIN - 1
    c, m, st = run([-1, -2], [0, 0], [0, 1], [I64_MAX, I64_MAX], [0, 0])
    assert st == [A, O]
    assert c == [I64_MIN, -2] and m == [0, 0]
    c, m, st = run([0, 1], [5, 5], [0, 1], [I64_MIN + 1, I64_MIN + 1], [0, 0])  # 0 - (INT64_MIN + 1) = INT64_MAX; 1 - ... = INT64_MAX + 1
    assert st == [A, O]
    assert c == [I64_MAX, 1] and m == [5, 5]
    c, m, st = run([0, 1], [0, 0], [0, 1], [0, 0], [I64_MAX, I64_MAX], flags=REL)  # mem 0 + INT64_MAX on both nodes
    c2, m2, st2 = run([0, 0], [0, 1], [0, 1], [0, 0], [I64_MAX, I64_MAX], flags=REL)  # node 1: 1 + INT64_MAX, one past
    assert st == [A, A] and c == [0, 1] and m == [I64_MAX, I64_MAX]
    assert st2 == [A, O] and c2 == [0, 0] and m2 == [I64_MAX, 1]


def test_overflow_in_cpu_alone_leaves_mem_unchanged_too():
    c, m, st = run([I64_MIN + 1, 7], [1000, 1000], [0, 0, 1], [1, 1, 1], [10, 20, 30])  # cpu of node 0: INT64_MIN + 1 - 2
    assert st == [O, O, A]
    assert c == [I64_MIN + 1, 6] and m == [1000, 970]


def test_a_sum_that_leaves_int64_on_the_way_but_ends_inside_it():
    big = 1 << 62
    # requests 2^62, 2^62, 2^62, -2^62, -2^62, -2^62 on node 0: the running sum reaches 3 * 2^62 > INT64_MAX and comes back to 0
    c, m, st = run([5], [9], [0] * 6, [big, big, big, -big, -big, -big], [1, 1, 1, 1, 1, 1])
    assert st == [A] * 6
    assert c == [5] and m == [3]
    # the whole batch's sum counts, not the order: INT64_MAX + INT64_MAX - INT64_MAX
    c, m, st = run([0], [0], [0, 0, 0], [I64_MAX, I64_MAX, -I64_MAX], [0, 0, 0])
    assert st == [A] * 3 and c == [-I64_MAX] and m == [0]


@pytest.mark.parametrize("okv", [1, 2, 255])
def test_any_nonzero_ok_counts_as_landed(okv):
    c, m, st = run([10], [10], [0, 0], [1, 2], [3, 4], ok=[okv, 0])
    assert st == [A, NO]
    assert c == [9] and m == [7]


def test_no_nodes():
    c, m, st = run([], [], [0, -1, 3], [1, 1, 1], [1, 1, 1], flags=FPN)
    assert c == [] and m == [] and st == [BAD, U, BAD]
    c, m, st = run([], [], [], [], [])
    assert c == [] and m == [] and st == []


def test_no_pods_changes_nothing():
    c, m, st = run([I64_MAX, I64_MIN], [3, 4], [], [], [], flags=REL)
    assert c == [I64_MAX, I64_MIN] and m == [3, 4] and st == []


def test_the_gpu_tests_see_the_same_function():
    """tests/test_gpu_apply_bindings.py (and through it tests/apply_sharded_worker.py) uses this restatement under its old name"""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_apply_bindings.py")).read()
    names = {(n.module, a.name, a.asname) for n in ast.walk(ast.parse(src)) if isinstance(n, ast.ImportFrom) for a in n.names}
    assert ("oracle.oracle_ref", "apply_bindings_exact", "restate") in names
