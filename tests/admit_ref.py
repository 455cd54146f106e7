"""KSCHED_APPLY_WHILE_FIT restated in Python integers (include/ksched.h): the expected columns and statuses of every admit test.

One pass over the pods in ascending index -- per node that IS the node's eligible pods in ascending pod index, and nodes do not touch one
another.  A pod is eligible when 0 <= binding < n and ok (when given) is nonzero; the statuses UNBOUND (binding < 0), BAD_NODE
(binding >= n) and NOT_OK precede in that order.  An eligible pod is admitted iff both requests are <= what is left of its node (the
compares of can_pod_fit, src/predicates.rs:37-42); an admitted pod takes its requests off both resources; a pod that fits but would take
either resource past INT64_MAX (a negative request) reports OVERFLOW and changes nothing; every other pod is DEFERRED, changes nothing,
and the walk goes on behind it.  No numpy arithmetic: nothing can wrap."""
import numpy as np

from oracle.oracle_ref import APPLY_FIRST_PER_NODE, APPLY_RELEASE, apply_bindings_exact

WHILE_FIT = 0x08  # KSCHED_APPLY_WHILE_FIT
APPLIED, UNBOUND, NOT_OK, DEFERRED, OVERFLOW, BAD_NODE = 0, 1, 2, 3, 4, 5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def apply_while_fit_exact(cpu, mem, bindings, req_cpu, req_mem, ok=None):
    """-> (new cpu, new mem, status) as int64 / int64 / int32 numpy arrays"""
    cpu, mem = [int(x) for x in cpu], [int(x) for x in mem]
    b_, rc, rm = np.asarray(bindings).tolist(), np.asarray(req_cpu).tolist(), np.asarray(req_mem).tolist()
    okl = None if ok is None else np.asarray(ok).tolist()
    n, status = len(cpu), []
    for i, b in enumerate(b_):
        if b < 0:
            status.append(UNBOUND)
        elif b >= n:
            status.append(BAD_NODE)
        elif okl is not None and okl[i] == 0:
            status.append(NOT_OK)
        elif rc[i] <= cpu[b] and rm[i] <= mem[b]:
            nc, nm = cpu[b] - rc[i], mem[b] - rm[i]  # (never below INT64_MIN: req <= R)
            if nc > I64_MAX or nm > I64_MAX:
                status.append(OVERFLOW)
            else:
                cpu[b], mem[b] = nc, nm
                status.append(APPLIED)
        else:
            status.append(DEFERRED)
    return np.array(cpu, dtype=np.int64).reshape(-1), np.array(mem, dtype=np.int64).reshape(-1), np.array(status, dtype=np.int32).reshape(-1)


def apply_exact(cpu, mem, bindings, req_cpu, req_mem, ok, flags):
    """one apply restated by its flags: WHILE_FIT alone -> apply_while_fit_exact, any combination of FIRST_PER_NODE / RELEASE ->
    oracle_ref.apply_bindings_exact; everything else (WHILE_FIT with another flag, an unknown bit) is refused, as the library refuses it"""
    if flags == WHILE_FIT:
        return apply_while_fit_exact(cpu, mem, bindings, req_cpu, req_mem, ok)
    if flags & ~(APPLY_FIRST_PER_NODE | APPLY_RELEASE):
        raise ValueError(f"no restatement of an apply with flags {flags:#x}")
    return apply_bindings_exact(cpu, mem, bindings, req_cpu, req_mem, ok, flags)


def longest_segment(bindings, n, ok=None):
    """the most eligible pods bound to one node"""
    b = np.asarray(bindings)
    elig = (b >= 0) & (b < n) & (True if ok is None else np.asarray(ok) != 0)
    return int(np.bincount(b[elig], minlength=1).max()) if elig.any() else 0


def admitted_behind_deferred(bindings, status, nodes=None):
    """pods admitted although a lower pod of their node was DEFERRED: the skip rule seen.  nodes: a set that receives the nodes where
    that happened"""
    seen, k = set(), 0
    for b, s in zip(np.asarray(bindings).tolist(), np.asarray(status).tolist()):
        if s == DEFERRED:
            seen.add(b)
        elif s == APPLIED and b in seen:
            k += 1
            if nodes is not None:
                nodes.add(b)
    return k
