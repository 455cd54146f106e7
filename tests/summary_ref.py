"""The yardstick of the ksched_summarize* tests: per-pod node counts by reason, restated in numpy on top of the EXISTING oracle.

Three oracle.capi.eval_encoded calls with flags = FIT, SEL, TAINT alone give the masks F, S, T ("predicates not selected are
treated as true": a predicate that the request leaves out is the all-nodes mask), and then, with the precedence of
check_node_validity (src/predicates.rs:63-77: resources :68-70, then the selector :72-74, then the taint extension),

    ok = popcount(F & S & T)    resources = N - popcount(F)    selector = popcount(F & ~S)    taint = popcount(F & S & ~T)

tests/test_summary_restatement.py pins this module against oracle.capi.check_node_validity pair by pair.  Nothing here touches the
library under test.
"""
from __future__ import annotations

import numpy as np

from oracle import capi

FIT, SEL, TAINT = 0x01, 0x02, 0x04
WORDS = 4  # [ok, NotEnoughResources, NodeSelectorMismatch, TaintNotTolerated] = REASON_* order


def popcount_rows(m: np.ndarray) -> np.ndarray:
    """[p, W] uint64 -> [p] set bits per row"""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(m).sum(axis=1, dtype=np.int64)
    return np.unpackbits(np.ascontiguousarray(m).view(np.uint8), axis=1).sum(axis=1, dtype=np.int64)


def _full_mask(p: int, n: int) -> np.ndarray:
    W = (n + 63) // 64
    m = np.full((p, W), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    if n % 64:
        m[:, -1] = np.uint64((1 << (n % 64)) - 1)
    return m


def masks(avail_cpu, avail_mem, label_ids, taints, req_cpu, req_mem, sel_ids, tolerations, flags: int):
    """(F, S, T) of a batch, each from ONE oracle call with that predicate alone; a predicate not in `flags` is all nodes."""
    n, p = len(avail_cpu), len(req_cpu)
    out = []
    for bit in (FIT, SEL, TAINT):
        if flags & bit:
            m, _, _ = capi.eval_encoded(avail_cpu, avail_mem, label_ids, taints, req_cpu, req_mem, sel_ids, tolerations, None, bit)
        else:
            m = _full_mask(p, n)
        out.append(m)
    return tuple(out)


def counts_from_masks(F, S, T, n: int) -> np.ndarray:
    out = np.empty((F.shape[0], WORDS), dtype=np.uint32)
    FS = F & S
    out[:, 0] = popcount_rows(FS & T)
    out[:, 1] = n - popcount_rows(F)
    out[:, 2] = popcount_rows(F & ~S)
    out[:, 3] = popcount_rows(FS & ~T)
    return out


def expected_counts(avail_cpu, avail_mem, label_ids, taints, req_cpu, req_mem, sel_ids, tolerations, flags: int, block: int = 8192) -> np.ndarray:
    """[p, 4] uint32, computed in row blocks (three full-size masks of a 125 k x 50 k batch would be 2.4 GB at once)."""
    n, p = len(avail_cpu), len(req_cpu)
    out = np.empty((p, WORDS), dtype=np.uint32)
    req_cpu, req_mem = np.asarray(req_cpu), np.asarray(req_mem)
    for lo in range(0, p, block):
        hi = min(p, lo + block)
        sel = None if sel_ids is None else np.ascontiguousarray(np.asarray(sel_ids)[:, lo:hi])
        tol = None if tolerations is None else np.asarray(tolerations)[lo:hi]
        F, S, T = masks(avail_cpu, avail_mem, label_ids, taints, req_cpu[lo:hi], req_mem[lo:hi], sel, tol, flags)
        out[lo:hi] = counts_from_masks(F, S, T, n)
    return out


def cluster_expected(c, flags: int, lo: int = 0, hi=None) -> np.ndarray:
    """expected_counts for pods [lo, hi) of a synth.Cluster"""
    hi = c.P if hi is None else hi
    return expected_counts(c.avail_cpu, c.avail_mem, c.node_labels if c.n_keys else None, c.node_taints if c.n_taints else None,
                           c.req_cpu[lo:hi], c.req_mem[lo:hi], np.ascontiguousarray(c.pod_sel[:, lo:hi]) if c.n_keys else None,
                           c.pod_tol[lo:hi] if c.n_taints else None, flags)
