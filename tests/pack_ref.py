"""KSCHED_PICK_PACK restated in numpy (include/ksched.h): the expected bindings of every pack-pick test.

For pod i with the d 32-bit draws draws[i, :]: candidate j is what KSCHED_PICK_UNIFORM gives for draw j (tests/spread_ref.py's two routes
to the candidates); the binding is -1 when the pod has no feasible node, else the candidate with the smallest signed (avail_mem,
avail_cpu), memory first, the lowest node index among equals.  Only comparisons of int64 values, no arithmetic on them."""
import numpy as np

from tests.spread_ref import spread_candidates, spread_candidates_listed


def tightest_of(cand: np.ndarray, avail_mem: np.ndarray, avail_cpu: np.ndarray) -> np.ndarray:
    """cand int [p, d] of node indices (a row of -1: no feasible node) -> int32 [p]: the arg-min of (mem, cpu, node) over every row."""
    cand = np.asarray(cand, dtype=np.int64)
    p = cand.shape[0]
    out = np.full((p,), -1, dtype=np.int32)
    if p == 0:
        return out
    some = cand[:, 0] >= 0
    mem, cpu = np.asarray(avail_mem, dtype=np.int64), np.asarray(avail_cpu, dtype=np.int64)
    if not some.any() or mem.size == 0:
        return out
    v = np.where(cand >= 0, cand, 0)
    m, q = mem[v], cpu[v]
    highest = np.iinfo(np.int64).max
    keep = m == m.min(axis=1, keepdims=True)                                   # the smallest memory
    keep &= q == np.where(keep, q, highest).min(axis=1, keepdims=True)         # among those the smallest cpu
    node = np.where(keep, v, highest).min(axis=1)                              # among those the lowest node
    out[some] = node[some].astype(np.int32)
    return out


def pack_pick(mask: np.ndarray, draws: np.ndarray, n: int, avail_mem: np.ndarray, avail_cpu: np.ndarray) -> np.ndarray:
    """mask [p, >= ceil(n / 64)] uint64, draws [p, d], the snapshot's [n] int64 columns -> int32 [p]."""
    return tightest_of(spread_candidates(mask, draws, n), avail_mem, avail_cpu)


def pack_pick_listed(mask: np.ndarray, draws: np.ndarray, n: int, avail_mem: np.ndarray, avail_cpu: np.ndarray) -> np.ndarray:
    """pack_pick with the candidates by spread_ref's listed route (no [p, n] int64 table per column): for the longer rows of the GPU tests.
    tests/test_pack_restatement.py pins it equal to pack_pick."""
    return tightest_of(spread_candidates_listed(mask, draws, n), avail_mem, avail_cpu)
