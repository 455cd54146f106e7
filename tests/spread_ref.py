"""KSCHED_PICK_SPREAD restated in numpy (include/ksched.h): the expected bindings of every spread-pick test.

For pod i with the d 32-bit draws draws[i, :]: candidate j is what KSCHED_PICK_UNIFORM gives for draw j (tests/uniform_ref.py, column by
column); the binding is -1 when the pod has no feasible node, else the candidate with the largest signed (avail_mem, avail_cpu), memory
first, the lowest node index among equals.  Exact integers throughout: only comparisons of int64 values, no arithmetic on them."""
import numpy as np

from tests.uniform_ref import uniform_pick


def spread_candidates(mask: np.ndarray, draws: np.ndarray, n: int) -> np.ndarray:
    """mask [p, >= ceil(n / 64)] uint64, draws [p, d >= 1] (values < 2^32), n nodes -> int32 [p, d]; a row is all -1 or has no -1."""
    draws = np.asarray(draws)
    assert draws.ndim == 2 and draws.shape[1] >= 1
    return np.stack([uniform_pick(mask, draws[:, j], n) for j in range(draws.shape[1])], axis=1)


def spread_candidates_listed(mask: np.ndarray, draws: np.ndarray, n: int) -> np.ndarray:
    """spread_candidates by another route, for the large shapes of the GPU tests (uniform_pick builds a [p, n] int64 table per column):
    the feasible nodes of all rows listed once in ascending order, candidate (i, j) read at position k_ij of row i's stretch of the list.
    tests/test_spread_restatement.py pins it equal to spread_candidates."""
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    draws = np.asarray(draws)
    p, d = draws.shape
    assert mask.ndim == 2 and mask.shape[0] == p and d >= 1
    out = np.full((p, d), -1, dtype=np.int32)
    W = (int(n) + 63) // 64
    if p == 0 or W == 0:
        return out
    assert mask.shape[1] >= W
    bits = np.unpackbits(np.ascontiguousarray(mask[:, :W]).view(np.uint8), axis=1, bitorder="little")[:, :n]
    c = bits.sum(axis=1, dtype=np.int64)
    listed = np.flatnonzero(bits)  # row-major: row i's feasible nodes, ascending, at [start[i], start[i] + c[i]) as i * n + node
    start = np.cumsum(c) - c
    k = (draws.astype(np.uint64) * c.astype(np.uint64)[:, None]) >> np.uint64(32)  # < c where c > 0
    some = c > 0
    at = start[some, None] + k[some].astype(np.int64)
    out[some] = (listed[at] - np.nonzero(some)[0][:, None] * int(n)).astype(np.int32)
    return out


def best_of(cand: np.ndarray, avail_mem: np.ndarray, avail_cpu: np.ndarray) -> np.ndarray:
    """cand int [p, d] of node indices (a row of -1: no feasible node) -> int32 [p]: the arg-max of (mem, cpu, -node) over every row."""
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
    lowest = np.iinfo(np.int64).min
    keep = m == m.max(axis=1, keepdims=True)                                   # the largest memory
    keep &= q == np.where(keep, q, lowest).max(axis=1, keepdims=True)          # among those the largest cpu
    node = np.where(keep, v, np.iinfo(np.int64).max).min(axis=1)               # among those the lowest node
    out[some] = node[some].astype(np.int32)
    return out


def spread_pick(mask: np.ndarray, draws: np.ndarray, n: int, avail_mem: np.ndarray, avail_cpu: np.ndarray) -> np.ndarray:
    """mask [p, >= ceil(n / 64)] uint64, draws [p, d], the snapshot's [n] int64 columns -> int32 [p]."""
    return best_of(spread_candidates(mask, draws, n), avail_mem, avail_cpu)


def spread_pick_blocks(mask: np.ndarray, draws: np.ndarray, n: int, avail_mem: np.ndarray, avail_cpu: np.ndarray, cells: int = 1 << 24) -> np.ndarray:
    """spread_pick by the listed route in blocks of pods (the counterpart of uniform_ref.uniform_pick_blocks): spread_candidates_listed
    unpacks a [pods, n] table of bits, so a block is at most `cells` entries of it.  tests/test_spread_restatement.py pins it equal to
    spread_pick."""
    draws = np.asarray(draws)
    p = mask.shape[0]
    step = max(1, cells // max(int(n), 1))
    if p <= step:
        return best_of(spread_candidates_listed(mask, draws, n), avail_mem, avail_cpu)
    return np.concatenate([best_of(spread_candidates_listed(mask[lo:lo + step], draws[lo:lo + step], n), avail_mem, avail_cpu)
                           for lo in range(0, p, step)])
