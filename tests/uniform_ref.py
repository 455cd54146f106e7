"""KSCHED_PICK_UNIFORM restated in numpy (include/ksched.h): the expected bindings of every uniform-pick test.

For pod i with c = the set bits of mask row i over nodes [0, n) and the 32-bit draw u = draws[i]:
binding = -1 when c == 0, else the node index of set bit number k = (u * c) >> 32 (0-based, ascending).  Bits at or beyond n and
words at or beyond ceil(n / 64) are ignored.  Exact integers throughout (u * c < 2^64)."""
import numpy as np


def uniform_pick(mask: np.ndarray, draws: np.ndarray, n: int) -> np.ndarray:
    """mask [p, >= ceil(n / 64)] uint64, draws [p] (values < 2^32), n nodes -> int32 [p]."""
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    draws = np.asarray(draws)
    p = mask.shape[0]
    assert mask.ndim == 2 and draws.shape == (p,)
    out = np.full((p,), -1, dtype=np.int32)
    W = (int(n) + 63) // 64
    if p == 0 or W == 0:
        return out
    assert mask.shape[1] >= W
    bits = np.unpackbits(np.ascontiguousarray(mask[:, :W]).view(np.uint8), axis=1, bitorder="little")[:, :n]  # [p, n] of 0 / 1
    rank = np.cumsum(bits, axis=1, dtype=np.int64)  # set bits up to and including each node
    c = rank[:, -1]
    k = (draws.astype(np.uint64) * c.astype(np.uint64)) >> np.uint64(32)  # < c where c > 0
    # the first node whose inclusive rank exceeds k is set bit number k
    node = (rank > k.astype(np.int64)[:, None]).argmax(axis=1)
    out[c > 0] = node[c > 0].astype(np.int32)
    return out


def uniform_pick_blocks(mask: np.ndarray, draws: np.ndarray, n: int, cells: int = 1 << 24) -> np.ndarray:
    """uniform_pick in blocks of pods: the restatement holds a [pods, n] int64 table, so a block is at most `cells` entries of it."""
    p = mask.shape[0]
    step = max(1, cells // max(int(n), 1))
    if p <= step:
        return uniform_pick(mask, draws, n)
    draws = np.asarray(draws)
    return np.concatenate([uniform_pick(mask[lo:lo + step], draws[lo:lo + step], n) for lo in range(0, p, step)])
