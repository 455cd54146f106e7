"""KSCHED_SELOP_EXISTS / _GT / _LT restated in numpy (include/ksched.h, extension E8): the expected mask of every operator-call test.

selop_mask(labels, entries, op, n): labels [k][n] are the snapshot's label ids (0 = the node does not carry the key), entries [k][p] the
batch's selector entries (0 = the pod does not constrain the key, NEVER = matches nothing).  Per (pod, key, node) a constrained key passes
where the node carries the key and, for GT / LT, its id lies above / below the entry -- ids compared as unsigned 32-bit numbers (here:
as Python-sized integers in uint64, which cannot wrap).  The pod's row is the AND over the keys, packed into uint64 words with the bits at
or beyond n zero.  entries None, or no keys: every node passes.  Written from the header's table, independent of csrc/sel_ops.hpp and of
oracle/.  A plain module: no test, no fixture."""
import numpy as np

EXISTS, GT, LT = 0x4000, 0x8000, 0x10000
OPS = (EXISTS, GT, LT)
NAMES = {EXISTS: "exists", GT: "gt", LT: "lt"}
NEVER = 0xFFFFFFFF


def pass_bits(labels, entries, op: int) -> np.ndarray:
    """[p, n] bool: the AND over the keys of the header's table"""
    if op not in OPS:
        raise ValueError(f"op: expected one of {OPS}, got {op}")
    labels = np.asarray(labels, dtype=np.uint64)
    n = labels.shape[1] if labels.ndim == 2 else 0
    if entries is None or labels.ndim != 2 or labels.shape[0] == 0:
        p = 0 if entries is None else np.asarray(entries).shape[-1]
        return np.ones((p, n), dtype=bool)
    entries = np.asarray(entries, dtype=np.uint64)
    assert entries.ndim == 2 and entries.shape[0] == labels.shape[0], (entries.shape, labels.shape)
    p = entries.shape[1]
    ok = np.ones((p, n), dtype=bool)
    for k in range(labels.shape[0]):
        pods = np.nonzero(entries[k])[0]  # e == 0: the pod does not constrain key k -- its row is left as it is
        if pods.size == 0:
            continue
        e = entries[k][pods][:, None]  # [pods, 1]
        v = labels[k][None, :]         # [1, n]
        present = v != 0
        if op == EXISTS:
            term = np.broadcast_to(present, (pods.size, n))
        elif op == GT:
            term = present & (v > e)
        else:
            term = present & (v < e)
        ok[pods] &= np.where(e == NEVER, False, term)
    return ok


def pack(bits: np.ndarray) -> np.ndarray:
    """[p, n] bool -> [p, ceil(n / 64)] uint64: bit (node % 64) of word (node / 64), padding bits zero"""
    p, n = bits.shape
    W = (n + 63) // 64
    if W == 0:
        return np.zeros((p, 0), dtype=np.uint64)
    padded = np.zeros((p, W * 64), dtype=np.uint8)
    padded[:, :n] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(p, W)


def selop_mask(labels, entries, op: int, p: int = None) -> np.ndarray:
    """packed rows [p, W]; `p` is needed only where entries is None"""
    bits = pass_bits(labels, entries, op)
    if entries is None:
        n = np.asarray(labels).shape[1] if np.asarray(labels).ndim == 2 else 0
        bits = np.ones((int(p), n), dtype=bool)
    return pack(bits)
