"""KSCHED_SELOP_TAGGED restated in numpy (include/ksched.h, extension E9): the expected mask of every tagged-call test.

seltag_mask(labels, entries): labels [k][n] are the snapshot's label ids, the node's WHOLE 32-bit id (0 = the node does not carry the
key); entries [k][p] the batch's tagged selector entries, e = tag << 29 | id.  Per (pod, key, node), from the header's table:

    e == 0        passes (the pod does not constrain the key)
    tag 0 EQ      v == id
    tag 1 NE      v != id                (an absent node passes)
    tag 2 EXISTS  v != 0                 (the id is not looked at)
    tag 3 ABSENT  v == 0                 (the id is not looked at)
    tag 4 GT      v != 0 and v > id
    tag 5 LT      v != 0 and v < id
    tag 6, 7      nowhere                (NEVER = 0xFFFFFFFF is tag 7)

-- the compares between the node's whole id and the 29-bit id field as unsigned numbers (here: in uint64, which cannot wrap).  The pod's row
is the AND over the keys, packed into uint64 words with the bits at or beyond n zero.  entries None, or no keys: every node passes.
Written from the header's table, independent of csrc/sel_tags.hpp and of oracle/.  A plain module: no test, no fixture."""
import numpy as np

TAGGED = 0x40000
SHIFT = 29
ID_MASK = 0x1FFFFFFF
EQ, NE, EXISTS, ABSENT, GT, LT = range(6)
TAGS = (EQ, NE, EXISTS, ABSENT, GT, LT)
NAMES = {EQ: "eq", NE: "ne", EXISTS: "exists", ABSENT: "absent", GT: "gt", LT: "lt"}
NEVER = 0xFFFFFFFF


def entry(tag, ident):
    """tag << 29 | id as uint32 (array or scalar); no check: the tests build tags 6 and 7 with it too"""
    return ((np.asarray(tag, dtype=np.uint64) << np.uint64(SHIFT)) | (np.asarray(ident, dtype=np.uint64) & np.uint64(ID_MASK))).astype(np.uint32)


def pair(e, v) -> np.ndarray:
    """the table for entries e and node ids v (broadcast against each other), bool"""
    e = np.asarray(e, dtype=np.uint64)
    v = np.asarray(v, dtype=np.uint64)
    tag = e >> np.uint64(SHIFT)
    ident = e & np.uint64(ID_MASK)
    present = v != 0
    out = np.zeros(np.broadcast(e, v).shape, dtype=bool)  # tags 6 and 7: nowhere
    for t, term in ((EQ, v == ident), (NE, v != ident), (EXISTS, present & (e == e)), (ABSENT, ~present & (e == e)),
                    (GT, present & (v > ident)), (LT, present & (v < ident))):
        out = np.where(tag == t, term, out)
    return np.where(e == 0, True, out)


def pass_bits(labels, entries) -> np.ndarray:
    """[p, n] bool: the AND over the keys of the header's table"""
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
        if pods.size:
            ok[pods] &= pair(entries[k][pods][:, None], labels[k][None, :])
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


def seltag_mask(labels, entries, p: int = None) -> np.ndarray:
    """packed rows [p, W]; `p` is needed only where entries is None"""
    bits = pass_bits(labels, entries)
    if entries is None:
        n = np.asarray(labels).shape[1] if np.asarray(labels).ndim == 2 else 0
        bits = np.ones((int(p), n), dtype=bool)
    return pack(bits)
