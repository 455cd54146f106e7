"""KSCHED_SEL_TERMS restated in numpy (include/ksched.h, extension E10): the expected mask of every test of a tagged call with a term count.

selterms_mask(labels, entries): labels [k][n] are the snapshot's label ids; entries [T][k][p] (or [T * k][p]) the batch's tagged selector
entries, T rows per pod.  From the header: row(pod) = valid bits AND ( OR over t of ( AND over k of [E9's table for entries[t][k][pod] and
labels[k][node]] ) ) -- the OR over t of seltag_ref.pass_bits(labels, entries[t]), packed into uint64 words with the bits at or beyond n
zero.  entries None, or no keys: every node passes.  Written from the header, independent of csrc/sel_terms.hpp and of oracle/.  A plain
module: no test, no fixture."""
import numpy as np

from tests import seltag_ref

SHIFT = 20
MASK = 0x00F00000
MAX_TERMS = 15
NEVER = seltag_ref.NEVER


def field(t):
    """the flag field of a call with t terms per pod"""
    assert 1 <= t <= MAX_TERMS
    return t << SHIFT


def as_terms(labels, entries):
    """entries as [T][k][p], from [T][k][p] or [T * k][p]"""
    labels = np.asarray(labels)
    entries = np.asarray(entries)
    k = labels.shape[0]
    if entries.ndim == 2:
        assert k > 0 and entries.shape[0] % k == 0, (entries.shape, labels.shape)
        entries = entries.reshape(entries.shape[0] // k, k, entries.shape[1])
    assert entries.ndim == 3 and entries.shape[1] == k, (entries.shape, labels.shape)
    return entries


def pass_bits(labels, entries) -> np.ndarray:
    """[p, n] bool: the OR over the terms of the AND over the keys of E9's table"""
    labels = np.asarray(labels)
    if entries is None or labels.ndim != 2 or labels.shape[0] == 0:
        return seltag_ref.pass_bits(labels, entries)  # (all ones, [p, n]; p is the entries' last axis)
    entries = as_terms(labels, entries)
    ok = np.zeros((entries.shape[2], labels.shape[1]), dtype=bool)
    for t in range(entries.shape[0]):
        ok |= seltag_ref.pass_bits(labels, entries[t])
    return ok


def term_masks(labels, entries):
    """the packed rows of every single term, [T][p, W]"""
    return [seltag_ref.seltag_mask(labels, e) for e in as_terms(labels, entries)]


def selterms_mask(labels, entries, p: int = None) -> np.ndarray:
    """packed rows [p, W]; `p` is needed only where entries is None"""
    if entries is None:
        return seltag_ref.seltag_mask(labels, None, p=p)
    return seltag_ref.pack(pass_bits(labels, entries))


def selterms_and_term_masks(labels, entries):
    """(selterms_mask(labels, entries), term_masks(labels, entries)) with every term's bits computed once: for callers that want the
    single terms' rows beside the call's on large tables"""
    labels = np.asarray(labels)
    entries = as_terms(labels, entries)
    bits = [seltag_ref.pass_bits(labels, e) for e in entries]
    ok = np.zeros((entries.shape[2], labels.shape[1]), dtype=bool)
    for b in bits:
        ok |= b
    return seltag_ref.pack(ok), [seltag_ref.pack(b) for b in bits]


def and_of_ors_mask(labels, entries, keys_per_pass: int = 8) -> np.ndarray:
    """What a WRONG kernel computes that ORs the terms pass by pass (`keys_per_pass` keys at a time) and ANDs the passes' words: the formula
    the header's layout does NOT mean.  (A0 & A1) | (B0 & B1) against (A0 | B0) & (A1 | B1)."""
    labels = np.asarray(labels)
    entries = as_terms(labels, entries)
    k = labels.shape[0]
    ok = np.ones((entries.shape[2], labels.shape[1]), dtype=bool)
    for k0 in range(0, k, keys_per_pass):
        part = np.zeros_like(ok)
        for t in range(entries.shape[0]):
            part |= seltag_ref.pass_bits(labels[k0:k0 + keys_per_pass], entries[t][k0:k0 + keys_per_pass])
        ok &= part
    return seltag_ref.pack(ok)
