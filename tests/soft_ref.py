"""KSCHED_COMBINE_SOFT restated in numpy (include/ksched.h, extension E7): the expected mask of every soft-combine test.

soft_combine(old, new, op, n): per pod row, r = tests/combine_ref.py's combine of the row (old & new or old & ~new over the words [0, W), the
last word ANDed with the valid-bits word of n); where r has a set bit the row is r, elsewhere it is old' -- the old row with the bits at or
beyond n cleared.  `new` is feasible(this call): what the same call without any combine flag writes.  decisions() names what happened to
every row.  Only bitwise operations on uint64 words.  A plain module: no test, no fixture."""
import numpy as np

from tests import combine_ref

SOFT = 0x2000
AND, ANDNOT = combine_ref.AND, combine_ref.ANDNOT
OPS = (AND, ANDNOT)
NAMES = {AND: "and", ANDNOT: "andnot"}
NARROWED, DROPPED, EMPTY = 0, 1, 2


def old_prime(old: np.ndarray, n: int) -> np.ndarray:
    """the caller's rows with the bits at or beyond n in the last word cleared (a new array)"""
    out = np.array(old, dtype=np.uint64)
    if out.shape[1]:
        out[:, -1] &= np.uint64(combine_ref.valid_bits_word(n))
    return out


def soft_combine(old: np.ndarray, new: np.ndarray, op: int, n: int) -> np.ndarray:
    """old, new [p, W] uint64 with W = ceil(n / 64), op AND or ANDNOT (with or without the SOFT bit) -> [p, W] uint64 (a new array)."""
    op = int(op) & ~SOFT
    if op not in OPS:
        raise ValueError(f"op: expected one of {OPS}, got {op}")
    r = combine_ref.combine(old, new, op, n)
    keep = r.any(axis=1)
    return np.where(keep[:, None], r, old_prime(old, n))


def decisions(old: np.ndarray, new: np.ndarray, op: int, n: int) -> np.ndarray:
    """[p] of NARROWED (r has a set bit: the row became r), DROPPED (r is empty, old' is not: the row kept old') and EMPTY (old' is)"""
    r = combine_ref.combine(old, new, int(op) & ~SOFT, n)
    return np.where(r.any(axis=1), NARROWED, np.where(old_prime(old, n).any(axis=1), DROPPED, EMPTY))
