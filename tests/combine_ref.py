"""KSCHED_COMBINE_AND / _OR / _ANDNOT restated in numpy (include/ksched.h, extension E6): the expected mask of every combine test.

combine(old, new, op, n): per pod row, words [0, W) of `old` combined with `new` -- old & new, old | new, old & ~new -- and the row's last
word ANDed with the valid-bits word of n, so bits at or beyond n come out zero whatever `old` held there.  `new` is feasible(this call):
what the same call without the combine flag writes.  Only bitwise operations on uint64 words.  A plain module: no test, no fixture."""
import numpy as np

AND, OR, ANDNOT = 0x200, 0x400, 0x800
OPS = (AND, OR, ANDNOT)
NAMES = {AND: "and", OR: "or", ANDNOT: "andnot"}


def valid_bits_word(n: int) -> int:
    """the bits of a row's last word that stand for nodes below n (n >= 1)"""
    return (1 << (n % 64)) - 1 if n % 64 else (1 << 64) - 1


def combine(old: np.ndarray, new: np.ndarray, op: int, n: int) -> np.ndarray:
    """old, new [p, W] uint64 with W = ceil(n / 64), op one of AND / OR / ANDNOT -> [p, W] uint64 (a new array)."""
    old = np.asarray(old, dtype=np.uint64)
    new = np.asarray(new, dtype=np.uint64)
    W = (int(n) + 63) // 64
    assert old.shape == new.shape and old.ndim == 2 and old.shape[1] == W, (old.shape, new.shape, W)
    if op == AND:
        out = old & new
    elif op == OR:
        out = old | new
    elif op == ANDNOT:
        out = old & ~new
    else:
        raise ValueError(f"op: expected one of {OPS}, got {op}")
    if W:
        out[:, W - 1] &= np.uint64(valid_bits_word(n))
    return out
