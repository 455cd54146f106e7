"""tests/combine_ref.py pinned with hand-written known answers, without a GPU: the three ops of KSCHED_COMBINE_* at n = 1, 63, 64, 65 -- the
valid-bits word on either side of a word boundary --, with garbage in the old mask's bits at or beyond n, which must come out zero."""
import numpy as np
import pytest

from tests import combine_ref as R

ALL = 0xFFFFFFFFFFFFFFFF


def u64(*rows):
    return np.array(rows, dtype=np.uint64)


def test_the_ops_carry_the_flag_values():
    assert (R.AND, R.OR, R.ANDNOT) == (0x200, 0x400, 0x800) and R.OPS == (R.AND, R.OR, R.ANDNOT)


@pytest.mark.parametrize("n,want", [(1, 0x1), (2, 0x3), (63, 0x7FFFFFFFFFFFFFFF), (64, ALL), (65, 0x1), (127, 0x7FFFFFFFFFFFFFFF), (128, ALL), (129, 0x1)])
def test_valid_bits_word(n, want):
    assert R.valid_bits_word(n) == want


# (n, old row, new row) -> (and, or, andnot); the old rows carry set bits at and beyond n
KNOWN = [
    # n = 1: one node, bit 0; old = all ones (63 garbage bits)
    (1, [ALL], [0x1], ([0x1], [0x1], [0x0])),
    (1, [ALL], [0x0], ([0x0], [0x1], [0x1])),
    (1, [0xFFFFFFFFFFFFFFFE], [0x1], ([0x0], [0x1], [0x0])),  # old has ONLY garbage: node 0 is not in it
    # n = 63: bit 63 is garbage
    (63, [0x8000000000000005], [0x0000000000000006], ([0x4], [0x7], [0x1])),
    (63, [ALL], [0x7FFFFFFFFFFFFFFF], ([0x7FFFFFFFFFFFFFFF], [0x7FFFFFFFFFFFFFFF], [0x0])),
    # n = 64: the whole word is valid, nothing to clear
    (64, [0x8000000000000005], [0x8000000000000006], ([0x8000000000000004], [0x8000000000000007], [0x1])),
    (64, [ALL], [0x0], ([0x0], [ALL], [ALL])),
    # n = 65: two words, the second holds one valid bit; the first is never masked
    (65, [0xF0F0F0F0F0F0F0F0, ALL], [0xFF00FF00FF00FF00, 0x1], ([0xF000F000F000F000, 0x1], [0xFFF0FFF0FFF0FFF0, 0x1], [0x00F000F000F000F0, 0x0])),
    (65, [0x8000000000000000, 0xFFFFFFFFFFFFFFFE], [0x8000000000000000, 0x1], ([0x8000000000000000, 0x0], [0x8000000000000000, 0x1], [0x0, 0x0])),
]


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_known_answers(case):
    n, old, new, want = KNOWN[case]
    for op, w in zip(R.OPS, want):
        got = R.combine(u64(old), u64(new), op, n)
        assert got.dtype == np.uint64 and got.tolist() == [w], (n, R.NAMES[op], [hex(x) for x in got[0]])


def test_rows_are_independent_and_the_inputs_are_left_alone():
    old, new = u64([ALL, ALL], [0x0, ALL], [0x5, 0x2]), u64([0x3, 0x1], [0x3, 0x1], [0x6, 0x3])
    old0, new0 = old.copy(), new.copy()
    assert R.combine(old, new, R.AND, 65).tolist() == [[0x3, 0x1], [0x0, 0x1], [0x4, 0x0]]
    assert R.combine(old, new, R.OR, 65).tolist() == [[ALL, 0x1], [0x3, 0x1], [0x7, 0x1]]
    assert R.combine(old, new, R.ANDNOT, 65).tolist() == [[0xFFFFFFFFFFFFFFFC, 0x0], [0x0, 0x0], [0x1, 0x0]]
    assert (old == old0).all() and (new == new0).all()


def test_no_pods_and_a_wrong_shape():
    assert R.combine(np.zeros((0, 2), np.uint64), np.zeros((0, 2), np.uint64), R.OR, 65).shape == (0, 2)
    with pytest.raises(AssertionError):
        R.combine(u64([0, 0]), u64([0, 0]), R.AND, 64)  # two words for 64 nodes
    with pytest.raises(ValueError):
        R.combine(u64([0]), u64([0]), 0x1000, 64)
