"""tests/selop_ref.py pinned to answers worked by hand from include/ksched.h's table (extension E8), no GPU and no library: every cell of the
table; the ids 1, 2, 0x7FFFFFFF, 0x80000000 and 0xFFFFFFFE on both sides of a compare (a signed compare would turn the middle pairs
round); an absent node under LT with a large bound; NEVER under each operator; two constrained keys; and n = 63, 64, 65, where the padding
bits of the last word must be zero."""
import numpy as np
import pytest

from tests import selop_ref as R

E, G, L = R.EXISTS, R.GT, R.LT
NEVER = 0xFFFFFFFF
IDS = [1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE]


def one(op, e, v):
    """the bit of one (entry, node id) pair"""
    m = R.selop_mask(np.array([[v]], dtype=np.uint32), np.array([[e]], dtype=np.uint32), op)
    assert m.shape == (1, 1) and int(m[0, 0]) in (0, 1)
    return int(m[0, 0])


def test_the_constants():
    assert (R.EXISTS, R.GT, R.LT, R.NEVER) == (0x4000, 0x8000, 0x10000, 0xFFFFFFFF) and R.OPS == (E, G, L)
    with pytest.raises(ValueError):
        R.pass_bits(np.zeros((1, 1), np.uint32), np.zeros((1, 1), np.uint32), 0x2)


@pytest.mark.parametrize("op", R.OPS, ids=["exists", "gt", "lt"])
def test_an_unconstrained_key_passes_and_never_never_does(op):
    for v in [0] + IDS:
        assert one(op, 0, v) == 1, "e == 0: the key is not constrained, also on a node without it"
        assert one(op, NEVER, v) == 0, "e == NEVER never passes, also on a node that carries the key"


# (op, e, v) -> bit, each worked from the table: v != 0 [&& v > e | v < e]
CELLS = [
    (E, 1, 0, 0), (E, 1, 1, 1), (E, 1, 2, 1), (E, 7, 0xFFFFFFFE, 1), (E, 0xFFFFFFFE, 1, 1), (E, 0xFFFFFFFE, 0, 0),
    (G, 1, 0, 0), (G, 1, 1, 0), (G, 1, 2, 1), (G, 2, 1, 0), (G, 2, 2, 0), (G, 2, 3, 1),
    (L, 1, 0, 0), (L, 1, 1, 0), (L, 2, 1, 1), (L, 2, 2, 0), (L, 2, 0, 0), (L, 3, 2, 1),
    # the sign bit: 0x7FFFFFFF < 0x80000000 < 0xFFFFFFFE as unsigned numbers (as signed ones the last two are negative)
    (G, 0x7FFFFFFF, 0x80000000, 1), (G, 0x80000000, 0x7FFFFFFF, 0), (G, 0x7FFFFFFF, 0xFFFFFFFE, 1), (G, 0xFFFFFFFE, 0x7FFFFFFF, 0),
    (G, 1, 0x80000000, 1), (G, 0x80000000, 1, 0), (G, 0x80000000, 0xFFFFFFFE, 1), (G, 0xFFFFFFFE, 0x80000000, 0), (G, 0xFFFFFFFE, 0xFFFFFFFE, 0),
    (L, 0x80000000, 0x7FFFFFFF, 1), (L, 0x7FFFFFFF, 0x80000000, 0), (L, 0xFFFFFFFE, 0x7FFFFFFF, 1), (L, 0x7FFFFFFF, 0xFFFFFFFE, 0),
    (L, 0x80000000, 1, 1), (L, 1, 0x80000000, 0), (L, 0xFFFFFFFE, 0x80000000, 1), (L, 0x80000000, 0xFFFFFFFE, 0), (L, 0xFFFFFFFE, 0xFFFFFFFE, 0),
    # an absent node under LT with a large bound: 0 < e as numbers, but the node does not carry the key
    (L, 0xFFFFFFFE, 0, 0), (L, 0x80000000, 0, 0), (L, 0x7FFFFFFF, 0, 0), (G, 0xFFFFFFFE, 0, 0), (G, 0x80000000, 0, 0),
]


@pytest.mark.parametrize("op,e,v,bit", CELLS)
def test_every_cell_of_the_table(op, e, v, bit):
    assert one(op, e, v) == bit


def test_the_ids_on_both_sides_of_a_compare():
    """IDS is ascending as unsigned numbers: GT passes exactly below the diagonal of (entry, id), LT exactly above it"""
    for i, e in enumerate(IDS):
        for j, v in enumerate(IDS):
            assert one(G, e, v) == int(j > i), (hex(e), hex(v))
            assert one(L, e, v) == int(j < i), (hex(e), hex(v))
            assert one(E, e, v) == 1


def test_two_constrained_keys_are_anded():
    # nodes 0 .. 3: (key 0, key 1) = (5, 0), (5, 9), (0, 9), (3, 12)
    lab = np.array([[5, 5, 0, 3], [0, 9, 9, 12]], dtype=np.uint32)
    # pods: 0 constrains both keys, 1 only key 0, 2 only key 1, 3 neither, 4 key 0 with NEVER and key 1 properly
    sel = np.array([[4, 4, 0, 0, NEVER], [10, 0, 10, 0, 10]], dtype=np.uint32)
    assert R.selop_mask(lab, sel, E)[:, 0].tolist() == [0b1010, 0b1011, 0b1110, 0b1111, 0]
    # GT: key 0 > 4 on nodes 0, 1; key 1 > 10 on node 3
    assert R.selop_mask(lab, sel, G)[:, 0].tolist() == [0b0000, 0b0011, 0b1000, 0b1111, 0]
    # LT: key 0 < 4 on node 3 (node 2 is absent); key 1 < 10 on nodes 1, 2 (node 0 is absent)
    assert R.selop_mask(lab, sel, L)[:, 0].tolist() == [0b0000, 0b1000, 0b0110, 0b1111, 0]
    # both keys together differ from each key alone
    lab2 = np.array([[5, 5, 0, 3], [11, 9, 9, 12]], dtype=np.uint32)
    both = R.selop_mask(lab2, np.array([[4], [10]], np.uint32), G)[0, 0]
    assert both == 0b0001 and both != 0b0011 and both != 0b1001


def test_no_selectors_and_no_keys_pass_every_node():
    lab = np.array([[0, 1, 2]], dtype=np.uint32)
    for op in R.OPS:
        assert R.selop_mask(lab, None, op, p=2).tolist() == [[0b111], [0b111]]
        assert R.selop_mask(np.zeros((0, 3), np.uint32), np.zeros((0, 2), np.uint32), op).tolist() == [[0b111], [0b111]]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_padding_bits_are_zero(n):
    lab = np.full((1, n), 7, dtype=np.uint32)
    lab[0, 0] = 0  # node 0 does not carry the key
    sel = np.array([[1, 9, 0]], dtype=np.uint32)  # pod 0: > 1 / < 1 / exists; pod 1: > 9 / < 9; pod 2: unconstrained
    W = (n + 63) // 64
    full = [(1 << min(64, n - 64 * w)) - 1 for w in range(W)]
    but0 = [full[0] & ~1] + full[1:]
    zero = [0] * W
    assert R.selop_mask(lab, sel, E).tolist() == [but0, but0, full]
    assert R.selop_mask(lab, sel, G).tolist() == [but0, zero, full]
    assert R.selop_mask(lab, sel, L).tolist() == [zero, but0, full]
    assert n != 65 or full == [0xFFFFFFFFFFFFFFFF, 1]
    assert n != 63 or full == [0x7FFFFFFFFFFFFFFF]
