"""tests/selterms_ref.py, the numpy restatement of KSCHED_SEL_TERMS (include/ksched.h, extension E10), pinned to answers worked out by hand,
without a GPU: two terms that each pass a different node; an all-zero term; a NEVER-padded term; one term IS tests/seltag_ref.py's row;
n = 63, 64, 65 under NE and ABSENT terms (padding bits zero); two terms over two keys where the AND of ORs and the OR of ANDs differ; both
layouts of the entries; no selectors and no keys."""
import numpy as np
import pytest

from tests import selterms_ref, seltag_ref

EQ, NE, EX, AB, GT, LT = seltag_ref.TAGS
E = seltag_ref.entry
NEVER = seltag_ref.NEVER
# four nodes, two keys: zone = (1, 2, 1, absent), disk = (5, 5, 6, 6)
LAB = np.array([[1, 2, 1, 0], [5, 5, 6, 6]], dtype=np.uint32)


def rows(sel):
    """the packed rows of [T][2][p] entries over LAB, as Python ints (one word each)"""
    return [int(r[0]) for r in selterms_ref.selterms_mask(LAB, np.array(sel, dtype=np.uint32))]


def test_the_constants():
    assert (selterms_ref.SHIFT, selterms_ref.MASK, selterms_ref.MAX_TERMS) == (20, 0x00F00000, 15)
    assert selterms_ref.field(1) == 0x100000 and selterms_ref.field(15) == selterms_ref.MASK
    assert not selterms_ref.MASK & (0x1FF | 0xE00 | 0x2000 | 0x1C000 | 0x40000 | 0x1000 | 0x20000 | 0x80000)


def test_two_terms_that_each_pass_a_different_node():
    # pod 0: (zone = 2) | (zone absent) -> nodes 1 and 3;  pod 1: (disk = 6 & zone = 1) | (zone = 2) -> nodes 2 and 1
    sel = [[[E(EQ, 2), E(EQ, 1)], [0, E(EQ, 6)]],
           [[E(AB, 0), E(EQ, 2)], [0, 0]]]
    assert rows(sel) == [0b1010, 0b0110]
    one = selterms_ref.term_masks(LAB, np.array(sel, dtype=np.uint32))
    assert [int(r[0]) for r in one[0]] == [0b0010, 0b0100] and [int(r[0]) for r in one[1]] == [0b1000, 0b0010]


def test_the_mask_and_the_single_terms_in_one_pass_are_the_two_functions():
    sel = np.array([[[E(EQ, 2), E(EQ, 1)], [0, E(EQ, 6)]],
                    [[E(AB, 0), E(EQ, 2)], [0, 0]],
                    [[0, 0], [NEVER, E(LT, 6)]]], dtype=np.uint32)  # pod 0: padding; pod 1: disk < 6 -> nodes 0 and 1
    both, one = selterms_ref.selterms_and_term_masks(LAB, sel)
    assert [int(r[0]) for r in both] == rows(sel) == [0b1010, 0b0111]
    assert [[int(r[0]) for r in m] for m in one] == [[int(r[0]) for r in m] for m in selterms_ref.term_masks(LAB, sel)] == [[0b0010, 0b0100], [0b1000, 0b0010], [0, 0b0011]]
    both2, one2 = selterms_ref.selterms_and_term_masks(LAB, sel.reshape(6, 2))  # the flat layout
    assert np.array_equal(both2, both) and all(np.array_equal(a, b) for a, b in zip(one2, one))


def test_an_all_zero_term_passes_everywhere_wherever_it_stands():
    assert rows([[[0], [0]], [[E(EQ, 2)], [0]], [[NEVER], [0]]]) == [0b1111]
    assert rows([[[E(EQ, 2)], [0]], [[0], [NEVER]], [[0], [0]]]) == [0b1111]
    assert rows([[[0], [0]]]) == [0b1111], "a pod without affinity is all zeros"


def test_a_never_padded_term_adds_nothing():
    assert rows([[[E(EQ, 2)], [0]], [[0], [NEVER]]]) == [0b0010]
    assert rows([[[E(EQ, 2)], [0]], [[E(6, 2)], [0]], [[0], [E(7, 5)]]]) == [0b0010], "tags 6 and 7, whatever the id field holds"
    assert rows([[[NEVER], [0]], [[0], [NEVER]]]) == [0], "every term NEVER: no node (an empty list of terms)"
    # NEVER in one key kills the term whatever its other keys say
    assert rows([[[NEVER], [E(EQ, 5)]], [[E(EQ, 1)], [E(EQ, 6)]]]) == [0b0100]


def test_the_or_of_ands_is_not_the_and_of_ors():
    # (zone = 1 & disk = 5) | (zone = 2 & disk = 6): node 0 alone.  Key by key, (zone in {1, 2}) & (disk in {5, 6}) says nodes 0, 1, 2.
    sel = np.array([[[E(EQ, 1)], [E(EQ, 5)]], [[E(EQ, 2)], [E(EQ, 6)]]], dtype=np.uint32)
    assert rows(sel) == [0b0001]
    assert int(selterms_ref.and_of_ors_mask(LAB, sel, keys_per_pass=1)[0, 0]) == 0b0111
    assert int(selterms_ref.and_of_ors_mask(LAB, sel, keys_per_pass=2)[0, 0]) == 0b0001, "both keys in one pass: nothing to get wrong"


def test_one_term_is_the_tagged_row():
    rng = np.random.default_rng(0xE10)
    lab = rng.integers(0, 5, size=(3, 70)).astype(np.uint32)
    sel = np.where(rng.random((3, 9)) < 0.5, E(rng.integers(0, 8, size=(3, 9)), rng.integers(0, 5, size=(3, 9))), 0).astype(np.uint32)
    want = seltag_ref.seltag_mask(lab, sel)
    assert np.array_equal(selterms_ref.selterms_mask(lab, sel[None]), want)
    assert np.array_equal(selterms_ref.selterms_mask(lab, sel), want), "[1 * k][p] is the same array"
    # and T terms are the OR of the T tagged rows, in either layout
    sel3 = np.stack([sel, np.roll(sel, 1, axis=1), np.roll(sel, 2, axis=0)])
    want3 = want | seltag_ref.seltag_mask(lab, sel3[1]) | seltag_ref.seltag_mask(lab, sel3[2])
    assert np.array_equal(selterms_ref.selterms_mask(lab, sel3), want3)
    assert np.array_equal(selterms_ref.selterms_mask(lab, sel3.reshape(9, 9)), want3)
    assert not np.array_equal(want3, want)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_padding_bits_stay_zero_under_ne_and_absent_terms(n):
    lab = np.zeros((1, n), dtype=np.uint32)
    lab[0, 0] = 3  # node 0 carries the key with id 3, no other node carries it
    sel = np.array([[[E(NE, 3), E(AB, 0), E(EQ, 3)]], [[E(AB, 0), E(NE, 4), E(NE, 3)]]], dtype=np.uint32)  # [2][1][3]
    got = selterms_ref.selterms_mask(lab, sel)
    W = (n + 63) // 64
    assert got.shape == (3, W)
    everyone = [(1 << min(64, n - 64 * w)) - 1 for w in range(W)]
    but_node_0 = [everyone[0] & ~1] + everyone[1:]
    assert [int(x) for x in got[0]] == but_node_0, "NE 3 | ABSENT: every node but node 0, and no bit at or beyond n"
    assert [int(x) for x in got[1]] == everyone, "ABSENT | NE 4: every node"
    assert [int(x) for x in got[2]] == everyone, "EQ 3 | NE 3: every node"


def test_no_selectors_and_no_keys_pass_every_node():
    assert selterms_ref.selterms_mask(LAB, None, p=2).tolist() == [[0b1111], [0b1111]]
    none = np.zeros((0, 4), dtype=np.uint32)
    assert selterms_ref.selterms_mask(none, np.zeros((3, 0, 2), dtype=np.uint32)).tolist() == [[0b1111], [0b1111]]
