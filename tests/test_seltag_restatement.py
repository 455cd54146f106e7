"""tests/seltag_ref.py pinned to answers worked by hand from include/ksched.h's table (extension E9), no GPU and no library: every tag
against the node ids 0, 1, 2, id - 1, id, id + 1, 0x1FFFFFFF, 0x20000000, 0x20000001, 0x7FFFFFFF, 0x80000000 and 0xFFFFFFFE (ids at or
above 2^29 are compared WHOLE: masking them to 29 bits, or a signed compare, turns cells round); tags 6 and 7 with any id field; NEVER;
e == 0; LT with id 0, 1 and 2; GT with id 0x1FFFFFFF; two constrained keys; and n = 63, 64, 65, where the padding bits of the last word
must be zero under NE and ABSENT too -- the two rules an all-zero padding lane would pass."""
import numpy as np
import pytest

from tests import seltag_ref as R

EQ, NE, EX, AB, GT, LT = R.TAGS
NEVER = 0xFFFFFFFF
ID = 1000  # the entry's id in the hand table: id - 1, id and id + 1 are distinct from every other column
NODE_IDS = [0, 1, 2, ID - 1, ID, ID + 1, 0x1FFFFFFF, 0x20000000, 0x20000001, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE]
# per tag the expected bit for each node id above, in that order, with the entry's id = ID; written out by hand from the table
TABLE = {
    #     0  1  2  999 1000 1001 1FFFFFFF 20000000 20000001 7FFFFFFF 80000000 FFFFFFFE
    EQ: [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0],
    NE: [1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1],
    EX: [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    AB: [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    GT: [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1],
    LT: [0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0],
    6: [0] * 12,
    7: [0] * 12,
}


def one(e, v):
    """the bit of one (entry, node id) pair"""
    m = R.seltag_mask(np.array([[v]], dtype=np.uint32), np.array([[e]], dtype=np.uint32))
    assert m.shape == (1, 1) and int(m[0, 0]) in (0, 1)
    assert bool(R.pair(e, v)) == bool(m[0, 0])
    return int(m[0, 0])


def test_the_constants():
    assert (R.TAGGED, R.SHIFT, R.ID_MASK, R.NEVER) == (0x40000, 29, 0x1FFFFFFF, 0xFFFFFFFF)
    assert R.TAGS == (0, 1, 2, 3, 4, 5) and (R.EQ, R.NE, R.EXISTS, R.ABSENT, R.GT, R.LT) == R.TAGS
    assert int(R.entry(GT, 16)) == 0x80000010 and int(R.entry(EQ, 5)) == 5 and int(R.entry(7, R.ID_MASK)) == NEVER
    assert NEVER >> 29 == 7 and int(R.entry(LT, 3)) == 0xA0000003


@pytest.mark.parametrize("tag", list(TABLE), ids=[R.NAMES.get(t, "tag%d" % t) for t in TABLE])
def test_every_tag_against_the_hand_table(tag):
    e = int(R.entry(tag, ID))
    assert e >> 29 == tag and e & 0x1FFFFFFF == ID
    assert [one(e, v) for v in NODE_IDS] == TABLE[tag]


def test_an_unconstrained_entry_passes_everywhere_and_never_nowhere():
    for v in NODE_IDS:
        assert one(0, v) == 1, "e == 0: the key is not constrained, also on a node without it"
        assert one(NEVER, v) == 0, "NEVER is tag 7"


@pytest.mark.parametrize("tag", [6, 7])
def test_tags_6_and_7_pass_nowhere_whatever_the_id_field_holds(tag):
    for ident in (0, 1, 2, ID, 0x1FFFFFFE, 0x1FFFFFFF):
        for v in NODE_IDS + [ident]:
            assert one(int(R.entry(tag, ident)), v) == 0, (tag, hex(ident), hex(v))


def test_exists_and_absent_do_not_look_at_the_id_field():
    for ident in (0, 1, 2, ID, 0x1FFFFFFF):
        for v in NODE_IDS:
            assert one(int(R.entry(EX, ident)), v) == int(v != 0)
            assert one(int(R.entry(AB, ident)), v) == int(v == 0)


def test_lt_with_id_0_1_and_2():
    for v in NODE_IDS:
        assert one(int(R.entry(LT, 0)), v) == 0, "no id is below 0"
        assert one(int(R.entry(LT, 1)), v) == 0, "below 1 lies only 0, the absent node"
        assert one(int(R.entry(LT, 2)), v) == int(v == 1)


def test_gt_with_the_largest_id_and_with_id_0():
    top = int(R.entry(GT, 0x1FFFFFFF))
    assert [one(top, v) for v in NODE_IDS] == [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1], "ids at or above 2^29 pass GT for every bound"
    assert [one(int(R.entry(GT, 0)), v) for v in NODE_IDS] == [0] + [1] * 11, "GT 0: every node that carries the key"


def test_ne_with_id_0_and_eq_against_ids_beyond_the_field():
    assert [one(int(R.entry(NE, 0)), v) for v in NODE_IDS] == [0] + [1] * 11, "v != 0, by the table"
    # an entry cannot name an id at or above 2^29: 0x20000001 & ID_MASK == 1, and the node's id is compared whole
    assert one(int(R.entry(EQ, 1)), 0x20000001) == 0 and one(int(R.entry(NE, 1)), 0x20000001) == 1
    assert one(int(R.entry(EQ, 0x1FFFFFFF)), 0x1FFFFFFF) == 1 and one(int(R.entry(EQ, 0x1FFFFFFF)), 0xFFFFFFFF) == 0
    assert one(int(R.entry(LT, 2)), 0x20000001) == 0 and one(int(R.entry(LT, 0x1FFFFFFF)), 0x80000000) == 0


def test_two_constrained_keys_are_anded():
    # nodes 0 .. 3: (key 0, key 1) = (5, 0), (5, 9), (0, 9), (3, 12)
    lab = np.array([[5, 5, 0, 3], [0, 9, 9, 12]], dtype=np.uint32)
    # pod 0: key 0 NE 5 and key 1 GT 10; pod 1: key 0 EXISTS; pod 2: key 1 ABSENT; pod 3 neither; pod 4: key 0 NEVER, key 1 EQ 9;
    # pod 5: key 0 EQ 5 and key 1 LT 10
    sel = np.array([[R.entry(NE, 5), R.entry(EX, 0), 0, 0, NEVER, 5], [R.entry(GT, 10), 0, R.entry(AB, 77), 0, 9, R.entry(LT, 10)]], dtype=np.uint32)
    assert R.seltag_mask(lab, sel)[:, 0].tolist() == [0b1000, 0b1011, 0b0001, 0b1111, 0, 0b0010]


def test_no_selectors_and_no_keys_pass_every_node():
    lab = np.array([[0, 1, 2]], dtype=np.uint32)
    assert R.seltag_mask(lab, None, p=2).tolist() == [[0b111], [0b111]]
    assert R.seltag_mask(np.zeros((0, 3), np.uint32), np.zeros((0, 2), np.uint32)).tolist() == [[0b111], [0b111]]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_padding_bits_are_zero_under_ne_and_absent_too(n):
    lab = np.full((1, n), 7, dtype=np.uint32)
    lab[0, 0] = 0  # node 0 does not carry the key
    # pod 0: NE 9 (every node); pod 1: NE 7 (node 0 alone); pod 2: ABSENT (node 0 alone); pod 3: unconstrained; pod 4: EXISTS (all but node 0)
    sel = np.array([[R.entry(NE, 9), R.entry(NE, 7), R.entry(AB, 0), 0, R.entry(EX, 0)]], dtype=np.uint32)
    W = (n + 63) // 64
    full = [(1 << min(64, n - 64 * w)) - 1 for w in range(W)]
    only0 = [1] + [0] * (W - 1)
    but0 = [full[0] & ~1] + full[1:]
    assert R.seltag_mask(lab, sel).tolist() == [full, only0, only0, full, but0]
    assert n != 65 or full == [0xFFFFFFFFFFFFFFFF, 1]
    assert n != 63 or full == [0x7FFFFFFFFFFFFFFF]
