"""tests/soft_ref.py pinned with hand-written known answers, without a GPU: KSCHED_COMBINE_SOFT over AND and AND-NOT at n = 1, 63, 64, 65 --
an empty old row, an old row holding only garbage bits at and beyond n, a result whose only bit is node n - 1, a result whose only bit would
be node n, and the plain narrowing and dropped rows around them."""
import numpy as np
import pytest

from tests import combine_ref
from tests import soft_ref as S

ALL = 0xFFFFFFFFFFFFFFFF
N, D, E = S.NARROWED, S.DROPPED, S.EMPTY


def u64(*rows):
    return np.array(rows, dtype=np.uint64)


def test_the_ops_and_the_bit():
    assert S.SOFT == 0x2000 and S.OPS == (0x200, 0x800) and not (S.SOFT & 0xE00)


# (n, op, old row, new row) -> (row afterwards, what happened to it); the old rows carry set bits at and beyond n
KNOWN = [
    # n = 1: one node
    (1, S.AND, [ALL], [0x1], [0x1], N),
    (1, S.AND, [ALL], [0x0], [0x1], D),                     # would empty: node 0 stays, the 63 garbage bits go
    (1, S.ANDNOT, [ALL], [0x1], [0x1], D),
    (1, S.ANDNOT, [ALL], [0x0], [0x1], N),
    (1, S.AND, [0xFFFFFFFFFFFFFFFE], [0x1], [0x0], E),      # only garbage: counts as empty and comes out zero
    (1, S.ANDNOT, [0xFFFFFFFFFFFFFFFE], [0x0], [0x0], E),
    (1, S.AND, [0x0], [0x1], [0x0], E),                     # an empty row stays empty
    # n = 63: bit 63 is garbage
    (63, S.AND, [ALL], [0x4000000000000000], [0x4000000000000000], N),   # the only bit left is node n - 1
    (63, S.AND, [ALL], [0x8000000000000000], [0x7FFFFFFFFFFFFFFF], D),   # the only bit left would be node n
    (63, S.ANDNOT, [0xC000000000000000], [0x0], [0x4000000000000000], N),
    (63, S.ANDNOT, [0xC000000000000000], [0x4000000000000000], [0x4000000000000000], D),  # r would hold only the garbage bit
    (63, S.AND, [0x8000000000000000], [ALL], [0x0], E),
    # n = 64: the whole word is valid
    (64, S.AND, [0x8000000000000005], [0x8000000000000000], [0x8000000000000000], N),
    (64, S.AND, [0x8000000000000005], [0x0000000000000002], [0x8000000000000005], D),
    (64, S.ANDNOT, [ALL], [ALL], [ALL], D),
    (64, S.ANDNOT, [ALL], [0x7FFFFFFFFFFFFFFF], [0x8000000000000000], N),
    (64, S.AND, [0x0], [ALL], [0x0], E),
    # n = 65: two words, the second holds one valid bit
    (65, S.AND, [0x6, ALL], [0x4, 0x0], [0x4, 0x0], N),
    (65, S.AND, [0x6, ALL], [0x9, 0x0], [0x6, 0x1], D),                   # dropped: old', with node 64 kept and the garbage cleared
    (65, S.AND, [0x6, ALL], [0x0, 0x1], [0x0, 0x1], N),                   # the only bit left is node n - 1 = 64
    (65, S.AND, [0x6, 0xFFFFFFFFFFFFFFFE], [0x0, 0x2], [0x6, 0x0], D),    # the only bit left would be node n = 65
    (65, S.ANDNOT, [0x6, ALL], [0x6, 0x0], [0x0, 0x1], N),
    (65, S.ANDNOT, [0x6, 0xFFFFFFFFFFFFFFFE], [0x6, 0x0], [0x6, 0x0], D),
    (65, S.AND, [0x0, 0xFFFFFFFFFFFFFFFE], [ALL, 0x1], [0x0, 0x0], E),    # only garbage, in the second word
    (65, S.ANDNOT, [0x0, 0x0], [0x0, 0x0], [0x0, 0x0], E),
]


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_known_answers(case):
    n, op, old, new, want, what = KNOWN[case]
    for flag in (op, op | S.SOFT):
        got = S.soft_combine(u64(old), u64(new), flag, n)
        assert got.dtype == np.uint64 and got.tolist() == [want], (n, S.NAMES[op], [hex(x) for x in got[0]])
        assert S.decisions(u64(old), u64(new), flag, n).tolist() == [what]


def test_the_consequences_on_random_rows():
    """an empty row stays empty, a non-empty row never becomes empty, bits at or beyond n come out zero, and a narrowed row is the plain
    combine's"""
    rng = np.random.default_rng(0xE7)
    for n in (1, 63, 64, 65, 129):
        W = (n + 63) // 64
        old = rng.integers(0, 1 << 64, size=(400, W), dtype=np.uint64)
        new = rng.integers(0, 1 << 64, size=(400, W), dtype=np.uint64)
        old[::4] = 0
        new[1::4] = 0
        new[2::4] = ALL
        old[3::8, -1] |= np.uint64(~combine_ref.valid_bits_word(n) & ALL)
        for op in S.OPS:
            got, what = S.soft_combine(old, new, op, n), S.decisions(old, new, op, n)
            before = S.old_prime(old, n)
            assert (got.any(axis=1) == before.any(axis=1)).all()
            assert not (got[:, -1] & np.uint64(~combine_ref.valid_bits_word(n) & ALL)).any()
            plain = combine_ref.combine(old, new, op, n)
            assert np.array_equal(got[what == N], plain[what == N]) and np.array_equal(got[what != N], before[what != N])
            assert not plain[what != N].any() and not got[what == E].any() and got[what == D].any(axis=1).all()
            assert {N, D, E} <= set(what.tolist())


def test_rows_are_independent_and_the_inputs_are_left_alone():
    old, new = u64([0x6, ALL], [0x6, ALL], [0x0, 0x0]), u64([0x4, 0x0], [0x9, 0x0], [ALL, ALL])
    old0, new0 = old.copy(), new.copy()
    assert S.soft_combine(old, new, S.AND, 65).tolist() == [[0x4, 0x0], [0x6, 0x1], [0x0, 0x0]]
    assert S.decisions(old, new, S.AND, 65).tolist() == [N, D, E]
    assert (old == old0).all() and (new == new0).all()


def test_no_pods_and_the_ops_it_refuses():
    assert S.soft_combine(np.zeros((0, 2), np.uint64), np.zeros((0, 2), np.uint64), S.AND, 65).shape == (0, 2)
    for op in (0x400, 0x400 | S.SOFT, S.SOFT, 0x1000):
        with pytest.raises(ValueError):
            S.soft_combine(u64([0]), u64([0]), op, 64)
