"""tests/uniform_ref.py, the numpy restatement of KSCHED_PICK_UNIFORM that every GPU test of the uniform pick compares against, pinned
by hand-written cases and by a bit-by-bit Python loop.  No GPU, no library."""
import numpy as np
import pytest

from tests.uniform_ref import uniform_pick


def row(words, W=None):
    a = np.array([words], dtype=np.uint64)
    if W is not None and a.shape[1] < W:
        a = np.concatenate([a, np.zeros((1, W - a.shape[1]), np.uint64)], axis=1)
    return a


def slow_pick(mask_row, u, n):
    """bit by bit, in Python integers"""
    nodes = [i for i in range(n) if (int(mask_row[i // 64]) >> (i % 64)) & 1]
    if not nodes:
        return -1
    return nodes[(int(u) * len(nodes)) >> 32]


@pytest.mark.parametrize("u, node", [(0, 0), (0x3FFFFFFF, 0), (0x40000000, 2), (0x7FFFFFFF, 2), (0x80000000, 3), (0xC0000000, 5),
                                     (0xFFFFFFFF, 5)])
def test_four_of_six(u, node):
    assert uniform_pick(row([0b101101]), np.array([u], np.uint32), 6)[0] == node


def test_bits_63_and_64_across_a_word_edge():
    m = row([1 << 63, 1])
    assert uniform_pick(m, np.array([0], np.uint32), 128)[0] == 63
    assert uniform_pick(m, np.array([0x7FFFFFFF], np.uint32), 128)[0] == 63
    assert uniform_pick(m, np.array([0x80000000], np.uint32), 128)[0] == 64
    assert uniform_pick(m, np.array([0xFFFFFFFF], np.uint32), 128)[0] == 64
    assert uniform_pick(m, np.array([0xFFFFFFFF], np.uint32), 64)[0] == 63  # n = 64: node 64 does not exist


def test_padding_bits_and_padding_words_are_ignored():
    ones = 0xFFFFFFFFFFFFFFFF
    # n = 70: bits 6 .. 63 of word 1 and the whole of words 2, 3 are padding
    m = row([1 << 5, ones & ~0x3F, ones, ones])
    for u in (0, 0x80000000, 0xFFFFFFFF):
        assert uniform_pick(m, np.array([u], np.uint32), 70)[0] == 5
    m = row([0, ones & ~0x3F, ones, ones])
    assert uniform_pick(m, np.array([123456789], np.uint32), 70)[0] == -1
    m = row([0, ones, ones])
    assert uniform_pick(m, np.array([0xFFFFFFFF], np.uint32), 70)[0] == 69
    assert uniform_pick(m, np.array([0], np.uint32), 70)[0] == 64


def test_no_feasible_node_and_degenerate_shapes():
    assert uniform_pick(np.zeros((3, 2), np.uint64), np.array([0, 7, 0xFFFFFFFF], np.uint32), 100).tolist() == [-1, -1, -1]
    assert uniform_pick(np.zeros((2, 0), np.uint64), np.array([1, 2], np.uint32), 0).tolist() == [-1, -1]
    assert uniform_pick(np.zeros((0, 2), np.uint64), np.zeros((0,), np.uint32), 100).shape == (0,)


def test_equals_the_bit_by_bit_loop_on_random_rows():
    rng = np.random.default_rng(0x0E3)
    for _ in range(200):
        n = int(rng.integers(1, 400))
        W = (n + 63) // 64
        pitch = W + int(rng.integers(0, 3))
        density = rng.choice([0.0, 0.01, 0.2, 0.9, 1.0])
        bits = rng.random((1, pitch * 64)) < density  # (padding bits and words are set at the same density)
        m = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
        u = int(rng.choice([0, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))]))
        assert uniform_pick(m, np.array([u], np.uint32), n)[0] == slow_pick(m[0], u, n), (n, u)


def test_even_over_37_feasible_nodes():
    rng = np.random.default_rng(37)
    n = 300
    nodes = np.sort(rng.choice(n, size=37, replace=False))
    bits = np.zeros((1, 320), bool)
    bits[0, nodes] = True
    m = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
    draws = (np.arange(4096, dtype=np.uint64) << np.uint64(20)).astype(np.uint32)  # u_i = i * 2^32 / 4096
    got = uniform_pick(np.repeat(m, 4096, axis=0), draws, n)
    chosen, counts = np.unique(got, return_counts=True)
    assert chosen.tolist() == nodes.tolist()
    assert set(counts.tolist()) <= {110, 111} and counts.sum() == 4096
