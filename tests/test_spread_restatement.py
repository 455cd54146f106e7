"""tests/spread_ref.py, the numpy restatement of KSCHED_PICK_SPREAD that every GPU test of the spread pick compares against, pinned by
hand-written cases and by an independent per-pod loop in Python integers.  No GPU, no library."""
import numpy as np

from tests.spread_ref import best_of, spread_candidates, spread_candidates_listed, spread_pick, spread_pick_blocks
from tests.uniform_ref import uniform_pick

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def row(words):
    return np.array([words], dtype=np.uint64)


def slow_spread(mask_row, draws, n, mem, cpu):
    """one pod, bit by bit, in Python integers: every draw's candidate, then the best key"""
    nodes = [i for i in range(n) if (int(mask_row[i // 64]) >> (i % 64)) & 1]
    if not nodes:
        return -1
    cands = [nodes[(int(u) * len(nodes)) >> 32] for u in draws]
    return max(cands, key=lambda v: (int(mem[v]), int(cpu[v]), -v))


def u_for(j, c):
    """the smallest draw whose k is j among c feasible nodes"""
    return -((-j << 32) // c)


def test_one_draw_is_the_uniform_pick():
    rng = np.random.default_rng(0xE4)
    n = 300
    bits = rng.random((50, 320)) < 0.2
    bits[7] = False
    m = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
    u = rng.integers(0, 1 << 32, size=(50, 1), dtype=np.uint64).astype(np.uint32)
    mem, cpu = rng.integers(-5, 5, n), rng.integers(-5, 5, n)
    want = uniform_pick(m, u[:, 0], n)
    assert want[7] == -1 and (want >= 0).sum() >= 40
    assert np.array_equal(spread_pick(m, u, n, mem, cpu), want)


def test_hand_written_answers_over_four_of_six():
    m = row([0b101101])  # feasible: 0, 2, 3, 5 -- c = 4
    at = lambda *js: np.array([[u_for(j, 4) for j in js]], np.uint32)  # noqa: E731  draws naming set bits js
    assert spread_candidates(m, at(0, 1, 2, 3), 6).tolist() == [[0, 2, 3, 5]]
    mem = np.array([10, 99, 30, 20, 99, 30], np.int64)  # (nodes 1 and 4 are infeasible: their 99 never wins)
    cpu = np.array([1, 0, 5, 0, 0, 7], np.int64)
    assert spread_pick(m, at(0, 1, 2, 3), 6, mem, cpu)[0] == 5     # memory ties at 30: the larger cpu
    assert spread_pick(m, at(0, 2), 6, mem, cpu)[0] == 3           # 20 beats 10
    assert spread_pick(m, at(0, 0, 0), 6, mem, cpu)[0] == 0        # repeated candidates
    assert spread_pick(m, at(1, 1, 2, 1), 6, mem, cpu)[0] == 2     # repeated, and the other one loses
    # a permutation of the draws gives the same binding
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 3, 1]):
        assert spread_pick(m, at(*perm), 6, mem, cpu)[0] == 5
    # all-equal columns: the lowest candidate index, whatever the order
    flat = np.zeros(6, np.int64)
    assert spread_pick(m, at(3, 1, 2), 6, flat, flat)[0] == 2
    assert spread_pick(m, at(2, 3, 0), 6, flat, flat)[0] == 0
    # equal memory: the larger cpu, then the lower node
    assert spread_pick(m, at(3, 1), 6, flat, np.array([0, 0, 4, 0, 0, 4], np.int64))[0] == 2


def test_negative_values_and_both_ends_of_int64():
    m = row([0b1111])
    at = lambda *js: np.array([[u_for(j, 4) for j in js]], np.uint32)  # noqa: E731
    mem = np.array([I64_MIN, -1, I64_MAX, I64_MAX], np.int64)
    cpu = np.array([I64_MAX, I64_MIN, I64_MIN, I64_MIN + 1], np.int64)
    assert spread_pick(m, at(0, 1), 4, mem, cpu)[0] == 1        # -1 > int64 min: signed
    assert spread_pick(m, at(0, 1, 2), 4, mem, cpu)[0] == 2
    assert spread_pick(m, at(2, 3), 4, mem, cpu)[0] == 3        # cpu: min + 1 > min
    assert spread_pick(m, at(0, 0), 4, mem, cpu)[0] == 0
    mem2 = np.array([-7, -7, -7, -8], np.int64)
    cpu2 = np.array([I64_MIN, I64_MIN, -3, I64_MAX], np.int64)
    assert spread_pick(m, at(1, 0, 3), 4, mem2, cpu2)[0] == 0   # (-7, min) twice: the lower node; (-8, max) loses on memory
    assert spread_pick(m, at(3, 2, 1), 4, mem2, cpu2)[0] == 2


def test_no_feasible_node_and_degenerate_shapes():
    z = np.zeros(100, np.int64)
    assert spread_pick(np.zeros((3, 2), np.uint64), np.full((3, 4), 0xFFFFFFFF, np.uint32), 100, z, z).tolist() == [-1, -1, -1]
    e = np.zeros(0, np.int64)
    assert spread_pick(np.zeros((2, 0), np.uint64), np.ones((2, 3), np.uint32), 0, e, e).tolist() == [-1, -1]
    assert spread_pick(np.zeros((0, 2), np.uint64), np.zeros((0, 2), np.uint32), 100, z, z).shape == (0,)
    # padding bits and words are no candidates: n = 70, only node 5 is real
    ones = 0xFFFFFFFFFFFFFFFF
    m = row([1 << 5, ones & ~0x3F, ones])
    big = np.arange(70, dtype=np.int64)
    assert spread_pick(m, np.array([[0, 0x80000000, 0xFFFFFFFF]], np.uint32), 70, big, big)[0] == 5


def test_equals_the_per_pod_loop_on_random_rows():
    rng = np.random.default_rng(0x5E4)
    for _ in range(200):
        n = int(rng.integers(1, 400))
        W = (n + 63) // 64
        pitch = W + int(rng.integers(0, 3))
        d = int(rng.choice([1, 2, 3, 5, 8, 64]))
        density = rng.choice([0.0, 0.01, 0.2, 0.9, 1.0])
        bits = rng.random((1, pitch * 64)) < density  # (padding bits and words are set at the same density)
        m = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
        u = rng.integers(0, 1 << 32, size=(1, d), dtype=np.uint64).astype(np.uint32)
        span = int(rng.choice([1, 2, 4, 1 << 40]))  # few distinct values: ties in memory, in both, in neither
        mem = rng.integers(-span, span, n)
        cpu = rng.integers(-span, span, n)
        if rng.random() < 0.2:
            mem[rng.integers(0, n)] = rng.choice([I64_MIN, I64_MAX])
            cpu[rng.integers(0, n)] = rng.choice([I64_MIN, I64_MAX])
        assert spread_pick(m, u, n, mem, cpu)[0] == slow_spread(m[0], u[0], n, mem, cpu), (n, d)


def test_the_listed_route_to_the_candidates_equals_uniform_pick_per_column():
    rng = np.random.default_rng(0x115)
    for n in (1, 63, 64, 65, 130, 400, 8191, 8192, 8193, 16385):
        W = (n + 63) // 64
        for density in (0.0, 0.02, 0.5, 1.0):
            p, d = 7, int(rng.choice([1, 2, 5, 64]))
            bits = rng.random((p, (W + 2) * 64)) < density  # (two padding words, set at the same density)
            bits[3] = False
            m = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
            u = rng.integers(0, 1 << 32, size=(p, d), dtype=np.uint64).astype(np.uint32)
            u[0, 0], u[1, -1] = 0, 0xFFFFFFFF
            want = spread_candidates(m, u, n)
            assert np.array_equal(spread_candidates_listed(m, u, n), want), (n, density, d)
            mem, cpu = rng.integers(-3, 3, n), rng.integers(-3, 3, n)
            assert np.array_equal(best_of(want, mem, cpu), spread_pick(m, u, n, mem, cpu))
    assert spread_candidates_listed(np.zeros((2, 0), np.uint64), np.ones((2, 3), np.uint32), 0).tolist() == [[-1] * 3] * 2
    assert spread_candidates_listed(np.zeros((0, 2), np.uint64), np.zeros((0, 2), np.uint32), 100).shape == (0, 2)


def test_blocks_of_pods_equal_the_whole():
    """spread_pick_blocks (the listed route, a block of pods at a time) == spread_pick: block lengths of 1, 7 and 8 pods over 50 (a last
    block of one pod, of one row short, every block full but the last), one block for all, a block longer than the batch; an empty row
    first in its block, last in its block and in the middle; d = 1, 5 and 64; columns with ties"""
    rng = np.random.default_rng(0xB10C)
    for n in (1, 130, 250, 8200):
        W = (n + 63) // 64
        p = 50
        bits = rng.random((p, (W + 1) * 64)) < 0.3  # (one padding word, set at the same density)
        for empty in (0, 6, 7, 20, 49):
            bits[empty] = False
        m = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
        mem, cpu = rng.integers(-3, 3, n), rng.integers(-3, 3, n)
        for d in (1, 5, 64):
            u = rng.integers(0, 1 << 32, size=(p, d), dtype=np.uint64).astype(np.uint32)
            want = spread_pick(m, u, n, mem, cpu)
            assert (want[[0, 6, 7, 20, 49]] == -1).all() and (n < 130 or (want >= 0).sum() == p - 5)
            for pods_per_block in (1, 7, 8, 49, 50, 51):
                got = spread_pick_blocks(m, u, n, mem, cpu, cells=n * pods_per_block)
                assert got.dtype == np.int32 and np.array_equal(got, want), (n, d, pods_per_block)
            assert np.array_equal(spread_pick_blocks(m, u, n, mem, cpu), want), (n, d)
    z = np.zeros(100, np.int64)
    assert spread_pick_blocks(np.zeros((0, 2), np.uint64), np.zeros((0, 3), np.uint32), 100, z, z).shape == (0,)
