"""tests/pack_ref.py, the numpy restatement of KSCHED_PICK_PACK that every GPU test of the pack pick compares against, pinned by an
independent per-pod loop in Python integers, by the uniform pick at d = 1, by the spread pick's restatement on the bitwise complement of
the columns, and by hand-written answers.  No GPU, no library."""
import numpy as np

from tests.pack_ref import pack_pick, pack_pick_listed, tightest_of
from tests.spread_ref import spread_candidates, spread_pick
from tests.uniform_ref import uniform_pick

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def row(words):
    return np.array([words], dtype=np.uint64)


def slow_pack(mask_row, draws, n, mem, cpu):
    """one pod, bit by bit, in Python integers: a loop over the draws, a loop over the nodes for each"""
    c = sum((int(mask_row[i // 64]) >> (i % 64)) & 1 for i in range(n))
    if c == 0:
        return -1
    best = None
    for u in draws:
        k, v = (int(u) * c) >> 32, -1
        for i in range(n):
            if (int(mask_row[i // 64]) >> (i % 64)) & 1:
                if k == 0:
                    v = i
                    break
                k -= 1
        key = (int(mem[v]), int(cpu[v]), v)
        if best is None or key < best:
            best = key
    return best[2]


def u_for(j, c):
    """the smallest draw whose k is j among c feasible nodes"""
    return -((-j << 32) // c)


def random_case(rng, n_hi=300):
    n = int(rng.integers(1, n_hi))
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
    if rng.random() < 0.3:
        mem[rng.integers(0, n)] = rng.choice([I64_MIN, I64_MAX])
        cpu[rng.integers(0, n)] = rng.choice([I64_MIN, I64_MAX])
    return m, u, n, mem, cpu


def test_equals_the_plain_double_loop_on_small_random_cases():
    rng = np.random.default_rng(0xE5)
    bound = 0
    for _ in range(200):
        m, u, n, mem, cpu = random_case(rng)
        want = slow_pack(m[0], u[0], n, mem, cpu)
        bound += want >= 0
        assert pack_pick(m, u, n, mem, cpu)[0] == want, (n, u.shape)
        assert pack_pick_listed(m, u, n, mem, cpu)[0] == want, (n, u.shape)
    assert bound >= 100


def test_one_draw_is_the_uniform_pick():
    rng = np.random.default_rng(0xE51)
    n = 300
    bits = rng.random((50, 320)) < 0.2
    bits[7] = False
    m = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
    u = rng.integers(0, 1 << 32, size=(50, 1), dtype=np.uint64).astype(np.uint32)
    mem, cpu = rng.integers(-5, 5, n), rng.integers(-5, 5, n)
    want = uniform_pick(m, u[:, 0], n)
    assert want[7] == -1 and (want >= 0).sum() >= 40
    assert np.array_equal(pack_pick(m, u, n, mem, cpu), want)


def test_pack_is_spread_on_the_complemented_columns():
    """bitwise NOT reverses the order of int64 exactly (~x = -x - 1 without overflow, INT64_MIN <-> INT64_MAX), and both rules break ties
    to the lowest node: pack_pick(m, q) == spread_pick(~m, ~q)"""
    rng = np.random.default_rng(0xE52)
    differs = 0
    for _ in range(200):
        m, u, n, mem, cpu = random_case(rng)
        got = pack_pick(m, u, n, mem, cpu)
        assert np.array_equal(got, spread_pick(m, u, n, ~mem, ~cpu))
        differs += int(got[0] != spread_pick(m, u, n, mem, cpu)[0])
    assert differs >= 30  # (the two picks are not the same function on these inputs)
    ends = np.array([I64_MIN, I64_MAX, 0, -1], np.int64)
    assert (~ends).tolist() == [I64_MAX, I64_MIN, -1, 0]


def test_permuting_a_pods_draws_changes_nothing():
    rng = np.random.default_rng(0xE53)
    for _ in range(60):
        m, u, n, mem, cpu = random_case(rng)
        want = pack_pick(m, u, n, mem, cpu)
        for _ in range(3):
            assert np.array_equal(pack_pick(m, u[:, rng.permutation(u.shape[1])], n, mem, cpu), want)


def test_hand_written_answers_over_four_of_six():
    m = row([0b101101])  # feasible: 0, 2, 3, 5 -- c = 4
    at = lambda *js: np.array([[u_for(j, 4) for j in js]], np.uint32)  # noqa: E731  draws naming set bits js
    assert spread_candidates(m, at(0, 1, 2, 3), 6).tolist() == [[0, 2, 3, 5]]
    mem = np.array([30, 1, 10, 20, 1, 10], np.int64)  # (nodes 1 and 4 are infeasible: their 1 never wins)
    cpu = np.array([1, 0, 5, 0, 0, 3], np.int64)
    assert pack_pick(m, at(0, 1, 2, 3), 6, mem, cpu)[0] == 5     # memory ties at 10: the smaller cpu
    assert pack_pick(m, at(0, 2), 6, mem, cpu)[0] == 3           # 20 beats 30
    assert pack_pick(m, at(0, 0, 0), 6, mem, cpu)[0] == 0        # repeated candidates
    assert pack_pick(m, at(2, 2, 1, 2), 6, mem, cpu)[0] == 2     # repeated, and the other one loses
    flat = np.zeros(6, np.int64)
    assert pack_pick(m, at(3, 1, 2), 6, flat, flat)[0] == 2      # all equal: the lowest candidate, whatever the order
    assert pack_pick(m, at(2, 3, 0), 6, flat, flat)[0] == 0
    assert pack_pick(m, at(3, 1), 6, flat, np.array([9, 0, 4, 9, 0, 4], np.int64))[0] == 2  # equal memory and cpu: the lower node


def test_negative_values_and_both_ends_of_int64():
    m = row([0b1111])
    at = lambda *js: np.array([[u_for(j, 4) for j in js]], np.uint32)  # noqa: E731
    mem = np.array([I64_MAX, 0, I64_MIN, I64_MIN], np.int64)
    cpu = np.array([I64_MIN, I64_MAX, I64_MAX, I64_MAX - 1], np.int64)
    assert pack_pick(m, at(0, 1), 4, mem, cpu)[0] == 1        # 0 < int64 max
    assert pack_pick(m, at(0, 1, 2), 4, mem, cpu)[0] == 2     # int64 min < 0: signed
    assert pack_pick(m, at(2, 3), 4, mem, cpu)[0] == 3        # cpu: max - 1 < max
    mem2 = np.array([-7, -7, -7, -6], np.int64)
    cpu2 = np.array([I64_MAX, I64_MAX, 3, I64_MIN], np.int64)
    assert pack_pick(m, at(1, 0, 3), 4, mem2, cpu2)[0] == 0   # (-7, max) twice: the lower node; (-6, min) loses on memory
    assert pack_pick(m, at(3, 2, 1), 4, mem2, cpu2)[0] == 2


def test_no_feasible_node_and_degenerate_shapes():
    z = np.zeros(100, np.int64)
    assert pack_pick(np.zeros((3, 2), np.uint64), np.full((3, 4), 0xFFFFFFFF, np.uint32), 100, z, z).tolist() == [-1, -1, -1]
    e = np.zeros(0, np.int64)
    assert pack_pick(np.zeros((2, 0), np.uint64), np.ones((2, 3), np.uint32), 0, e, e).tolist() == [-1, -1]
    assert pack_pick(np.zeros((0, 2), np.uint64), np.zeros((0, 2), np.uint32), 100, z, z).shape == (0,)
    assert tightest_of(np.zeros((0, 3), np.int64), z, z).shape == (0,)
    # padding bits and words are no candidates: n = 70, only node 5 is real
    ones = 0xFFFFFFFFFFFFFFFF
    m = row([1 << 5, ones & ~0x3F, ones])
    big = -np.arange(70, dtype=np.int64)
    assert pack_pick(m, np.array([[0, 0x80000000, 0xFFFFFFFF]], np.uint32), 70, big, big)[0] == 5
