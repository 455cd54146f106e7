"""Mask rows that reach the edges of k_pick_uniform's own structure, each with the binding the contract of KSCHED_PICK_UNIFORM
(include/ksched.h) gives for a draw u, written as a closed form that does not go through tests/uniform_ref.py.

The kernel (csrc/kernels_pick_uniform.hpp) gives lane l of a wave words 2l and 2l + 1 of every 128-word chunk of a row, adds the lanes'
counts with a prefix sum over DPP rows of 16 lanes, keeps a row of W <= 128 words in registers and walks a longer one twice (a counting
pass unrolled by four chunks, then a pass that stops in the chunk that holds set bit number k).  Its edges, as node indices: 63 / 64 (the
two words of a lane), 127 / 128 (two lanes), 2047 / 2048, 4095 / 4096 and 6143 / 6144 (the DPP rows: lanes 15 / 16, 31 / 32, 47 / 48),
8191 / 8192 and every further multiple of 8192 (two chunks).

tests/test_uniform_rows_host.py pins every closed form here against uniform_pick (no GPU); tests/test_gpu_uniform_rows.py runs the rows
through ksched_pick_device and ksched_pick."""
import numpy as np

# n -> what it reaches (W = ceil(n / 64))
NODE_COUNTS = [8191,   # W = 128: register path, last word has 63 valid bits
               8192,   # W = 128: register path, longest row, last word full
               8193,   # W = 129: shortest two-pass row, second chunk holds one valid bit
               8256,   # W = 129: two-pass row with a full last word
               16384,  # W = 256: exactly two chunks
               16385,  # W = 257: three chunks, the last with one valid bit
               32769]  # W = 513: five chunks, one trip past the unrolled four of the counting pass
DRAWS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
SINGLE_BITS = [0, 63, 64, 127, 128, 8127, 8128, 8191, 8192]  # and n - 1
EDGE_PAIRS = [(63, 64), (127, 128), (2047, 2048), (4095, 4096), (6143, 6144), (8191, 8192), (16383, 16384)]
# (n, density) of the rows whose every set bit is reached: one pod per set bit, so the densest long row (16 385 pods x 257 words = 34 MB)
# is the largest mask
REACH = [(n, d) for n in (8191, 8192, 8193, 8256) for d in (0.02, 0.5, 1.0)] + [(16385, 0.02), (16385, 1.0), (32769, 0.02)]
CHUNK_NODES = 128 * 64
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def words(n):
    return (n + 63) // 64


def row_of(n, nodes):
    """the row of n nodes with exactly `nodes` set"""
    r = np.zeros(words(n), np.uint64)
    nodes = np.asarray(nodes, dtype=np.int64)
    assert nodes.size == 0 or (0 <= nodes.min() and nodes.max() < n)
    np.bitwise_or.at(r, nodes >> 6, np.uint64(1) << (nodes & 63).astype(np.uint64))
    return r


def structured_rows(n):
    """-> [(name, row [W] uint64 with no bit at or beyond n, expect)]: expect(u) is the binding for the 32-bit draw u"""
    W = words(n)
    out = []
    for j in sorted({j for j in SINGLE_BITS + [n - 1] if j < n}):
        out.append((f"bit {j}", row_of(n, [j]), lambda u, j=j: j))
    for lo, hi in EDGE_PAIRS:
        if hi < n:
            out.append((f"bits {lo} and {hi}", row_of(n, [lo, hi]), lambda u, lo=lo, hi=hi: lo if u < (1 << 31) else hi))
    # one bit per word: bit (7w) mod 64 of word w, bit 0 of the last word (which may hold one valid bit only) -- c = W
    offset = lambda w: 0 if w == W - 1 else (7 * w) % 64  # noqa: E731
    out.append(("one bit per word", row_of(n, [64 * w + offset(w) for w in range(W)]), lambda u: 64 * ((u * W) >> 32) + offset((u * W) >> 32)))
    out.append(("every valid bit", row_of(n, np.arange(n)), lambda u: (u * n) >> 32))
    if W > 128:
        # the first chunk empty: every third node from 8192 on
        beyond = np.arange(CHUNK_NODES, n, 3)
        out.append(("bits only at or beyond word 128", row_of(n, beyond), lambda u, c=beyond.size: CHUNK_NODES + 3 * ((u * c) >> 32)))
        # the second pass returns in its first trip: every fifth node below 8192
        first = np.arange(0, CHUNK_NODES, 5)
        out.append(("bits only in chunk 0", row_of(n, first), lambda u, c=first.size: 5 * ((u * c) >> 32)))
    out.append(("all zero", np.zeros(W, np.uint64), lambda u: -1))
    return out


def structured_batch(n):
    """the structured rows of n under every draw of DRAWS, ordered draw-major so that neighbouring pods (the four of a block) carry
    different rows.  -> names [p], valid [p, W] uint64, draws [p] uint32, want [p] int32 (from the closed forms)"""
    rows = structured_rows(n)
    R = len(rows)
    assert R >= 4
    names = [f"{rows[i % R][0]}, u = {DRAWS[i // R]:#x}" for i in range(R * len(DRAWS))]
    valid = np.tile(np.stack([r for _, r, _ in rows]), (len(DRAWS), 1))
    draws = np.repeat(np.array(DRAWS, np.uint32), R)
    want = np.array([rows[i % R][2](int(draws[i])) for i in range(R * len(DRAWS))], np.int32)
    return names, valid, draws, want


def reach_batch(n, density, seed):
    """One random row of about `density` set bits at pos[0 .. c), and the two draws per set bit that bound its interval: with
    u = ceil(j * 2^32 / c), k = (u * c) >> 32 = j, and with u = ceil((j + 1) * 2^32 / c) - 1 still k = j.  Pod j of either batch carries
    the row and draw j: the expected bindings are pos itself.  -> row [W] uint64, pos [c] int32, lo [c] uint32, hi [c] uint32"""
    rng = np.random.default_rng([seed, n])
    pos = np.arange(n) if density >= 1.0 else np.nonzero(rng.random(n) < density)[0]
    c = int(pos.size)
    assert c >= 1
    j = np.arange(c + 1, dtype=np.uint64)  # (j * 2^32 < 2^48)
    ceil = ((j << np.uint64(32)) + np.uint64(c - 1)) // np.uint64(c)  # ceil(j * 2^32 / c), j = 0 .. c
    lo, hi = ceil[:-1], ceil[1:] - np.uint64(1)
    assert (hi < (1 << 32)).all() and (lo <= hi).all()
    return row_of(n, pos), pos.astype(np.int32), lo.astype(np.uint32), hi.astype(np.uint32)


def padded(valid, n, pitch, ones):
    """[p, pitch] host rows: `valid` in the first W words; the padding bits of the last word and the words [W, pitch) all zero or all ones"""
    p, W = valid.shape
    assert W == words(n) and pitch >= W
    host = np.full((p, pitch), ONES if ones else np.uint64(0), np.uint64)
    host[:, :W] = valid
    if ones and n & 63:
        host[:, W - 1] |= ~np.uint64((1 << (n & 63)) - 1)
    return host
