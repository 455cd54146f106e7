"""tests/uniform_rows.py, the structured mask rows of tests/test_gpu_uniform_rows.py, pinned against tests/uniform_ref.py: every builder's
closed-form expectation equals the restatement, at every node count the GPU test uses, with the padding all zero and all ones.  This is
the condition that the GPU test's inputs are what they claim to be.  No GPU, no library."""
import numpy as np
import pytest

from tests import uniform_rows as R
from tests.uniform_ref import uniform_pick, uniform_pick_blocks


def test_node_counts_reach_what_they_claim():
    assert [R.words(n) for n in R.NODE_COUNTS] == [128, 128, 129, 129, 256, 257, 513]
    assert [n & 63 for n in R.NODE_COUNTS] == [63, 0, 1, 0, 0, 1, 1]


@pytest.mark.parametrize("n", R.NODE_COUNTS)
def test_structured_rows_closed_forms_equal_the_restatement(n):
    names, valid, draws, want = R.structured_batch(n)
    W = R.words(n)
    assert valid.shape == (len(names), W) and len(set(names)) == len(names)
    # no builder sets a bit at or beyond n; the rows it names exist
    if n & 63:
        assert not (valid[:, W - 1] >> np.uint64(n & 63)).any()
    have = {nm.split(",")[0] for nm in names}
    assert {"bit 0", f"bit {n - 1}", "bits 63 and 64", "bits 6143 and 6144", "one bit per word", "every valid bit", "all zero"} <= have
    assert ("bits only in chunk 0" in have) == (W > 128) == ("bits only at or beyond word 128" in have) == ("bit 8192" in have)
    assert ("bits 8191 and 8192" in have) == (n > 8192) and ("bits 16383 and 16384" in have) == (n > 16384)
    # four neighbouring pods carry four different rows
    per = len(names) // len(R.DRAWS)
    assert all(len({names[i + q].split(",")[0] for q in range(4)}) == 4 for i in range(0, len(names) - 3) if (i % per) + 3 < per)
    got = uniform_pick(valid, draws, n)
    bad = [names[i] for i in np.nonzero(got != want)[0]]
    assert not bad, bad
    for pitch, ones in ((W, True), (W + 1, True), (W + 3, False)):  # the padding changes nothing
        assert np.array_equal(uniform_pick(R.padded(valid, n, pitch, ones), draws, n), want), (pitch, ones)
    # every outcome appears: -1, the lowest and the highest node
    assert want.min() == -1 and 0 in want and n - 1 in want


@pytest.mark.parametrize("n,density", [(130, 0.02), (130, 0.5), (130, 1.0)] + R.REACH)
def test_reach_draws_select_every_set_bit_at_both_ends_of_its_interval(n, density):
    row, pos, lo, hi = R.reach_batch(n, density, seed=0x2EAC)
    c = pos.size
    assert abs(c - density * n) <= max(4.0, 0.25 * density * n) and (np.diff(pos) > 0).all()
    assert lo[0] == 0 and hi[-1] == 0xFFFFFFFF and (lo[1:] == hi[:-1].astype(np.uint64) + 1).all()  # the intervals tile [0, 2^32)
    mask = np.broadcast_to(row, (c, row.size))
    assert np.array_equal(uniform_pick_blocks(mask, lo, n), pos)
    assert np.array_equal(uniform_pick_blocks(mask, hi, n), pos)


def test_blocks_equal_the_whole():
    rng = np.random.default_rng(3)
    m = rng.integers(0, 1 << 63, (50, 4), dtype=np.uint64) & rng.integers(0, 1 << 63, (50, 4), dtype=np.uint64)
    u = rng.integers(0, 1 << 32, 50, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(uniform_pick_blocks(m, u, 250, cells=250 * 7), uniform_pick(m, u, 250))
