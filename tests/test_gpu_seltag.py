"""KSCHED_SELOP_TAGGED (extension E9) on the GPU, bit for bit against tests/seltag_ref.py (pinned by tests/test_seltag_restatement.py), with
tests/combine_ref.py / tests/soft_ref.py, the calls that exist already and ksched_pick_device on top of it.
 1. mask parity at the word, wave and block edges of the kernel's mapping (n), the tile edges of its pod walk (p) and each side of its key
    passes (keys), into packed rows, rows at ksched_mask_pitch(n) and views that start one word into their buffer, and one shape in which a
    block walks more than one pod tile; node ids on both sides of 2^29 and of the sign bit, entries of all six tags, tags 6 and 7 and
    NEVER; what the cases tell apart is asserted on the EXPECTED values before the device is asked;
 2. agreement with what exists: untagged entries == the plain KSCHED_SEL mask; entries all GT / LT / EXISTS == the operator call; one NE
    or ABSENT entry per pod == AND-NOT of the equality / EXISTS call; a mixed batch == the four-call sequence it replaces;
 3. the call under AND, OR, AND-NOT and the soft modifier into a caller's mask with garbage beyond n; each of the five picks in a tagged
    call, plain and combining == ksched_pick_device on the resulting mask; the header's recipe;
 4. the host forms ksched_eval and ksched_eval_begin / _end give the device form's bits;
 5. label updates within the planned maxima and past them, another key count, and two streams around a label update;
 6. the refusals at every entry point, outputs untouched, and the edge sizes p == 0, n == 0, no snapshot.
Every output goes into sentinel-filled buffers with guard rows.  Shapes are the smallest at which the kernel takes each path.  What the three selector
files share -- the guarded evaluation, the bodies that are the same for every call -- is tests/selector_calls.py's."""
import ctypes as C

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (COMBINE_AND, COMBINE_ANDNOT, COMBINE_OR, COMBINE_SOFT, FIT, PICK_BESTFIT, PICK_SAMPLED, PICK_SPREAD, PICK_UNIFORM,
                                             SEL, SEL_NEVER, SELOP_EXISTS, SELOP_GT, SELOP_LT, SELOP_TAGGED, SELTAG_ABSENT, SELTAG_EQ, SELTAG_EXISTS, SELTAG_GT,
                                             SELTAG_ID_MASK, SELTAG_LT, SELTAG_NE, SELTAG_SHIFT, TAINT, WANT_FIT_MASK, Evaluator, _lib, pack_mask, seltag, synth)
from tests import combine_ref, selector_calls, seltag_ref
from tests.pick_helpers import dev_of, fresh, mask_np, oracle_mask, pod_tensors, to_dev
from tests.selector_calls import (COMBINES, CORES_KEY, GPU_KEY, PICKS, SENTINEL, ZONE_3, ZONE_KEY, SelectorCall, as_signed, ev, eval_into_view, indexed_cluster,  # noqa: F401 (ev: the fixture)
                                  recipe_cluster, row_kinds, zeros_dev)

pytestmark = pytest.mark.gpu

T = SEL | SELOP_TAGGED
CALL = SelectorCall(T, "seltag", seltag_ref.seltag_mask)
EQ, NE, EX, AB, GT, LT = seltag_ref.TAGS
# what a node carries: 0 = not the key; ids on both sides of 2^29 (an entry cannot name those at or above it) and of the sign bit
IDS = np.array([0, 1, 2, 3, 0x1FFFFFFF, 0x20000000, 0x20000001, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)
ENTRY_IDS = np.array([0, 1, 2, 3, 4, 0x1FFFFFFF], dtype=np.uint32)  # what an entry's id field holds


def test_the_constants_are_the_restatements():
    assert (SELOP_TAGGED, SELTAG_SHIFT, SELTAG_ID_MASK, SEL_NEVER) == (seltag_ref.TAGGED, seltag_ref.SHIFT, seltag_ref.ID_MASK, seltag_ref.NEVER)
    assert (SELTAG_EQ, SELTAG_NE, SELTAG_EXISTS, SELTAG_ABSENT, SELTAG_GT, SELTAG_LT) == seltag_ref.TAGS
    ids = np.array([0, 1, 5, SELTAG_ID_MASK])
    for tag in seltag_ref.TAGS:
        assert np.array_equal(seltag(tag, ids), seltag_ref.entry(tag, ids))


# ---- 1. mask parity -----------------------------------------------------------------------------------------------------------------------
NODES = [1, 63, 64, 65, 1023, 1024, 1025, 4097]  # a word, a wave's four words and a block's sixteen, each side; several blocks
PODS = [1, 63, 64, 65, 129]                      # a tile of 64 pods, each side; more than two tiles
KEYS = [1, 8, 9, 32]                             # one pass of eight keys, each side; KSCHED_MAX_KEYS
P_MAX = max(PODS)
_CASES = {}


def entries_for(rng, keys, p):
    """[keys][p] tagged entries: each (pod, key) constrained with probability min(0.3, 2 / keys); of the constrained ones 1 in 16 is tag 6,
    tag 7 or NEVER, the rest one of the six tags, uniformly; the id field from ENTRY_IDS whatever the tag (EXISTS and ABSENT must not look
    at it).  Every eighth pod of a snapshot with more than eight keys constrains a key on each side of the pass boundary, each by a rule
    that passes some nodes and not others."""
    constrained = rng.random((keys, p)) < min(0.3, 2.0 / keys)
    tags = rng.integers(0, 6, size=(keys, p))
    odd = rng.integers(0, 48, size=(keys, p))
    ids = ENTRY_IDS[rng.integers(0, ENTRY_IDS.size, size=(keys, p))]
    sel = seltag_ref.entry(tags, ids)
    sel = np.where(odd == 0, seltag_ref.entry(6, ids), sel)
    sel = np.where(odd == 1, seltag_ref.entry(7, ids), sel)
    sel = np.where(odd == 2, np.uint32(SEL_NEVER), sel)
    sel = np.where(constrained, sel, np.uint32(0)).astype(np.uint32)
    if keys > 8:
        for pod in range(4, p, 8):
            sel[:, pod] = 0
            sel[int(rng.integers(0, 8)), pod] = seltag_ref.entry(rng.choice([NE, EX, GT]), rng.choice([1, 2, 3]))
            sel[int(rng.integers(8, keys)), pod] = seltag_ref.entry(rng.choice([NE, AB, LT, EX]), rng.choice([2, 3, 4]))
    return sel


def case(n, keys, p=P_MAX):
    """labels [keys][n] drawn from IDS, entries [keys][p] by entries_for, and the expected mask; computed once, read-only"""
    if (n, keys, p) not in _CASES:
        rng = np.random.default_rng([0xE9, n, keys, p])
        lab = IDS[rng.integers(0, IDS.size, size=(keys, n))]
        sel = entries_for(rng, keys, p)
        want = seltag_ref.seltag_mask(lab, sel)
        for a in (lab, sel, want):
            a.setflags(write=False)
        _CASES[(n, keys, p)] = dict(lab=lab, sel=sel, want=want)
    return _CASES[(n, keys, p)]


def wrong_pair(kind, e, v):
    """the table as a WRONG kernel of the named kind would compute it, for constrained entries e [pods, 1] and node ids v [1, n]"""
    tag, ident = e >> np.uint64(SELTAG_SHIFT), e & np.uint64(SELTAG_ID_MASK)
    if kind == "v masked to 29 bits":
        return seltag_ref.pair(e, v & np.uint64(SELTAG_ID_MASK))
    right = seltag_ref.pair(e, v)
    if kind == "a signed compare":
        wrong = np.where(tag == GT, (v != 0) & (as_signed(v) > as_signed(ident)), (v != 0) & (as_signed(v) < as_signed(ident)))
        return np.where((tag == GT) | (tag == LT), wrong, right)
    if kind == "LT or GT letting absent nodes through":
        return np.where(tag == GT, v > ident, np.where(tag == LT, v < ident, right))
    if kind == "NE or ABSENT failing absent nodes":
        return np.where((tag == NE) | (tag == AB), right & (v != 0), right)
    if kind == "tags 6 and 7 read as EQ":
        return np.where(tag >= 6, v == ident, right)
    if kind == "EXISTS or ABSENT looking at the id field":
        inside = (v != 0) & (v >= ident)  # the range starting at the id, where it starts at 1
        return np.where(tag == EX, inside, np.where(tag == AB, ~inside, right))
    raise KeyError(kind)


WRONG_KINDS = ["v masked to 29 bits", "a signed compare", "LT or GT letting absent nodes through", "NE or ABSENT failing absent nodes",
               "tags 6 and 7 read as EQ", "EXISTS or ABSENT looking at the id field"]


def wrong_mask(kind, lab, sel):
    lab, sel = lab.astype(np.uint64), sel.astype(np.uint64)
    ok = np.ones((sel.shape[1], lab.shape[1]), dtype=bool)
    for k in range(lab.shape[0]):
        pods = np.nonzero(sel[k])[0]
        if pods.size:
            ok[pods] &= wrong_pair(kind, sel[k][pods][:, None], lab[k][None, :])
    return seltag_ref.pack(ok)


def unmasked_padding(lab, sel):
    """the rows of a kernel that does not clear the lanes at or beyond n: they hold id 0, which NE and ABSENT pass"""
    n = lab.shape[1]
    W = (n + 63) // 64
    padded = np.zeros((lab.shape[0], W * 64), dtype=np.uint32)
    padded[:, :n] = lab
    return seltag_ref.seltag_mask(padded, sel)


_FACTS = {}


def matrix_facts():
    """What the matrix contains, from the expected values alone -- asserted before any device call, so that no case can pass vacuously."""
    if _FACTS:
        return _FACTS
    differs = {kind: 0 for kind in WRONG_KINDS + ["NE or ABSENT leaving bits at or beyond n set"]}
    tags_in_mixed_rows, shapes = set(), {}
    full = empty = 0
    for n in NODES:
        for keys in KEYS:
            k = case(n, keys)
            want = k["want"]
            for kind in WRONG_KINDS:
                differs[kind] += int((wrong_mask(kind, k["lab"], k["sel"]) != want).any())
            differs["NE or ABSENT leaving bits at or beyond n set"] += int((unmasked_padding(k["lab"], k["sel"]) != want).any())
            f, e, m = row_kinds(want, n)
            full, empty = full + f, empty + e
            shapes[(n, keys)] = m / P_MAX
            count = np.unpackbits(want.view(np.uint8), axis=1).sum(axis=1)
            for pod in np.nonzero((count > 0) & (count < n))[0]:
                tags_in_mixed_rows.update(int(e_) >> SELTAG_SHIFT for e_ in k["sel"][:, pod] if e_)
    _FACTS.update(differs=differs, tags=tags_in_mixed_rows, shapes=shapes, full=full, empty=empty)
    return _FACTS


def check_matrix_facts():
    f = matrix_facts()
    for kind, cases in f["differs"].items():
        assert cases >= 1, f"no case of the matrix tells the kernel from one with {kind}"
    assert f["full"] >= 1 and f["empty"] >= 1
    for (n, keys), mixed in f["shapes"].items():
        if n > 1 and keys >= 4:
            assert mixed >= 0.5, f"n = {n}, keys = {keys}: only {mixed:.0%} of the rows are neither empty nor full"
        elif n > 1:
            assert mixed >= 0.1, f"n = {n}, keys = {keys}: only {mixed:.0%} of the rows are neither empty nor full"
    assert set(seltag_ref.TAGS) <= f["tags"], "every tag occurs in a row that is neither empty nor full"
    crossing = 0
    for keys in (9, 32):
        sel = case(65, keys)["sel"]
        crossing += int(((sel[:8] != 0).any(axis=0) & (sel[8:] != 0).any(axis=0)).sum())
    assert crossing >= 2 * (P_MAX // 8), "pods that constrain keys on both sides of the 8-key pass boundary"


def test_the_matrix_tells_the_kernel_from_each_wrong_one():
    check_matrix_facts()


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("n", NODES)
def test_mask_parity(ev, n, keys):
    check_matrix_facts()
    k = case(n, keys)
    W = (n + 63) // 64
    assert k["want"].shape == (P_MAX, W) and not (k["want"][:, -1] & ~np.uint64(combine_ref.valid_bits_word(n))).any()
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    assert ev.W == W
    std = int(_lib.load().ksched_mask_pitch(n))
    assert std % 16 == 0 and std >= W
    for p in PODS:
        for pitch, offset in ((W, 0), (std, 0), (W, 1), (std, 1)):
            got = eval_into_view(ev, k["sel"], T, n, p, pitch, offset)
            want = k["want"][:p]
            assert np.array_equal(got, want), f"p = {p}, pitch {pitch}, offset {offset}: pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from seltag_ref"
            assert ev.last_kernel == "seltag" and ev.last_pick == "none"


def test_a_block_that_walks_more_than_one_pod_tile(ev):
    """1024 column blocks leave two block rows for three pod tiles: the first block row walks two tiles, the second one"""
    n, keys, p = 16 * 64 * 1024 - 37, 2, 130
    W = (n + 63) // 64
    gx = (W + 15) // 16
    want_rows = (2048 + gx - 1) // gx
    tiles = (p + 63) // 64
    assert gx == 1024 and want_rows == 2 < tiles == 3, "pod_tiles_per_block == 2"
    k = case(n, keys, p)
    assert row_kinds(k["want"], n)[2] >= p // 4
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    got = eval_into_view(ev, k["sel"], T, n, p, W, 1)
    assert np.array_equal(got, k["want"]), f"pods {np.nonzero((got != k['want']).any(axis=1))[0][:5]} differ from seltag_ref"


def test_no_selectors_and_no_keys_pass_every_node(ev):
    selector_calls.no_selectors_and_no_keys_pass_every_node(ev, [CALL], [CALL], 0xE90, IDS)


# ---- 2. agreement with what exists ------------------------------------------------------------------------------------------------------------
def unindexed_cluster():
    """three high-cardinality keys: no bitmap index (tests/test_gpu_summary.py's builder); ids below 2^29"""
    rng = np.random.default_rng(0xE8002)
    N, P = 700, 129
    lab = rng.integers(1, 4_000_000, size=(3, N)).astype(np.uint32)
    lab[:, ::7] = 0
    sel = np.zeros((3, P), dtype=np.uint32)
    sel[0, ::3] = lab[0, rng.integers(0, N, size=len(sel[0, ::3]))]
    sel[2, ::4] = lab[2, rng.integers(0, N, size=len(sel[2, ::4]))]
    sel[2, 2::8] = rng.integers(1, 4_000_000, size=len(sel[2, 2::8]))
    sel[1, 5::16] = SEL_NEVER
    return rng.integers(0, 1000, N).astype(np.int64), rng.integers(0, 1000, N).astype(np.int64), lab, sel


def retag(sel, tag):
    """every constrained entry but NEVER under `tag`"""
    plain = (sel != 0) & (sel != SEL_NEVER)
    return np.where(plain, seltag_ref.entry(tag, sel & SELTAG_ID_MASK), sel).astype(np.uint32)


@pytest.mark.parametrize("kind", ["indexed", "unindexed"])
def test_untagged_entries_give_the_plain_selector_mask(ev, kind):
    cpu, mem, lab, sel = indexed_cluster() if kind == "indexed" else unindexed_cluster()
    n, p = lab.shape[1], sel.shape[1]
    assert lab.max() < 1 << 29 and ((sel == SEL_NEVER) | (sel < 1 << 29)).all(), "untagged entries ARE tag EQ, and NEVER is tag 7"
    want = seltag_ref.seltag_mask(lab, sel)
    assert row_kinds(want, n)[2] > p // 8
    ev.set_nodes(cpu, mem, lab)
    assert (ev.index_checksum() != (0, 0)) == (kind == "indexed")
    W = (n + 63) // 64
    for kernel in ("auto", "direct", "fused"):
        ev.set_kernel(kernel)  # (no effect on a tagged call: the fused kernel forced on an unindexed snapshot is no refusal here)
        got = eval_into_view(ev, sel, T, n, p, W, 0)
        assert np.array_equal(got, want), f"{kind}, {kernel}"
        assert ev.last_kernel == "seltag"
        if kernel == "fused" and kind == "unindexed":
            continue  # (the PLAIN call cannot be forced onto the fused kernel without an index)
        plain = eval_into_view(ev, sel, SEL, n, p, W, 0)
        assert ev.last_kernel in ("direct", "fused") and (kernel == "auto" or ev.last_kernel == kernel)
        assert np.array_equal(got, plain), f"{kind}, {kernel}: the tagged call and the plain KSCHED_SEL call differ on untagged entries"
    ev.set_kernel("auto")


@pytest.mark.parametrize("tag,op", [(GT, SELOP_GT), (LT, SELOP_LT), (EX, SELOP_EXISTS)], ids=["gt", "lt", "exists"])
def test_entries_of_one_tag_give_the_operator_calls_mask(ev, tag, op):
    cpu, mem, lab, sel = indexed_cluster()
    n, p = lab.shape[1], sel.shape[1]
    W = (n + 63) // 64
    tagged = retag(sel, tag)
    want = seltag_ref.seltag_mask(lab, tagged)
    assert row_kinds(want, n)[2] > p // 8
    ev.set_nodes(cpu, mem, lab)
    got = eval_into_view(ev, tagged, T, n, p, W, 0)
    assert ev.last_kernel == "seltag"
    by_op = eval_into_view(ev, sel, SEL | op, n, p, W, 0)
    assert ev.last_kernel == "selop"
    assert np.array_equal(got, want) and np.array_equal(got, by_op)


@pytest.mark.parametrize("tag,op", [(NE, 0), (AB, SELOP_EXISTS)], ids=["ne", "absent"])
def test_one_negated_entry_per_pod_is_andnot_of_the_positive_call(ev, tag, op):
    import torch
    cpu, mem, lab, sel = indexed_cluster()
    n, p = lab.shape[1], sel.shape[1]
    W = (n + 63) // 64
    one = np.zeros_like(sel)  # per pod ONE entry: its first constrained one, or (a pod without any) the id some node carries
    for pod in range(p):
        ks = np.nonzero((sel[:, pod] != 0) & (sel[:, pod] != SEL_NEVER))[0]
        if ks.size:
            one[ks[0], pod] = sel[ks[0], pod]
        else:
            one[pod % lab.shape[0], pod] = max(1, int(lab[pod % lab.shape[0], pod % n]))
    assert ((one != 0).sum(axis=0) == 1).all(), "a pod without an entry would pass every node here and none under AND-NOT"
    tagged = retag(one, tag)
    want = seltag_ref.seltag_mask(lab, tagged)
    assert row_kinds(want, n)[2] > p // 4
    ev.set_nodes(cpu, mem, lab)
    got = eval_into_view(ev, tagged, T, n, p, W, 0)
    M = torch.full((p, W), -1, dtype=torch.int64, device=dev_of(ev))  # all-valid, and garbage beyond n
    ev.eval_device(zeros_dev(ev, p), zeros_dev(ev, p), to_dev(ev, one, np.int32), None, None, SEL | op | COMBINE_ANDNOT, out_feasible=M)
    torch.cuda.synchronize()
    assert np.array_equal(got, want) and np.array_equal(got, mask_np(M))


def mixed_batch(sel):
    """pod j's constrained entries under EQ, EXISTS, GT or LT by j % 4; the four untagged selector arrays of the sequence it replaces"""
    p = sel.shape[1]
    tagged = np.zeros_like(sel)
    parts = []
    for q, tag in enumerate((EQ, EX, GT, LT)):
        mine = np.zeros_like(sel)
        mine[:, q::4] = sel[:, q::4]
        parts.append(mine)
        tagged[:, q::4] = retag(sel[:, q::4], tag)
    assert p >= 8
    return tagged, parts


def test_a_mixed_batch_is_the_four_call_sequence_it_replaces(ev):
    import torch
    cpu, mem, lab, sel = indexed_cluster()
    n, p = lab.shape[1], sel.shape[1]
    W = (n + 63) // 64
    tagged, parts = mixed_batch(sel)
    want = seltag_ref.seltag_mask(lab, tagged)
    assert row_kinds(want, n)[2] > p // 4
    ev.set_nodes(cpu, mem, lab)
    got = eval_into_view(ev, tagged, T, n, p, W, 0)
    assert ev.last_kernel == "seltag"
    M = torch.full((p, W), 0x5A, dtype=torch.int64, device=dev_of(ev))
    c0, c1 = zeros_dev(ev, p), zeros_dev(ev, p)
    ev.eval_device(c0, c1, to_dev(ev, parts[0], np.int32), None, None, SEL, out_feasible=M)
    for part, op in zip(parts[1:], (SELOP_EXISTS, SELOP_GT, SELOP_LT)):
        ev.eval_device(c0, c1, to_dev(ev, part, np.int32), None, None, SEL | op | COMBINE_AND, out_feasible=M)
    torch.cuda.synchronize()
    assert np.array_equal(got, want) and np.array_equal(got, mask_np(M))


def test_timing_brackets_the_tagged_kernel(ev):
    cpu, mem, lab, sel = indexed_cluster()
    ev.set_nodes(cpu, mem, lab)
    p = sel.shape[1]
    ev.set_timing(True)
    try:
        ev.kernel_time_ms()  # (reading the samples resets them)
        eval_into_view(ev, retag(sel, NE), T, lab.shape[1], p, ev.W, 0)
        ms, count = ev.kernel_time_ms()
        assert count == 1 and ms > 0, "one pair of stream events around the tagged kernel"
    finally:
        ev.set_timing(False)


# ---- 3. combining and picks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comb,comb_id", COMBINES, ids=[c[1] for c in COMBINES])
def test_the_tagged_call_under_every_combine(ev, comb, comb_id):
    k = case(1025, 9)
    selector_calls.the_call_under_every_combine(ev, CALL, k["lab"], k["sel"], k["want"], comb, np.random.default_rng([0xE93, comb]))


@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
def test_the_recipe_end_to_end(ev, pitched):
    """gpu Exists AND cores Gt 16 AND zone NotIn {z3} is ONE row and ONE call; then KSCHED_FIT | KSCHED_COMBINE_AND | the spread pick"""
    import torch
    c, lab = recipe_cluster(0xE9C4)
    P, N = c.P, c.N
    fits = (c.req_cpu[:, None] <= c.avail_cpu[None, :]) & (c.req_mem[:, None] <= c.avail_mem[None, :])
    gpu, cores, zone = lab[GPU_KEY], lab[CORES_KEY].astype(np.int64) - 1, lab[ZONE_KEY]
    ok_nodes = (gpu != 0) & (lab[CORES_KEY] != 0) & (cores > 16) & (zone != ZONE_3)  # (a node without a zone is not in z3: it passes NotIn)
    bits = fits & ok_nodes[None, :]
    assert 0 < ok_nodes.sum() < N and ((zone == 0) & ok_nodes).any() and ((lab[CORES_KEY] == 0) & (gpu != 0) & (zone != ZONE_3)).any() and ((cores == 16) & (gpu != 0)).any()
    assert P // 4 < bits.any(axis=1).sum() < P, "pods with a node and pods without one"
    want = pack_mask(bits)
    ev.set_nodes(c.avail_cpu, c.avail_mem, lab)
    cpu, mem = to_dev(ev, c.req_cpu, np.int64), to_dev(ev, c.req_mem, np.int64)
    row = np.zeros((c.n_keys, P), dtype=np.uint32)
    row[GPU_KEY] = seltag(SELTAG_EXISTS, 0)
    row[CORES_KEY] = seltag(SELTAG_GT, 16 + 1)
    row[ZONE_KEY] = seltag(SELTAG_NE, ZONE_3)
    draws = np.random.default_rng(0xE9C5).integers(0, 1 << 32, size=(P, 3), dtype=np.uint64).astype(np.uint32)
    smp = to_dev(ev, draws, np.int32)
    M = ev.alloc_mask(P, pitched=pitched)
    M.fill_(-1)  # whatever the mask held before the chain
    out = fresh(ev, P, 4)
    ev.eval_device(cpu, mem, to_dev(ev, row, np.int32), None, None, T, out_feasible=M)
    ev.eval_device(cpu, mem, None, None, smp, FIT | COMBINE_AND | PICK_SPREAD, out_feasible=M, out_binding=out[:P])
    alone = fresh(ev, P)
    ev.pick_device(to_dev(ev, want, np.int64), PICK_SPREAD, alone, samples=smp)
    torch.cuda.synchronize()
    got = mask_np(M)
    assert np.array_equal(got, want), f"pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from the label columns' answer"
    b = out.cpu().numpy()
    assert np.array_equal(b[:P], alone.cpu().numpy()) and (b[P:] == -7).all()
    assert ((b[:P] >= 0) == bits.any(axis=1)).all() and bits[np.nonzero(b[:P] >= 0)[0], b[:P][b[:P] >= 0]].all()


_PICK_CASE = {}


def pick_case():
    if not _PICK_CASE:
        P, N = 300, 700
        c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=0xE9B1C)
        rng = np.random.default_rng(0xE9B1)
        sel = np.ascontiguousarray(c.pod_sel).copy()
        tags = rng.integers(0, 6, size=sel.shape)
        sel = np.where(sel != 0, seltag_ref.entry(tags, sel & SELTAG_ID_MASK), 0).astype(np.uint32)
        sel[3, 1::9] = SEL_NEVER  # pods without a node
        old = pack_mask(rng.random((P, N)) < 0.4)
        draws = rng.integers(0, 1 << 32, size=(P, 5), dtype=np.uint64).astype(np.uint32)
        new = seltag_ref.seltag_mask(c.node_labels, sel)
        for a in (sel, old, draws, new):
            a.setflags(write=False)
        _PICK_CASE.update(c=c, sel=sel, old=old, draws=draws, new=new)
    return _PICK_CASE


@pytest.mark.parametrize("pick,last_pick", PICKS, ids=["sampled", "bestfit", "uniform", "spread", "pack"])
def test_a_pick_in_a_tagged_call_is_the_pick_from_the_resulting_mask(ev, pick, last_pick):
    selector_calls.a_pick_in_the_call_is_the_pick_from_the_resulting_mask(ev, CALL, pick_case(), pick_case()["new"], pick, last_pick)


# ---- 4. the host forms --------------------------------------------------------------------------------------------------------------------------
def test_the_host_forms_give_the_device_forms_bits(ev):
    selector_calls.the_host_forms_give_the_device_forms_bits(ev, CALL, pick_case(), pick_case()["new"])


# ---- 5. snapshot changes ------------------------------------------------------------------------------------------------------------------------
def snapshot_case(seed):
    c = synth.make_cluster(129, 1100, n_keys=8, n_taints=0, seed=seed)
    rng = np.random.default_rng(seed)
    sel = np.ascontiguousarray(c.pod_sel)
    sel = np.where(sel != 0, seltag_ref.entry(rng.integers(0, 6, size=sel.shape), sel & SELTAG_ID_MASK), 0).astype(np.uint32)
    return c, sel, rng


def test_label_updates_another_key_count_and_a_fresh_evaluator(built):
    c, sel, rng = snapshot_case(0xE96)
    lab = c.node_labels.copy()
    n, p = c.N, c.P
    W = (n + 63) // 64
    e = Evaluator(0)
    try:
        e.set_nodes(c.avail_cpu, c.avail_mem, lab)
        assert np.array_equal(eval_into_view(e, sel, T, n, p, W, 0), seltag_ref.seltag_mask(lab, sel))
        # within the planned maxima: ids the keys already have, and nodes that lose a key
        idx = rng.choice(n, size=200, replace=False).astype(np.uint32)
        rows = rng.integers(0, lab.max(axis=1)[:, None] + 1, size=(8, idx.size)).astype(np.uint32)
        before = seltag_ref.seltag_mask(lab, sel)
        lab[:, idx] = rows
        assert not np.array_equal(before, seltag_ref.seltag_mask(lab, sel)), "the update shows in the mask"
        e.update_node_labels(idx, rows)
        assert np.array_equal(eval_into_view(e, sel, T, n, p, W, 0), seltag_ref.seltag_mask(lab, sel)), "after an update within the planned maxima"
        # past them: ids above every planned maximum (the layout is planned again)
        idx = rng.choice(n, size=300, replace=False).astype(np.uint32)
        rows = rng.integers(0, 5000, size=(8, idx.size)).astype(np.uint32)
        lab[:, idx] = rows
        assert (lab.max(axis=1) > c.node_labels.max(axis=1)).all()
        e.update_node_labels(idx, rows)
        assert np.array_equal(eval_into_view(e, sel, T, n, p, W, 0), seltag_ref.seltag_mask(lab, sel)), "after a relabel past the planned maxima"
        # another key count: eleven keys (two passes) over other nodes
        k = case(1025, 9)
        lab2 = np.concatenate([k["lab"], k["lab"][:2][:, ::-1]])
        sel2 = np.concatenate([k["sel"], k["sel"][:2]])
        e.set_nodes(np.zeros(1025, np.int64), np.zeros(1025, np.int64), lab2)
        assert e.n_keys == 11
        want = seltag_ref.seltag_mask(lab2, sel2)
        got = eval_into_view(e, sel2, T, 1025, P_MAX, 17, 0)
        assert np.array_equal(got, want) and not np.array_equal(want, k["want"]), "after ksched_set_nodes with eleven keys"
    finally:
        e.close()


def test_two_streams_around_a_label_update(ev):
    selector_calls.two_streams_around_a_label_update(ev, CALL, *snapshot_case(0xE97))


# ---- 6. refusals and edge sizes -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_mask_and_bindings_untouched(ev):
    import torch
    c = synth.make_cluster(40, 130, n_keys=4, n_taints=4, seed=0xE9E44)
    ev.set_nodes(c.avail_cpu, c.avail_mem, c.node_labels, c.node_taints)
    P, W = c.P, ev.W
    lib, h = _lib.load(), ev._h
    cpu, mem, sel, tol = pod_tensors(ev, c)
    smp = to_dev(ev, c.samples, np.int32)
    dM, dF = (torch.full((P, W), 0x5A5A5A5A, dtype=torch.int64, device=dev_of(ev)) for _ in range(2))
    dB = fresh(ev, P)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ops = [SELOP_EXISTS, SELOP_GT, SELOP_LT]
    f = T
    st = C.c_void_p(torch.cuda.current_stream(ev.device).cuda_stream)

    def device(flags, feas, fit, bind, attempts=0, samples=None, p=P):
        return lib.ksched_eval_device_pitched(h, p, vp(cpu), vp(mem), vp(sel), vp(tol), vp(samples), attempts, flags, vp(feas), vp(fit), vp(bind), W, st)
    # the accepting entry points
    for op in ops:
        assert device(f | op, dM, None, None) == _lib.E_INVAL, "the operator is the entry's or the call's, not both"
    assert device(f | SELOP_GT | SELOP_LT, dM, None, None) == _lib.E_INVAL
    assert device(SELOP_TAGGED, dM, None, None) == _lib.E_INVAL, "the flag needs KSCHED_SEL"
    assert device(SELOP_TAGGED | PICK_UNIFORM, dM, None, dB, 5, smp) == _lib.E_INVAL
    assert device(f | FIT, dM, None, None) == _lib.E_INVAL
    assert device(f | TAINT, dM, None, None) == _lib.E_INVAL
    assert device(f | FIT | TAINT | PICK_BESTFIT, dM, None, dB) == _lib.E_INVAL
    assert device(f | WANT_FIT_MASK, dM, dF, None) == _lib.E_INVAL
    assert device(f | WANT_FIT_MASK, dM, None, None) == _lib.E_INVAL
    assert device(f, dM, dF, None) == _lib.E_INVAL
    assert device(f | COMBINE_AND | FIT, dM, None, None) == _lib.E_INVAL
    # every refusal of a plain or a combining call stays
    assert device(f, None, None, None) == _lib.E_INVAL, "nothing to write"
    assert device(f | COMBINE_AND, None, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_AND | PICK_UNIFORM, None, None, dB, 5, smp) == _lib.E_INVAL, "a pick does not stand in for the combine's mask"
    assert device(f | COMBINE_AND | COMBINE_OR, dM, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_SOFT, dM, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_OR | COMBINE_SOFT, dM, None, None) == _lib.E_INVAL
    assert device(f | PICK_UNIFORM | PICK_SPREAD, dM, None, dB, 5, smp) == _lib.E_INVAL
    assert device(f | PICK_UNIFORM, dM, None, None, 5, smp) == _lib.E_INVAL, "a pick needs out_binding"
    assert device(f | PICK_UNIFORM, dM, None, dB, 0, smp) == _lib.E_INVAL
    assert device(f | 0x1000, dM, None, None) == _lib.E_INVAL, "0x1000 stays unknown"
    assert device(f | 0x20000, dM, None, None) == _lib.E_INVAL, "0x20000 stays unknown"
    assert device(SEL | 0x20000, dM, None, None) == _lib.E_INVAL and device(SEL | 0x80000, dM, None, None) == _lib.E_INVAL
    assert lib.ksched_eval_device(h, P, None, vp(mem), vp(sel), None, None, 0, f, vp(dM), None, None, st) == _lib.E_INVAL, "the requests stay required"
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, f | SELOP_GT, vp(dM), None, None, st) == _lib.E_INVAL
    hM, hB = np.full((P, W), SENTINEL, np.uint64), np.full(P, -7, np.int32)
    hsel = np.ascontiguousarray(c.pod_sel)
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, f | SELOP_EXISTS, hp(hM), None, None) == _lib.E_INVAL
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, SELOP_TAGGED, hp(hM), None, None) == _lib.E_INVAL
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, f | FIT, hp(hM), None, None) == _lib.E_INVAL
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, f | COMBINE_AND, hp(hM), None, None) == _lib.E_INVAL, "the host form combines nothing"
    dev_b, stream = C.c_void_p(), C.c_void_p()
    for bad in (f | SELOP_LT, SELOP_TAGGED, f | TAINT, f | COMBINE_ANDNOT):
        assert lib.ksched_eval_begin(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), P, None, None, 0, bad, hp(hM), None, P, C.byref(dev_b), C.byref(stream)) == _lib.E_INVAL
        assert not dev_b.value
    # the entry points that do not take the flag
    table = torch.full((P, _lib.SUMMARY_WORDS), -7, dtype=torch.int32, device=dev_of(ev))
    htable = np.full((P, _lib.SUMMARY_WORDS), 7, np.uint32)
    pairs = np.zeros(1, np.uint32)
    reason = np.full(1, -7, np.int32)
    pipe = ev.pipe(2)
    try:
        assert lib.ksched_pipe_submit(pipe._h, 0, P, vp(cpu), vp(mem), vp(sel), None, vp(smp), 5, f | PICK_UNIFORM, vp(dM), W, vp(dB)) == _lib.E_INVAL
        assert lib.ksched_pipe_submit(pipe._h, 0, P, vp(cpu), vp(mem), vp(sel), None, vp(smp), 5, f | PICK_SAMPLED, vp(dM), W, vp(dB)) == _lib.E_INVAL
        assert pipe.slot_stream_handle(0) == 0, "nothing was enqueued on the slot"
    finally:
        pipe.close()
    for flags in (PICK_UNIFORM | SELOP_TAGGED, PICK_UNIFORM | f):
        assert lib.ksched_pick(h, P, hp(hM), None, hp(c.samples), 5, flags, hp(hB)) == _lib.E_INVAL
        assert lib.ksched_pick_device(h, P, vp(dM), W, None, vp(smp), 5, flags, vp(dB), st) == _lib.E_INVAL
    assert lib.ksched_summarize_device(h, P, vp(cpu), vp(mem), vp(sel), None, f, vp(table), st) == _lib.E_INVAL
    assert lib.ksched_summarize(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, f, hp(htable)) == _lib.E_INVAL
    assert lib.ksched_explain(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, 1, hp(pairs), hp(pairs), f, hp(reason)) == _lib.E_INVAL
    # the Python face: ValueError before the library
    for call in (lambda: ev.eval_device(cpu, mem, sel, None, None, f | FIT, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, f | SELOP_GT, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, SELOP_TAGGED, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, f, out_feasible=dM, out_fit=dF),
                 lambda: ev.pick_device(dM, PICK_UNIFORM | SELOP_TAGGED, dB, samples=smp),
                 lambda: ev.pick(hM, PICK_UNIFORM | SELOP_TAGGED, samples=c.samples),
                 lambda: ev.summarize_device(cpu, mem, sel, None, f, out=table),
                 lambda: ev.summarize(c.req_cpu, c.req_mem, hsel, None, f),
                 lambda: ev.explain(c.req_cpu, c.req_mem, hsel, None, [0], [1], f),
                 lambda: ev.eval(c.req_cpu, c.req_mem, hsel, None, None, f | TAINT)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert (dM == 0x5A5A5A5A).all() and (dF == 0x5A5A5A5A).all() and (dB == -7).all() and (table == -7).all()
    assert (hM == SENTINEL).all() and (hB == -7).all() and (htable == 7).all() and (reason == -7).all()
    # p == 0: a no-op; and a plain call still works
    assert device(f | PICK_UNIFORM, dM, None, dB, 5, smp, p=0) == _lib.OK
    torch.cuda.synchronize()
    assert (dM == 0x5A5A5A5A).all() and (dB == -7).all()
    ev.eval_device(cpu, mem, sel, tol, None, FIT | SEL | TAINT, out_feasible=dM)
    ev.eval_device(cpu, mem, sel, None, None, f, out_feasible=dF)
    torch.cuda.synchronize()
    assert np.array_equal(mask_np(dM), oracle_mask(c, FIT | SEL | TAINT))
    assert np.array_equal(mask_np(dF), seltag_ref.seltag_mask(c.node_labels, hsel))


def test_edge_sizes(built):
    selector_calls.edge_sizes(CALL)
