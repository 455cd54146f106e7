"""KSCHED_SELOP_EXISTS / _GT / _LT (extension E8) on the GPU, bit for bit against tests/selop_ref.py (pinned by tests/test_selop_restatement.py),
with tests/combine_ref.py / tests/soft_ref.py and ksched_pick_device on top of it.
 1. mask parity of every operator at the word, wave and block edges of the kernel's mapping (n), the tile edges of its pod walk (p) and each
    side of its key passes (keys), into packed rows, rows at ksched_mask_pitch(n) and views that start one word into their buffer; the ids
    sit on both sides of the sign bit; what the cases contain is asserted on the EXPECTED values before the device is asked;
 2. the same bits on an indexed and on an unindexed snapshot, with KSCHED_OPT_KERNEL forced to each value; ksched_last_kernel "selop";
 3. every operator under AND, OR, AND-NOT and the soft modifier into a caller's mask with garbage beyond n, and the header's recipe;
 4. each of the five picks in an operator call, plain and combining == ksched_pick_device on the resulting mask with the pick flag alone;
 5. the host forms ksched_eval and ksched_eval_begin / _end give the device form's bits;
 6. label updates within the planned maxima and past them, another key count, and two streams around a label update;
 7. the refusals at every entry point, outputs untouched, and the edge sizes p == 0, n == 0, no snapshot.
Every output goes into sentinel-filled buffers.  Shapes are the smallest at which the kernel takes each path.  What the three selector
files share -- the guarded evaluation, the bodies that are the same for every call -- is tests/selector_calls.py's."""
import ctypes as C

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (COMBINE_AND, COMBINE_ANDNOT, COMBINE_OR, COMBINE_SOFT, FIT, PICK_BESTFIT, PICK_SAMPLED, PICK_SPREAD, PICK_UNIFORM,
                                             SEL, SEL_NEVER, SELOP_EXISTS, SELOP_GT, SELOP_LT, TAINT, WANT_FIT_MASK, Evaluator, _lib, pack_mask, synth)
from tests import combine_ref, selector_calls, selop_ref
from tests.pick_helpers import dev_of, fresh, mask_np, pod_tensors, to_dev
from tests.selector_calls import (COMBINES, CORES_KEY, GPU_KEY, PICKS, SENTINEL, ZONE_3, ZONE_KEY, SelectorCall, as_signed, ev, eval_into_view, indexed_cluster,  # noqa: F401 (ev: the fixture)
                                  recipe_cluster, row_kinds)

pytestmark = pytest.mark.gpu

OPS = [SELOP_EXISTS, SELOP_GT, SELOP_LT]
OP_IDS = ["exists", "gt", "lt"]
IDS = np.array([0, 1, 2, 3, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)  # what a node carries: 0 = not the key
CALLS = {op: SelectorCall(SEL | op, "selop", lambda lab, sel, p=None, op=op: selop_ref.selop_mask(lab, sel, op, p=p)) for op in OPS}


def test_the_flags_are_the_restatements():
    assert (SELOP_EXISTS, SELOP_GT, SELOP_LT) == (selop_ref.EXISTS, selop_ref.GT, selop_ref.LT) and SEL_NEVER == selop_ref.NEVER


# ---- 1. mask parity -----------------------------------------------------------------------------------------------------------------------
NODES = [1, 63, 64, 65, 1023, 1024, 1025, 4097]  # a word, a wave's four words and a block's sixteen, each side; several blocks
PODS = [1, 63, 64, 65, 129]                      # a tile of 64 pods, each side; more than two tiles
KEYS = [1, 8, 9, 32]                             # one pass of eight keys, each side; KSCHED_MAX_KEYS
P_MAX = max(PODS)
_CASES = {}


def variant_bits(labels, entries, rule):
    """the mask bits under ANOTHER rule for a constrained (entry, id) pair -- rule(e [p, 1], v [1, n]) -> [p, n] bool --, 0 and NEVER as in
    the contract: what a wrong kernel would compute, to show that the cases tell it from the right one"""
    labels, entries = labels.astype(np.uint64), entries.astype(np.uint64)
    ok = np.ones((entries.shape[1], labels.shape[1]), dtype=bool)
    for k in range(labels.shape[0]):
        pods = np.nonzero(entries[k])[0]
        if pods.size:
            e = entries[k][pods][:, None]
            ok[pods] &= np.where(e == SEL_NEVER, False, rule(e, labels[k][None, :]))
    return ok


def case(n, keys):
    """labels [keys][n] drawn from IDS; entries [keys][P_MAX] by pod kind ((pod + 1) % 8): 0 nothing constrained; 1 one key, any id; 2 NEVER
    on one key beside another; 3 two keys; 4 two keys, the second one beyond the first pass where there is one; 5 three keys; 6 one key at
    the sign bit; 7 one key with the largest bound.  Per operator the expected mask; computed once, read-only."""
    if (n, keys) not in _CASES:
        rng = np.random.default_rng([0xE8, n, keys])
        lab = IDS[rng.integers(0, IDS.size, size=(keys, n))]
        sel = np.zeros((keys, P_MAX), dtype=np.uint32)
        two = []  # (pod, key a, key b) of the pods that constrain exactly two keys
        for pod in range(P_MAX):
            kind = (pod + 1) % 8
            ks = rng.permutation(keys)
            if kind == 1:
                sel[ks[0], pod] = IDS[rng.integers(1, IDS.size)]
            elif kind == 2:
                sel[ks[0], pod] = SEL_NEVER
                if keys > 1:
                    sel[ks[1], pod] = IDS[rng.integers(1, 4)]
            elif kind in (3, 4) and keys > 1:
                a, b = int(ks[0]), int(ks[1])
                if kind == 4 and keys > 8:
                    a, b = int(rng.integers(0, 8)), int(rng.integers(8, keys))
                sel[a, pod], sel[b, pod] = IDS[rng.integers(1, 5)], IDS[rng.integers(2, 6)]
                two.append((pod, a, b))
            elif kind in (3, 4):
                sel[0, pod] = IDS[rng.integers(1, 5)]
            elif kind == 5:
                for k in ks[:3]:
                    sel[k, pod] = IDS[rng.integers(1, IDS.size)]
            elif kind == 6:
                sel[ks[0], pod] = IDS[rng.integers(4, 6)]
            elif kind == 7:
                sel[ks[0], pod] = 0xFFFFFFFE
        want = {op: selop_ref.selop_mask(lab, sel, op) for op in OPS}
        for a in (lab, sel, *want.values()):
            a.setflags(write=False)
        _CASES[(n, keys)] = dict(lab=lab, sel=sel, want=want, two=two)
    return _CASES[(n, keys)]


_FACTS = {}


def matrix_facts():
    """What the matrix contains, per operator, from the expected values alone -- asserted before any device call, so that no case can pass
    vacuously: an all-valid row; an empty row; rows that are neither in at least a quarter of the multi-node cases; for GT and LT a pair
    whose answer a signed compare would flip; for LT a pair that only the `v != 0` term rejects; a pod with two constrained keys whose row
    differs from each key's alone."""
    if _FACTS:
        return _FACTS
    for op in OPS:
        full = empty = mixed_cases = multi = flips = presence = both_differ = 0
        for n in NODES:
            for keys in KEYS:
                k = case(n, keys)
                want = k["want"][op]
                f, e, m = row_kinds(want, n)
                full, empty = full + f, empty + e
                multi += n > 1
                mixed_cases += n > 1 and m > 0
                if op != SELOP_EXISTS:
                    cmp = np.greater if op == SELOP_GT else np.less
                    signed = variant_bits(k["lab"], k["sel"], lambda e_, v_, cmp=cmp: (v_ != 0) & cmp(as_signed(v_), as_signed(e_)))
                    flips += int((selop_ref.pack(signed) != want).any())
                if op == SELOP_LT:
                    bare = variant_bits(k["lab"], k["sel"], lambda e_, v_: v_ < e_)
                    presence += int((selop_ref.pack(bare) != want).any())
                for pod, a, b in k["two"]:
                    alone = []
                    for key in (a, b):
                        s = np.zeros((keys, 1), dtype=np.uint32)
                        s[key, 0] = k["sel"][key, pod]
                        alone.append(selop_ref.selop_mask(k["lab"], s, op)[0])
                    both_differ += int((want[pod] != alone[0]).any() and (want[pod] != alone[1]).any())
        _FACTS[op] = dict(full=full, empty=empty, mixed_cases=mixed_cases, multi=multi, flips=flips, presence=presence, both_differ=both_differ)
    return _FACTS


def check_matrix_facts():
    for op, f in matrix_facts().items():
        name = selop_ref.NAMES[op]
        assert f["full"] >= 1 and f["empty"] >= 1, f"{name}: {f}"
        assert 4 * f["mixed_cases"] >= f["multi"] > 0, f"{name}: {f}"
        assert op == SELOP_EXISTS or f["flips"] >= 1, f"{name}: no pair a signed compare would flip"
        assert op != SELOP_LT or f["presence"] >= 1, f"{name}: no pair that only the presence test rejects"
        assert f["both_differ"] >= 1, f"{name}: no pod whose two keys together differ from each alone"


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("n", NODES)
def test_mask_parity(ev, n, keys):
    check_matrix_facts()
    k = case(n, keys)
    W = (n + 63) // 64
    valid_last = combine_ref.valid_bits_word(n)
    for op in OPS:
        assert k["want"][op].shape == (P_MAX, W) and not (k["want"][op][:, -1] & ~np.uint64(valid_last)).any()
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    assert ev.W == W
    std = int(_lib.load().ksched_mask_pitch(n))
    assert std % 16 == 0 and std >= W
    for p in PODS:
        for pitch, offset in ((W, 0), (std, 0), (W, 1), (std, 1)):
            for op, name in zip(OPS, OP_IDS):
                got = eval_into_view(ev, k["sel"], SEL | op, n, p, pitch, offset)
                want = k["want"][op][:p]
                assert np.array_equal(got, want), f"{name}, p = {p}, pitch {pitch}, offset {offset}: pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from selop_ref"
                assert ev.last_kernel == "selop" and ev.last_pick == "none"


def test_a_block_that_walks_more_than_one_pod_tile(ev):
    """1024 column blocks leave two block rows for three pod tiles: the first block row walks two tiles, the second one (whose second slot
    lies past p: the `first >= p` break) -- the smallest shape at which k_eval_selop's tile loop takes a second turn.  Every pod's entries
    are its own, so a block that computed its first tile again, or stored a tile's rows a tile too low, gives rows that differ"""
    n, keys, p = 16 * 64 * 1024 - 37, 2, 130
    W = (n + 63) // 64
    gx = (W + 15) // 16
    want_rows = (2048 + gx - 1) // gx
    tiles = (p + 63) // 64
    assert gx == 1024 and want_rows == 2 < tiles == 3, "pod_tiles_per_block == 2"
    rng = np.random.default_rng([0xE8, n, keys, p])
    lab = IDS[rng.integers(0, IDS.size, size=(keys, n))]
    lab[:, rng.random(n) < 0.5] = 0  # (so that EXISTS rows are neither full nor empty too)
    lab[1] = np.where(rng.random(n) < 0.7, lab[1], IDS[rng.integers(0, IDS.size, size=n)])
    sel = np.zeros((keys, p), dtype=np.uint32)
    for pod in range(p):  # kind by pod: key 0, key 1, both, and now and then NEVER or nothing -- with a period of 7, so no tile repeats another
        kind = pod % 7
        if kind in (0, 2, 4, 5):
            sel[0, pod] = IDS[rng.integers(1, IDS.size)]
        if kind in (1, 2, 5, 6):
            sel[1, pod] = IDS[rng.integers(1, IDS.size)]
        if kind == 6 and pod % 3 == 0:
            sel[0, pod] = SEL_NEVER
    sel[:, 3] = 0
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), lab)
    assert ev.W == W
    pitch = W + 3
    for op, name in zip(OPS, OP_IDS):
        want = selop_ref.selop_mask(lab, sel, op)
        assert want.shape == (p, W) and not (want[:, -1] & ~np.uint64(combine_ref.valid_bits_word(n))).any()
        assert row_kinds(want, n)[2] >= p // 4, f"{name}: rows that are neither full nor empty"
        # what a block that walked tile 0 twice would leave in the rows of tile 1, and one that skipped to tile 2 in those of tile 1
        assert (want[64:128] != want[0:64]).any(axis=1).sum() >= 32 and (want[64:66] != want[128:130]).any(), f"{name}: the tiles' rows differ"
        got = eval_into_view(ev, sel, SEL | op, n, p, pitch, 1)
        assert np.array_equal(got, want), f"{name}: pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from selop_ref"
        assert ev.last_kernel == "selop" and ev.last_pick == "none"


def test_no_selectors_and_no_keys_pass_every_node(ev):
    selector_calls.no_selectors_and_no_keys_pass_every_node(ev, list(CALLS.values()), list(CALLS.values()), 0xE80, IDS)


# ---- 2. both kinds of snapshot --------------------------------------------------------------------------------------------------------------
def unindexed_cluster():
    """three high-cardinality keys: no bitmap index (tests/test_gpu_summary.py's builder)"""
    rng = np.random.default_rng(0xE8002)
    N, P = 700, 129
    lab = rng.integers(1, 4_000_000, size=(3, N)).astype(np.uint32)
    lab[:, ::7] = 0
    sel = np.zeros((3, P), dtype=np.uint32)
    sel[0, ::3] = lab[0, rng.integers(0, N, size=len(sel[0, ::3]))] + 1
    sel[2, ::4] = rng.integers(1, 4_000_000, size=len(sel[2, ::4]))
    sel[1, 5::16] = SEL_NEVER
    return rng.integers(0, 1000, N).astype(np.int64), rng.integers(0, 1000, N).astype(np.int64), lab, sel


@pytest.mark.parametrize("kind", ["indexed", "unindexed"])
def test_the_same_bits_on_both_kinds_of_snapshot_under_every_kernel_option(ev, kind):
    cpu, mem, lab, sel = indexed_cluster() if kind == "indexed" else unindexed_cluster()
    n, p = lab.shape[1], sel.shape[1]
    want = {op: selop_ref.selop_mask(lab, sel, op) for op in OPS}
    for op in OPS:
        assert row_kinds(want[op], n)[2] > p // 8, "most constrained rows are neither full nor empty"
    ev.set_nodes(cpu, mem, lab)
    assert (ev.index_checksum() != (0, 0)) == (kind == "indexed")
    for kernel in ("auto", "direct", "fused"):
        ev.set_kernel(kernel)  # (no effect on an operator call: the fused kernel forced on an unindexed snapshot is no refusal here)
        for op in OPS:
            got = eval_into_view(ev, sel, SEL | op, n, p, (n + 63) // 64, 0)
            assert np.array_equal(got, want[op]), f"{kind}, {kernel}, {selop_ref.NAMES[op]}"
            assert ev.last_kernel == "selop"
    ev.set_kernel("auto")
    plain = eval_into_view(ev, sel, SEL, n, p, (n + 63) // 64, 0)
    assert ev.last_kernel in ("direct", "fused") and not np.array_equal(plain, want[SELOP_EXISTS])


def test_timing_brackets_the_operator_kernel(ev):
    cpu, mem, lab, sel = indexed_cluster()
    ev.set_nodes(cpu, mem, lab)
    p = sel.shape[1]
    ev.set_timing(True)
    try:
        ev.kernel_time_ms()  # (reading the samples resets them)
        eval_into_view(ev, sel, SEL | SELOP_GT, lab.shape[1], p, ev.W, 0)
        ms, count = ev.kernel_time_ms()
        assert count == 1 and ms > 0, "one pair of stream events around the operator kernel"
    finally:
        ev.set_timing(False)


# ---- 3. combining ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comb,comb_id", COMBINES, ids=[c[1] for c in COMBINES])
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_every_operator_under_every_combine(ev, op, comb, comb_id):
    k = case(1025, 9)
    selector_calls.the_call_under_every_combine(ev, CALLS[op], k["lab"], k["sel"], k["want"][op], comb, np.random.default_rng([0xE83, op, comb]))


@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
def test_the_recipe_end_to_end(ev, pitched):
    """gpu Exists AND cores Gt 16 AND zone NotIn {z3} AND fit, then the spread pick: four calls on one mask, against the label columns"""
    import torch
    c, lab = recipe_cluster(0xE8C4)
    P, N = c.P, c.N
    fits = (c.req_cpu[:, None] <= c.avail_cpu[None, :]) & (c.req_mem[:, None] <= c.avail_mem[None, :])
    gpu, cores, zone = lab[GPU_KEY], lab[CORES_KEY].astype(np.int64) - 1, lab[ZONE_KEY]
    ok_nodes = (gpu != 0) & (lab[CORES_KEY] != 0) & (cores > 16) & (zone != ZONE_3)
    bits = fits & ok_nodes[None, :]
    assert 0 < ok_nodes.sum() < N and ((lab[CORES_KEY] == 0) & (gpu != 0) & (zone != ZONE_3)).any() and ((cores == 16) & (gpu != 0)).any()
    assert P // 4 < bits.any(axis=1).sum() < P, "pods with a node and pods without one"
    want = pack_mask(bits)
    ev.set_nodes(c.avail_cpu, c.avail_mem, lab)
    cpu, mem = to_dev(ev, c.req_cpu, np.int64), to_dev(ev, c.req_mem, np.int64)

    def sel_of(key, value):
        s = np.zeros((c.n_keys, P), dtype=np.uint32)
        s[key] = value
        return to_dev(ev, s, np.int32)
    draws = np.random.default_rng(0xE8C5).integers(0, 1 << 32, size=(P, 3), dtype=np.uint64).astype(np.uint32)
    smp = to_dev(ev, draws, np.int32)
    M = ev.alloc_mask(P, pitched=pitched)
    M.fill_(-1)  # whatever the mask held before the chain
    out = fresh(ev, P, 4)
    ev.eval_device(cpu, mem, sel_of(GPU_KEY, 1), None, None, SEL | SELOP_EXISTS, out_feasible=M)
    ev.eval_device(cpu, mem, sel_of(CORES_KEY, 16 + 1), None, None, SEL | SELOP_GT | COMBINE_AND, out_feasible=M)
    ev.eval_device(cpu, mem, sel_of(ZONE_KEY, ZONE_3), None, None, SEL | COMBINE_ANDNOT, out_feasible=M)
    ev.eval_device(cpu, mem, None, None, smp, FIT | COMBINE_AND | PICK_SPREAD, out_feasible=M, out_binding=out[:P])
    alone = fresh(ev, P)
    ev.pick_device(to_dev(ev, want, np.int64), PICK_SPREAD, alone, samples=smp)
    torch.cuda.synchronize()
    got = mask_np(M)
    assert np.array_equal(got, want), f"pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from the label columns' answer"
    b = out.cpu().numpy()
    assert np.array_equal(b[:P], alone.cpu().numpy()) and (b[P:] == -7).all()
    assert ((b[:P] >= 0) == bits.any(axis=1)).all() and bits[np.nonzero(b[:P] >= 0)[0], b[:P][b[:P] >= 0]].all()
    # DoesNotExist: EXISTS under AND-NOT; a preferred expression adds the modifier
    ev.eval_device(cpu, mem, None, None, None, FIT, out_feasible=M)
    ev.eval_device(cpu, mem, sel_of(GPU_KEY, 1), None, None, SEL | SELOP_EXISTS | COMBINE_ANDNOT, out_feasible=M)
    torch.cuda.synchronize()
    assert np.array_equal(mask_np(M), pack_mask(fits & (gpu == 0)[None, :]))


# ---- 4. picks -----------------------------------------------------------------------------------------------------------------------------------
_PICK_CASE = {}


def pick_case():
    if not _PICK_CASE:
        P, N = 300, 700
        c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=0xE8B1C)
        rng = np.random.default_rng(0xE8B1)
        sel = np.ascontiguousarray(c.pod_sel).copy()
        sel[3, 1::9] = SEL_NEVER  # pods without a node
        old = pack_mask(rng.random((P, N)) < 0.4)
        draws = rng.integers(0, 1 << 32, size=(P, 5), dtype=np.uint64).astype(np.uint32)
        new = {op: selop_ref.selop_mask(c.node_labels, sel, op) for op in OPS}
        for a in (sel, old, draws, *new.values()):
            a.setflags(write=False)
        _PICK_CASE.update(c=c, sel=sel, old=old, draws=draws, new=new)
    return _PICK_CASE


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("pick,last_pick", PICKS, ids=["sampled", "bestfit", "uniform", "spread", "pack"])
def test_a_pick_in_an_operator_call_is_the_pick_from_the_resulting_mask(ev, pick, last_pick, op):
    selector_calls.a_pick_in_the_call_is_the_pick_from_the_resulting_mask(ev, CALLS[op], pick_case(), pick_case()["new"][op], pick, last_pick)


# ---- 5. the host forms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_the_host_forms_give_the_device_forms_bits(ev, op):
    selector_calls.the_host_forms_give_the_device_forms_bits(ev, CALLS[op], pick_case(), pick_case()["new"][op])


# ---- 6. snapshot changes ------------------------------------------------------------------------------------------------------------------------
def all_ops(ev, sel, n, p):
    return {op: eval_into_view(ev, sel, SEL | op, n, p, (n + 63) // 64, 0) for op in OPS}


def test_label_updates_another_key_count_and_a_fresh_evaluator(built):
    c = synth.make_cluster(129, 1100, n_keys=8, n_taints=0, seed=0xE86)
    lab = c.node_labels.copy()
    sel = np.ascontiguousarray(c.pod_sel)
    n, p = c.N, c.P
    rng = np.random.default_rng(0xE86)
    e = Evaluator(0)
    try:
        e.set_nodes(c.avail_cpu, c.avail_mem, lab)
        for op, got in all_ops(e, sel, n, p).items():
            assert np.array_equal(got, selop_ref.selop_mask(lab, sel, op))
        # within the planned maxima: ids the keys already have, and nodes that lose a key
        idx = rng.choice(n, size=200, replace=False).astype(np.uint32)
        rows = rng.integers(0, lab.max(axis=1)[:, None] + 1, size=(8, idx.size)).astype(np.uint32)
        before = {op: selop_ref.selop_mask(lab, sel, op) for op in OPS}
        lab[:, idx] = rows
        assert all(not np.array_equal(before[op], selop_ref.selop_mask(lab, sel, op)) for op in OPS), "the update shows in every operator's mask"
        e.update_node_labels(idx, rows)
        for op, got in all_ops(e, sel, n, p).items():
            assert np.array_equal(got, selop_ref.selop_mask(lab, sel, op)), f"{selop_ref.NAMES[op]} after an update within the planned maxima"
        # past them: ids above every planned maximum (the layout is planned again)
        idx = rng.choice(n, size=300, replace=False).astype(np.uint32)
        rows = rng.integers(0, 5000, size=(8, idx.size)).astype(np.uint32)
        lab[:, idx] = rows
        assert (lab.max(axis=1) > c.node_labels.max(axis=1)).all()
        e.update_node_labels(idx, rows)
        for op, got in all_ops(e, sel, n, p).items():
            assert np.array_equal(got, selop_ref.selop_mask(lab, sel, op)), f"{selop_ref.NAMES[op]} after a relabel past the planned maxima"
        # another key count: eleven keys (two passes) over other nodes
        k = case(1025, 9)
        lab2 = np.concatenate([k["lab"], k["lab"][:2][:, ::-1]])
        sel2 = np.concatenate([k["sel"], k["sel"][:2]])
        e.set_nodes(np.zeros(1025, np.int64), np.zeros(1025, np.int64), lab2)
        assert e.n_keys == 11
        for op, got in all_ops(e, sel2, 1025, P_MAX).items():
            want = selop_ref.selop_mask(lab2, sel2, op)
            assert np.array_equal(got, want) and not np.array_equal(want, k["want"][op]), f"{selop_ref.NAMES[op]} after ksched_set_nodes with eleven keys"
    finally:
        e.close()


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_two_streams_around_a_label_update(ev, op):
    c = synth.make_cluster(129, 1100, n_keys=8, n_taints=0, seed=0xE87)
    selector_calls.two_streams_around_a_label_update(ev, CALLS[op], c, np.ascontiguousarray(c.pod_sel), np.random.default_rng([0xE87, op]))


# ---- 7. refusals and edge sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_refusals_leave_mask_and_bindings_untouched(ev, op):
    import torch
    c = synth.make_cluster(40, 130, n_keys=4, n_taints=4, seed=0xE8E44)
    ev.set_nodes(c.avail_cpu, c.avail_mem, c.node_labels, c.node_taints)
    P, W = c.P, ev.W
    lib, h = _lib.load(), ev._h
    cpu, mem, sel, tol = pod_tensors(ev, c)
    smp = to_dev(ev, c.samples, np.int32)
    dM, dF = (torch.full((P, W), 0x5A5A5A5A, dtype=torch.int64, device=dev_of(ev)) for _ in range(2))
    dB = fresh(ev, P)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    others = [o for o in OPS if o != op]
    f = SEL | op
    st = C.c_void_p(torch.cuda.current_stream(ev.device).cuda_stream)

    def device(flags, feas, fit, bind, attempts=0, samples=None, p=P):
        return lib.ksched_eval_device_pitched(h, p, vp(cpu), vp(mem), vp(sel), vp(tol), vp(samples), attempts, flags, vp(feas), vp(fit), vp(bind), W, st)
    # the accepting entry points
    for other in others:
        assert device(f | other, dM, None, None) == _lib.E_INVAL, "two operators"
    assert device(f | others[0] | others[1], dM, None, None) == _lib.E_INVAL
    assert device(op, dM, None, None) == _lib.E_INVAL, "an operator needs KSCHED_SEL"
    assert device(op | PICK_UNIFORM, dM, None, dB, 5, smp) == _lib.E_INVAL
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
    assert device(f | 0x20000, dM, None, None) == _lib.E_INVAL
    assert lib.ksched_eval_device(h, P, None, vp(mem), vp(sel), None, None, 0, f, vp(dM), None, None, st) == _lib.E_INVAL, "the requests stay required"
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, f | others[0], vp(dM), None, None, st) == _lib.E_INVAL
    hM, hB = np.full((P, W), SENTINEL, np.uint64), np.full(P, -7, np.int32)
    hsel = np.ascontiguousarray(c.pod_sel)
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, f | others[0], hp(hM), None, None) == _lib.E_INVAL
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, op, hp(hM), None, None) == _lib.E_INVAL
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, f | FIT, hp(hM), None, None) == _lib.E_INVAL
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, f | COMBINE_AND, hp(hM), None, None) == _lib.E_INVAL, "the host form combines nothing"
    dev_b, stream = C.c_void_p(), C.c_void_p()
    for bad in (f | others[0], op, f | TAINT, f | COMBINE_ANDNOT):
        assert lib.ksched_eval_begin(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), P, None, None, 0, bad, hp(hM), None, P, C.byref(dev_b), C.byref(stream)) == _lib.E_INVAL
        assert not dev_b.value
    # the entry points that take no operator flag
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
    for flags in (PICK_UNIFORM | op, PICK_UNIFORM | f):
        assert lib.ksched_pick(h, P, hp(hM), None, hp(c.samples), 5, flags, hp(hB)) == _lib.E_INVAL
        assert lib.ksched_pick_device(h, P, vp(dM), W, None, vp(smp), 5, flags, vp(dB), st) == _lib.E_INVAL
    assert lib.ksched_summarize_device(h, P, vp(cpu), vp(mem), vp(sel), None, f, vp(table), st) == _lib.E_INVAL
    assert lib.ksched_summarize(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, f, hp(htable)) == _lib.E_INVAL
    assert lib.ksched_explain(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, 1, hp(pairs), hp(pairs), f, hp(reason)) == _lib.E_INVAL
    # the Python face: ValueError before the library
    for call in (lambda: ev.eval_device(cpu, mem, sel, None, None, f | FIT, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, f | others[0], out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, op, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, f, out_feasible=dM, out_fit=dF),
                 lambda: ev.pick_device(dM, PICK_UNIFORM | op, dB, samples=smp),
                 lambda: ev.summarize_device(cpu, mem, sel, None, f, out=table),
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
    from tests.pick_helpers import oracle_mask
    assert np.array_equal(mask_np(dM), oracle_mask(c, FIT | SEL | TAINT))
    assert np.array_equal(mask_np(dF), selop_ref.selop_mask(c.node_labels, hsel, op))


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_edge_sizes(built, op):
    selector_calls.edge_sizes(CALLS[op])
