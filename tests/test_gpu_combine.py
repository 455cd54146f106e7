"""KSCHED_COMBINE_AND / _OR / _ANDNOT (extension E6) on the GPU, bit for bit: feasible(this call) is the oracle's mask of the same request,
the expected mask is tests/combine_ref.py (pinned by tests/test_combine_restatement.py) of the old mask and that one.
 1. every op at the knife edges of k_mask_combine: rows of one word, the valid-bits edge, odd and even W, packed and pitched rows, an
    unaligned base, more than one block and more than one grid pass; garbage in the old mask at and beyond n, sentinels in the padding
    words and in two guard rows;
 2. the recipe of include/ksched.h as a chain of four calls, against a restatement written from the label columns;
 3. a pick in a combining call == ksched_pick_device on the combined mask with the pick flag alone, for all five picks and three ops,
    and the reduced best-fit case that tells the two apart;
 4. the refusals: KSCHED_E_INVAL (KSCHED_E_UNSUPPORTED for a forced fused kernel without an index) with mask and bindings untouched;
 5. a combining call and a scratch-mask pick on two streams, alternately.
Shapes are the smallest at which the kernel takes each path; the launch geometry is read from csrc/mask_combine.hpp."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (COMBINE_AND, COMBINE_ANDNOT, COMBINE_OR, FIT, PICK_BESTFIT, PICK_PACK, PICK_SAMPLED, PICK_SPREAD,
                                             PICK_UNIFORM, SEL, TAINT, WANT_FIT_MASK, _lib, pack_mask, synth)
from tests import combine_ref
from tests.pick_helpers import dev_of, fresh, mask_np, oracle_mask, pod_tensors, to_dev
from tests.spread_ref import spread_pick

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = [COMBINE_AND, COMBINE_OR, COMBINE_ANDNOT]
OP_IDS = ["and", "or", "andnot"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD_ROWS = 2


def plan_constants():
    """kCombineBlock and kCombineMaxGrid as csrc/mask_combine.hpp states them"""
    text = open(os.path.join(ROOT, "kube_scheduler_rs_reference_amd", "csrc", "mask_combine.hpp")).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1)) for name in ("kCombineBlock", "kCombineMaxGrid"))


@pytest.fixture
def ev(evaluator):
    evaluator.set_kernel("auto")
    yield evaluator
    evaluator.set_kernel("auto")
    evaluator.set_option(_lib.OPT_PICK_FROM_MASK, 0)
    evaluator.set_option(_lib.OPT_FUSED_PICK, 1)


def set_cluster(ev, c):
    ev.set_nodes(c.avail_cpu, c.avail_mem, c.node_labels if c.n_keys else None, c.node_taints if c.n_taints else None)


def preds(c):
    return FIT | (SEL if c.n_keys else 0) | (TAINT if c.n_taints else 0)


# ---- 1. every op at the knife edges ---------------------------------------------------------------------------------------------------
EDGE_NODES = [1, 63, 64, 65, 127, 129, 1024, 1025, 2049]  # W = 1, 1, 1, 2, 2, 3, 16, 17, 33: one, two and three 1024-node tiles
EDGE_PODS = [1, 37, 257]
_EDGE = {}


def edge_case(n, P):
    """the cluster, its flags and the oracle's mask of P pods x n nodes: computed once, read-only"""
    if (n, P) not in _EDGE:
        c = synth.make_cluster(P, n, n_keys=4, n_taints=0, seed=0xE6000 + n)
        feas = oracle_mask(c, preds(c))
        feas.setflags(write=False)
        _EDGE[(n, P)] = (c, feas)
    return _EDGE[(n, P)]


def first_pods(cols, p):
    """the first p pods of pod_tensors' columns ([P] or [n_keys, P], or None)"""
    return tuple(None if t is None else t[:p] if t.dim() == 1 else t[:, :p].contiguous() for t in cols)


def combine_once(ev, cols, flags, op, n, p, pitch, offset, feas, rng, what):
    """One combining call into a [p, W] view of rows `pitch` words apart that starts `offset` words into its buffer; behind the view's rows
    lie GUARD_ROWS more.  Old words [0, W) random (garbage at and beyond n included), every other word of the buffer the sentinel."""
    import torch
    W = (n + 63) // 64
    rows = p + GUARD_ROWS
    host = np.full(offset + rows * pitch + 1, SENTINEL, dtype=np.uint64)
    body = host[offset:offset + rows * pitch].reshape(rows, pitch)
    old = rng.integers(0, 1 << 64, size=(p, W), dtype=np.uint64)
    old[0] = 0xFFFFFFFFFFFFFFFF  # a row of ones: everything at and beyond n is set
    body[:p, :W] = old
    buf = torch.from_numpy(host.view(np.int64)).to(dev_of(ev))
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + rows * pitch].view(rows, pitch)[:p, :W]
    assert view.data_ptr() % 16 == 8 * (offset % 2) and (p == 1 or view.stride(0) == pitch)
    ev.eval_device(*first_pods(cols, p), None, flags | op, out_feasible=view)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    got_body = got[offset:offset + rows * pitch].reshape(rows, pitch)
    want = combine_ref.combine(old, feas[:p], op, n)
    assert np.array_equal(got_body[:p, :W], want), f"{what}: pods {np.nonzero((got_body[:p, :W] != want).any(axis=1))[0][:5]} differ from combine_ref"
    pad = got_body[:p, W:]
    assert ((pad == SENTINEL) | (pad == 0)).all(), f"{what}: a padding word is neither untouched nor zero"
    assert (got_body[p:] == SENTINEL).all(), f"{what}: wrote into the guard rows"
    assert (got[:offset] == SENTINEL).all() and got[-1] == SENTINEL, f"{what}: wrote outside the view"


@pytest.mark.parametrize("kernel", ["direct", "auto"])
@pytest.mark.parametrize("n", EDGE_NODES)
def test_every_op_at_the_knife_edges(ev, n, kernel):
    c, feas = edge_case(n, max(EDGE_PODS))
    set_cluster(ev, c)
    W = ev.W
    assert W == (n + 63) // 64
    cols = pod_tensors(ev, c)
    flags = preds(c)
    # the mask kernel a plain call of this snapshot runs under `kernel`: a combining call names the same one
    ev.set_kernel(kernel)
    plain = ev.alloc_mask(max(EDGE_PODS), pitched=False)
    ev.eval_device(*cols, None, flags, out_feasible=plain)
    name = ev.last_kernel
    assert name == "direct" if kernel == "direct" else name in ("direct", "fused")
    assert np.array_equal(mask_np(plain), feas), "the plain call is the oracle's mask"
    std = int(_lib.load().ksched_mask_pitch(n))
    assert std % 16 == 0 and std >= W
    rng = np.random.default_rng([0xE6, n])
    for p in EDGE_PODS:
        for pitch, offset in ((W, 0), (W + 1, 0), (std, 0), (std, 1), (W, 1)):
            for op, op_id in zip(OPS, OP_IDS):
                combine_once(ev, cols, flags, op, n, p, pitch, offset, feas, rng, f"n = {n}, {kernel}, p = {p}, pitch {pitch}, offset {offset}, {op_id}")
                assert ev.last_kernel == name and ev.last_pick == "none"


@pytest.mark.parametrize("kernel", ["direct", "auto"])
def test_more_than_one_grid_pass(ev, kernel):
    """n = 65 (W = 2): one more row than a full grid of 16-byte units covers in one pass; packed and aligned (one unit per row, two passes),
    one word into the buffer (two one-word units per row, three passes) and at pitch W + 1 (odd: one-word units)"""
    block, max_grid = plan_constants()
    n, p = 65, block * max_grid + 1
    c, feas = edge_case(n, p)
    set_cluster(ev, c)
    assert ev.W == 2
    cols = pod_tensors(ev, c)
    ev.set_kernel(kernel)
    rng = np.random.default_rng([0xE6, n, p])
    for (pitch, offset), op in zip(((2, 0), (2, 1), (3, 0)), OPS):
        combine_once(ev, cols, preds(c), op, n, p, pitch, offset, feas, rng, f"n = {n}, {kernel}, p = {p}, pitch {pitch}, offset {offset}, op {op:#x}")


# ---- 2. the recipe ------------------------------------------------------------------------------------------------------------------------
ZONE, DISK, ZONE_A, ZONE_B, DISK_HDD = 2, 1, 1, 3, 2  # label keys (4 and 3 values; a tenth of the nodes carry none) and the values asked for


@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
@pytest.mark.parametrize("kernel", ["direct", "auto"])
def test_the_recipe_as_a_chain(ev, kernel, pitched):
    """zone In {a, b} and disk NotIn {hdd} and fit, then the spread pick: four calls on one mask"""
    import torch
    P, N, d = 200, 300, 3
    c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=0xE6C4A1)
    c.req_mem[0] = 1 << 60  # a pod that fits nowhere: its row ends empty, its binding -1
    set_cluster(ev, c)
    ev.set_kernel(kernel)
    cpu, mem, _, _ = pod_tensors(ev, c)

    def sel_of(key, value):
        s = np.zeros((c.n_keys, P), dtype=np.uint32)
        s[key] = value
        return to_dev(ev, s, np.int32)
    # written from the label columns, not from masks
    zone, disk = c.node_labels[ZONE], c.node_labels[DISK]
    node_ok = ((zone == ZONE_A) | (zone == ZONE_B)) & (disk != DISK_HDD)
    fits = (c.req_cpu[:, None] <= c.avail_cpu[None, :]) & (c.req_mem[:, None] <= c.avail_mem[None, :])
    bits = fits & node_ok[None, :]
    want = pack_mask(bits)
    assert 0 < node_ok.sum() < N and (disk == 0).any() and bits.any() and not fits.all() and (bits.sum(axis=1) == 0).any()
    draws = np.random.default_rng(0xE6C4).integers(0, 1 << 32, size=(P, d), dtype=np.uint64).astype(np.uint32)
    smp = to_dev(ev, draws, np.int32)
    M = ev.alloc_mask(P, pitched=pitched)
    M.fill_(-1)  # whatever the mask held before the chain
    out = fresh(ev, P, 4)
    ev.eval_device(cpu, mem, sel_of(ZONE, ZONE_A), None, None, SEL, out_feasible=M)
    ev.eval_device(cpu, mem, sel_of(ZONE, ZONE_B), None, None, SEL | COMBINE_OR, out_feasible=M)
    assert ev.last_pick == "none"
    ev.eval_device(cpu, mem, sel_of(DISK, DISK_HDD), None, None, SEL | COMBINE_ANDNOT, out_feasible=M)
    ev.eval_device(cpu, mem, None, None, smp, FIT | COMBINE_AND | PICK_SPREAD, out_feasible=M, out_binding=out[:P])
    assert ev.last_pick == "spread"
    torch.cuda.synchronize()
    got = mask_np(M)
    assert np.array_equal(got, want), f"pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from the label columns' answer"
    b = out.cpu().numpy()
    assert np.array_equal(b[:P], spread_pick(got, draws, N, c.avail_mem, c.avail_cpu)) and (b[P:] == -7).all()
    assert b[0] == -1 and (b[1:P] >= 0).any()


# ---- 3. a pick in a combining call ----------------------------------------------------------------------------------------------------------
PICKS = [(PICK_SAMPLED, "from-mask"), (PICK_BESTFIT, "from-mask"), (PICK_UNIFORM, "uniform"), (PICK_SPREAD, "spread"), (PICK_PACK, "pack")]
_PICK_CASE = {}


def pick_case():
    if not _PICK_CASE:
        P, N = 300, 700
        c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=0xE6B1C)
        feas = oracle_mask(c, preds(c))
        rng = np.random.default_rng(0xE6B1)
        old = pack_mask(rng.random((P, N)) < 0.3)
        old[0] = 0  # an empty row: AND and AND-NOT leave no node
        draws = rng.integers(0, 1 << 32, size=(P, 5), dtype=np.uint64).astype(np.uint32)
        for a in (feas, old, draws):
            a.setflags(write=False)
        _PICK_CASE.update(c=c, feas=feas, old=old, draws=draws)
    return _PICK_CASE


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("pick,last_pick", PICKS, ids=["sampled", "bestfit", "uniform", "spread", "pack"])
def test_a_pick_in_a_combining_call_is_the_pick_from_the_combined_mask(ev, pick, last_pick, op):
    """... with the pick flag alone and no predicate flag, under either setting of KSCHED_OPT_PICK_FROM_MASK and with the riding pick on or off"""
    import torch
    k = pick_case()
    c, N = k["c"], k["c"].N
    P = c.P
    set_cluster(ev, c)
    cols = pod_tensors(ev, c)
    want = combine_ref.combine(k["old"], k["feas"], op, N)
    smp = to_dev(ev, c.samples if pick == PICK_SAMPLED else k["draws"], np.int32) if pick != PICK_BESTFIT else None
    combined = to_dev(ev, want, np.int64)
    alone = fresh(ev, P)
    ev.pick_device(combined, pick, alone, req_mem_bytes=cols[1], samples=smp)
    torch.cuda.synchronize()
    alone = alone.cpu().numpy()
    assert (alone >= 0).any() and ((alone >= 0) <= want.any(axis=1)).all()
    for from_mask, fused_pick in ((0, 1), (1, 1), (0, 0)):
        ev.set_option(_lib.OPT_PICK_FROM_MASK, from_mask)
        ev.set_option(_lib.OPT_FUSED_PICK, fused_pick)
        M = to_dev(ev, k["old"], np.int64)
        out = fresh(ev, P, 4)
        ev.eval_device(*cols, smp, preds(c) | op | pick, out_feasible=M, out_binding=out[:P])
        assert ev.last_pick == last_pick
        torch.cuda.synchronize()
        assert np.array_equal(mask_np(M), want)
        b = out.cpu().numpy()
        assert np.array_equal(b[:P], alone), f"pods {np.nonzero(b[:P] != alone)[0][:5]} differ from ksched_pick_device on the combined mask"
        assert (b[P:] == -7).all()


def test_best_fit_is_not_told_that_the_combined_mask_includes_the_fit(ev):
    """two nodes with avail_mem = [5, 100], one pod with req_mem = 10, the old mask holds node 0: FIT | COMBINE_OR | PICK_BESTFIT combines to
    {0, 1} and binds node 0, the smallest residual; a pick that skips candidates by req_mem would bind node 1"""
    import torch
    ev.set_nodes(np.array([1000, 1000], np.int64), np.array([5, 100], np.int64))
    cpu, mem = to_dev(ev, np.array([1], np.int64), np.int64), to_dev(ev, np.array([10], np.int64), np.int64)
    for kernel in ("direct", "auto"):
        ev.set_kernel(kernel)
        M = to_dev(ev, np.array([[1]], np.uint64), np.int64)
        out = fresh(ev, 1, 2)
        ev.eval_device(cpu, mem, None, None, None, FIT | COMBINE_OR | PICK_BESTFIT, out_feasible=M, out_binding=out[:1])
        assert ev.last_pick == "from-mask"
        torch.cuda.synchronize()
        assert mask_np(M).tolist() == [[3]] and out.cpu().numpy().tolist() == [0, -7, -7]


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_refusals_leave_mask_and_bindings_untouched(ev, op):
    import torch
    c = synth.make_cluster(40, 130, n_keys=4, n_taints=0, seed=0xE6E44)
    set_cluster(ev, c)
    P, W = c.P, ev.W
    lib, h = _lib.load(), ev._h
    cpu, mem, sel, _ = pod_tensors(ev, c)
    smp = to_dev(ev, c.samples, np.int32)
    dM, dF = (torch.full((P, W), 0x5A5A5A5A, dtype=torch.int64, device=dev_of(ev)) for _ in range(2))
    dB = fresh(ev, P)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    other = COMBINE_OR if op != COMBINE_OR else COMBINE_ANDNOT
    f = FIT | SEL | op
    st = C.c_void_p(torch.cuda.current_stream(ev.device).cuda_stream)

    def device(flags, feas, fit, bind, attempts=0, samples=None, p=P):
        return lib.ksched_eval_device_pitched(h, p, vp(cpu), vp(mem), vp(sel), None, vp(samples), attempts, flags, vp(feas), vp(fit), vp(bind), W, st)
    # the accepting entry points: two flags, no mask, a fit mask
    assert device(f | other, dM, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_AND | COMBINE_OR | COMBINE_ANDNOT, dM, None, None) == _lib.E_INVAL
    assert device(f, None, None, None) == _lib.E_INVAL
    assert device(f | PICK_UNIFORM, None, None, dB, 5, smp) == _lib.E_INVAL, "a pick does not stand in for the mask"
    assert device(f | WANT_FIT_MASK, dM, dF, None) == _lib.E_INVAL
    assert device(f | WANT_FIT_MASK, dM, None, None) == _lib.E_INVAL
    assert device(f, dM, dF, None) == _lib.E_INVAL
    assert device(f | 0x1000, dM, None, None) == _lib.E_INVAL, "0x1000 stays unknown"
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, f | other, vp(dM), None, None, st) == _lib.E_INVAL
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, f, None, None, None, st) == _lib.E_INVAL
    # p == 0: a no-op
    assert device(f | PICK_UNIFORM, dM, None, dB, 5, smp, p=0) == _lib.OK
    # the entry points that do not take the flags
    hM, hB = np.full((P, W), SENTINEL, np.uint64), np.full(P, -7, np.int32)
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), None, None, None, 0, FIT | op, hp(hM), None, None) == _lib.E_INVAL
    assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), None, None, hp(c.samples), 5, FIT | op | PICK_UNIFORM, hp(hM), None, hp(hB)) == _lib.E_INVAL
    dev_b, stream = C.c_void_p(), C.c_void_p()
    assert lib.ksched_eval_begin(h, P, hp(c.req_cpu), hp(c.req_mem), None, P, None, None, 0, FIT | op, hp(hM), None, P, C.byref(dev_b), C.byref(stream)) == _lib.E_INVAL
    assert not dev_b.value
    assert lib.ksched_pick(h, P, hp(hM), None, hp(c.samples), 5, PICK_UNIFORM | op, hp(hB)) == _lib.E_INVAL
    assert lib.ksched_pick_device(h, P, vp(dM), W, None, vp(smp), 5, PICK_UNIFORM | op, vp(dB), st) == _lib.E_INVAL
    table = torch.full((P, _lib.SUMMARY_WORDS), -7, dtype=torch.int32, device=dev_of(ev))
    assert lib.ksched_summarize_device(h, P, vp(cpu), vp(mem), vp(sel), None, f, vp(table), st) == _lib.E_INVAL
    pipe = ev.pipe(2)
    try:
        assert lib.ksched_pipe_submit(pipe._h, 0, P, vp(cpu), vp(mem), vp(sel), None, vp(smp), 5, f | PICK_UNIFORM, vp(dM), W, vp(dB)) == _lib.E_INVAL
    finally:
        pipe.close()
    torch.cuda.synchronize()
    assert (dM == 0x5A5A5A5A).all() and (dF == 0x5A5A5A5A).all() and (dB == -7).all() and (table == -7).all()
    assert (hM == SENTINEL).all() and (hB == -7).all()


def test_a_forced_fused_kernel_without_an_index_is_unsupported(ev):
    """three high-cardinality keys: no bitmap index.  auto combines behind the direct kernel; forcing the fused one is KSCHED_E_UNSUPPORTED
    with nothing enqueued"""
    import torch
    rng = np.random.default_rng(0xE6F)
    N, P = 700, 50
    lab = rng.integers(1, 4_000_000, size=(3, N)).astype(np.uint32)
    sel = np.zeros((3, P), dtype=np.uint32)
    sel[0, ::3] = lab[0, rng.integers(0, N, size=len(sel[0, ::3]))]
    cpu, mem = rng.integers(0, 1000, N).astype(np.int64), rng.integers(0, 1000, N).astype(np.int64)
    rc, rm = rng.integers(0, 1000, P).astype(np.int64), rng.integers(0, 1000, P).astype(np.int64)
    ev.set_nodes(cpu, mem, lab)
    from oracle import capi
    feas, _, _ = capi.eval_encoded(cpu, mem, lab, None, rc, rm, sel, None, None, FIT | SEL)
    old = pack_mask(rng.random((P, N)) < 0.5)
    cols = (to_dev(ev, rc, np.int64), to_dev(ev, rm, np.int64), to_dev(ev, sel, np.int32))
    smp = to_dev(ev, rng.integers(0, 1 << 32, size=(P, 2), dtype=np.uint64).astype(np.uint32), np.int32)
    M = to_dev(ev, old, np.int64)
    ev.eval_device(*cols, None, None, FIT | SEL | COMBINE_AND, out_feasible=M)
    assert ev.last_kernel == "direct"
    torch.cuda.synchronize()
    assert np.array_equal(mask_np(M), combine_ref.combine(old, feas, COMBINE_AND, N))
    ev.set_kernel("fused")
    lib, st = _lib.load(), C.c_void_p(torch.cuda.current_stream(ev.device).cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for op in OPS:
        M = to_dev(ev, old, np.int64)
        out = fresh(ev, P)
        rc_ = lib.ksched_eval_device(ev._h, P, vp(cols[0]), vp(cols[1]), vp(cols[2]), None, vp(smp), 2, FIT | SEL | op | PICK_SPREAD, vp(M), None, vp(out), st)
        assert rc_ == _lib.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert np.array_equal(mask_np(M), old) and (out == -7).all()


# ---- 5. two users of the scratch mask ---------------------------------------------------------------------------------------------------------
def test_a_combining_call_and_a_scratch_mask_pick_on_two_streams(ev):
    """stream A: combining calls (they evaluate into the ctx's scratch mask); stream B: uniform picks without out_feasible (they do too), with
    other predicates; enqueued alternately, each gives its single-stream answer"""
    import torch
    from tests.uniform_ref import uniform_pick
    k = pick_case()
    c, N, P = k["c"], k["c"].N, k["c"].P
    set_cluster(ev, c)
    cols = pod_tensors(ev, c)
    smp = to_dev(ev, k["draws"], np.int32)
    want_masks = [combine_ref.combine(k["old"], k["feas"], op, N) for op in OPS]
    fit_only = oracle_mask(c, FIT)
    want_pick = uniform_pick(fit_only, k["draws"][:, 0], N)
    rounds = 2 * len(OPS)
    masks = [to_dev(ev, k["old"], np.int64) for _ in range(rounds)]
    outs = [fresh(ev, P) for _ in range(rounds)]
    a, b = torch.cuda.Stream(ev.device), torch.cuda.Stream(ev.device)
    torch.cuda.synchronize()
    try:
        for i in range(rounds):
            ev.eval_device(*cols, None, preds(c) | OPS[i % 3], out_feasible=masks[i], stream=a)
            ev.eval_device(cols[0], cols[1], None, None, smp, FIT | PICK_UNIFORM, out_binding=outs[i], stream=b)
        torch.cuda.synchronize()
        for i in range(rounds):
            assert np.array_equal(mask_np(masks[i]), want_masks[i % 3]), f"round {i}: the combined mask"
            assert np.array_equal(outs[i].cpu().numpy(), want_pick), f"round {i}: the pick from the scratch mask"
    finally:
        ev.forget_stream(a)
        ev.forget_stream(b)
