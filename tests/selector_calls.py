"""What the GPU suites of the three selector calls (tests/test_gpu_selop.py, test_gpu_seltag.py, test_gpu_selterms.py) share: the `ev`
fixture, the guarded evaluation into a view, small clusters, and the test bodies that are the same for every call -- each takes a
SelectorCall, the small description of the call under test, and each file keeps its test function as a one-line call of the body.
Shapes, seeds and parametrisations are the files'.  A plain module: no test; the fixture is imported by name into each file."""
import ctypes as C
from typing import Callable, NamedTuple

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (COMBINE_AND, COMBINE_ANDNOT, COMBINE_OR, COMBINE_SOFT, PICK_BESTFIT, PICK_PACK, PICK_SAMPLED, PICK_SPREAD,
                                             PICK_UNIFORM, Evaluator, KschedError, _lib, synth)
from tests import combine_ref, soft_ref
from tests.pick_helpers import dev_of, fresh, mask_np, to_dev
from tests.uniform_ref import uniform_pick

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD_ROWS = 2
COMBINES = [(COMBINE_AND, "and"), (COMBINE_OR, "or"), (COMBINE_ANDNOT, "andnot"), (COMBINE_AND | COMBINE_SOFT, "soft-and"), (COMBINE_ANDNOT | COMBINE_SOFT, "soft-andnot")]
PICKS = [(PICK_SAMPLED, "from-mask"), (PICK_BESTFIT, "from-mask"), (PICK_UNIFORM, "uniform"), (PICK_SPREAD, "spread"), (PICK_PACK, "pack")]


class SelectorCall(NamedTuple):
    flags: int           # KSCHED_SEL and what makes the call an operator, a tagged or a terms call
    last_kernel: str     # ksched_last_kernel after it
    mask: Callable       # mask(labels, table, p=None): the reference's packed rows (table None: no selectors, p rows)
    lead: tuple = ()     # a selector table is lead + (keys, p): () for [keys][p], (T,) for [T][keys][p]


@pytest.fixture
def ev(evaluator):
    evaluator.set_kernel("auto")
    yield evaluator
    evaluator.set_kernel("auto")
    evaluator.set_option(_lib.OPT_PICK_FROM_MASK, 0)
    evaluator.set_option(_lib.OPT_FUSED_PICK, 1)


def as_signed(x):
    return x.astype(np.uint32).astype(np.int32)


def row_kinds(m, n):
    """(rows with every node, rows with none, rows that are neither) of packed rows over n nodes"""
    count = np.unpackbits(np.ascontiguousarray(m).view(np.uint8), axis=1).sum(axis=1)
    return int((count == n).sum()), int((count == 0).sum()), int(((count > 0) & (count < n)).sum())


def combined(old, new, comb, n):
    return soft_ref.soft_combine(old, new, comb, n) if comb & COMBINE_SOFT else combine_ref.combine(old, new, comb, n)


def zeros_dev(ev, p):
    import torch
    return torch.zeros(p, dtype=torch.int64, device=dev_of(ev))


def eval_into_view(ev, sel, flags, n, p, pitch, offset, old=None):
    """One evaluation of the first p pods of `sel` ([keys][P] or [T][keys][P] numpy, or None) into a [p, W] view of rows `pitch` words apart
    that starts `offset` words into its buffer; behind the view's rows lie GUARD_ROWS more.  Every word of the buffer is the sentinel (words
    [0, W) of the rows: `old`, where given).  Returns the rows; the padding words, the guard rows and the words outside the view are checked
    here."""
    import torch
    W = (n + 63) // 64
    rows = p + GUARD_ROWS
    host = np.full(offset + rows * pitch + 1, SENTINEL, dtype=np.uint64)
    body = host[offset:offset + rows * pitch].reshape(rows, pitch)
    if old is not None:
        body[:p, :W] = old[:p]
    buf = torch.from_numpy(host.view(np.int64)).to(dev_of(ev))
    view = buf[offset:offset + rows * pitch].view(rows, pitch)[:p, :W]
    assert p == 1 or view.stride(0) == pitch
    sel_t = None if sel is None else to_dev(ev, np.ascontiguousarray(sel[..., :p]), np.int32)
    ev.eval_device(zeros_dev(ev, p), zeros_dev(ev, p), sel_t, None, None, flags, out_feasible=view)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    got_body = got[offset:offset + rows * pitch].reshape(rows, pitch)
    pad = got_body[:p, W:]
    assert ((pad == SENTINEL) | (pad == 0)).all(), "a padding word is neither untouched nor zero"
    assert (got_body[p:] == SENTINEL).all(), "wrote into the guard rows"
    assert (got[:offset] == SENTINEL).all() and got[-1] == SENTINEL, "wrote outside the view"
    return got_body[:p, :W].copy()


def indexed_cluster():
    c = synth.make_cluster(129, 1500, n_keys=8, n_taints=0, seed=0xE8001)
    return c.avail_cpu, c.avail_mem, c.node_labels, np.ascontiguousarray(c.pod_sel)


GPU_KEY, CORES_KEY, ZONE_KEY, ZONE_3 = 0, 1, 2, 3


def recipe_cluster(seed):
    """synth's capacities and requests (cluster seed `seed << 8 | 0xA1`, label seed `seed`) under labels of the recipe's own: gpu present on
    three nodes in five, cores = 4 .. 64 interned as id = cores + 1 (a tenth of the nodes carry none), zone 1 .. 3 (a tenth none)"""
    P, N = 200, 300
    c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=seed << 8 | 0xA1)
    c.req_mem[0] = 1 << 60  # pod 0 fits nowhere
    rng = np.random.default_rng(seed)
    lab = c.node_labels.copy()
    lab[GPU_KEY] = np.where(rng.random(N) < 0.6, 1, 0)
    lab[CORES_KEY] = np.where(rng.random(N) < 0.1, 0, np.array([4, 8, 16, 32, 64])[rng.integers(0, 5, N)] + 1)
    lab[ZONE_KEY] = np.where(rng.random(N) < 0.1, 0, rng.integers(1, 4, N))
    return c, lab.astype(np.uint32)


# ---- the bodies ---------------------------------------------------------------------------------------------------------------------------
def no_selectors_and_no_keys_pass_every_node(ev, with_keys, without_keys, seed, ids):
    """the calls `with_keys` without selectors on a snapshot of two keys, then `without_keys` on one without keys: every node; returns the rows"""
    n, p = 65, 3
    lab = ids[np.random.default_rng(seed).integers(0, ids.size, size=(2, n))]
    full = with_keys[0].mask(lab, None, p=p)
    assert full.tolist() == [[0xFFFFFFFFFFFFFFFF, 1]] * p
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), lab)
    for call in with_keys:
        got = eval_into_view(ev, None, call.flags, n, p, 2, 0)
        assert np.array_equal(got, full) and ev.last_kernel == call.last_kernel
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), None)
    assert ev.n_keys == 0
    for call in without_keys:
        got = eval_into_view(ev, None, call.flags, n, p, 16, 1)
        assert np.array_equal(got, full) and ev.last_kernel == call.last_kernel
    return full


def the_call_under_every_combine(ev, call, lab, sel, new, comb, rng):
    """the call of table `sel` (reference rows `new`) into a caller's mask drawn from `rng`, with garbage at and beyond n, at three layouts"""
    n, p = 1025, 129
    W = (n + 63) // 64
    old = rng.integers(0, 1 << 64, size=(p, W), dtype=np.uint64)
    old[::5] &= rng.integers(0, 1 << 64, size=(len(old[::5]), W), dtype=np.uint64) & rng.integers(0, 1 << 64, size=(len(old[::5]), W), dtype=np.uint64)
    old[:, -1] |= ~np.uint64(combine_ref.valid_bits_word(n))  # garbage at and beyond n
    want = combined(old, new, comb, n)
    assert not np.array_equal(want, new) and not np.array_equal(want, soft_ref.old_prime(old, n)), "the combine shows"
    if comb & COMBINE_SOFT:
        what = soft_ref.decisions(old, new, comb, n)
        assert (what == soft_ref.NARROWED).any() and (what == soft_ref.DROPPED).any(), "rows that narrow and rows whose tier is dropped"
        assert not np.array_equal(want, combine_ref.combine(old, new, comb & ~COMBINE_SOFT, n))
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), lab)
    std = int(_lib.load().ksched_mask_pitch(n))
    for pitch, offset in ((W, 0), (std, 0), (W, 1)):
        got = eval_into_view(ev, sel, call.flags | comb, n, p, pitch, offset, old=old)
        assert np.array_equal(got, want), f"pitch {pitch}, offset {offset}: pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ"
        assert ev.last_kernel == call.last_kernel and ev.last_pick == "none"


def a_pick_in_the_call_is_the_pick_from_the_resulting_mask(ev, call, k, new, pick, last_pick, options=((0, 1), (1, 1), (0, 0))):
    """plain (with and without out_feasible) and combining, under each (KSCHED_OPT_PICK_FROM_MASK, KSCHED_OPT_FUSED_PICK) of `options`: the
    bindings of ksched_pick_device on the resulting mask with the pick flag alone.  k: a pick case (c, sel, old, draws); new: its reference rows"""
    import torch
    c = k["c"]
    P, N = c.P, c.N
    ev.set_nodes(c.avail_cpu, c.avail_mem, c.node_labels)
    cpu, mem = to_dev(ev, c.req_cpu, np.int64), to_dev(ev, c.req_mem, np.int64)
    sel = to_dev(ev, k["sel"], np.int32)
    smp = to_dev(ev, c.samples if pick == PICK_SAMPLED else k["draws"], np.int32) if pick != PICK_BESTFIT else None
    masks = {0: new, COMBINE_AND: combine_ref.combine(k["old"], new, COMBINE_AND, N)}
    for comb, want in masks.items():
        f, e, m = row_kinds(want, N)
        assert e >= 1 and m > P // 4, "pods without a node, and many with some but not all"
        alone = fresh(ev, P)
        ev.pick_device(to_dev(ev, want, np.int64), pick, alone, req_mem_bytes=mem, samples=smp)
        torch.cuda.synchronize()
        alone = alone.cpu().numpy()
        assert (alone >= 0).any() and ((alone >= 0) <= want.any(axis=1)).all()
        if pick == PICK_UNIFORM:
            assert np.array_equal(alone, uniform_pick(want, k["draws"][:, 0], N))
        for from_mask, fused_pick in options:
            ev.set_option(_lib.OPT_PICK_FROM_MASK, from_mask)
            ev.set_option(_lib.OPT_FUSED_PICK, fused_pick)
            for with_mask in ([True] if comb else [True, False]):
                M = to_dev(ev, k["old"], np.int64) if with_mask else None
                out = fresh(ev, P, 4)
                ev.eval_device(cpu, mem, sel, None, smp, call.flags | comb | pick, out_feasible=M, out_binding=out[:P])
                assert ev.last_pick == last_pick and ev.last_kernel == call.last_kernel
                torch.cuda.synchronize()
                if with_mask:
                    assert np.array_equal(mask_np(M), want)
                b = out.cpu().numpy()
                assert np.array_equal(b[:P], alone), f"pods {np.nonzero(b[:P] != alone)[0][:5]} differ from ksched_pick_device on the mask"
                assert (b[P:] == -7).all()


def the_host_forms_give_the_device_forms_bits(ev, call, k, want, lo=0, p=None):
    """ksched_eval, and ksched_eval_begin / _end over rows [lo, lo + p) of the batch (all of it by default: sel_stride == p), against the
    reference rows `want` and, first, the device form.  k: a pick case (c, sel, draws)"""
    import torch
    c = k["c"]
    P, N = c.P, c.N
    p = P if p is None else p
    ev.set_nodes(c.avail_cpu, c.avail_mem, c.node_labels)
    W = ev.W
    M = torch.full((P, W), 0x5A, dtype=torch.int64, device=dev_of(ev))
    ev.eval_device(zeros_dev(ev, P), zeros_dev(ev, P), to_dev(ev, k["sel"], np.int32), None, None, call.flags, out_feasible=M)
    torch.cuda.synchronize()
    assert np.array_equal(mask_np(M), want), "the device form"
    picked = uniform_pick(want, k["draws"][:, 0], N)
    r = ev.eval(c.req_cpu, c.req_mem, k["sel"], None, None, call.flags)
    assert np.array_equal(r.feasible, want) and r.binding is None and ev.last_kernel == call.last_kernel and ev.last_pick == "none"
    r = ev.eval(c.req_cpu, c.req_mem, k["sel"].reshape(-1, P), None, k["draws"], call.flags | PICK_UNIFORM)  # ([T * keys][p] is the same array)
    assert np.array_equal(r.feasible, want) and np.array_equal(r.binding, picked) and ev.last_pick == "uniform"
    r = ev.eval(c.req_cpu, c.req_mem, k["sel"], None, k["draws"], call.flags | PICK_UNIFORM, want_mask=False)
    assert r.feasible is None and np.array_equal(r.binding, picked)
    # the two halves: column (t, k) starts (t * n_keys + k) * sel_stride entries in
    stride = P
    sub = want[lo:lo + p]
    sub_picked = uniform_pick(sub, k["draws"][lo:lo + p, 0], N)
    assert p == P or (stride > p and row_kinds(sub, N)[2] > p // 4)
    lib, hp = ev._lib, lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    feas = np.full((p, W), SENTINEL, dtype=np.uint64)
    part = np.full(p + 3, 555, dtype=np.int32)
    dev_b, stream = C.c_void_p(), C.c_void_p()
    flat = np.ascontiguousarray(k["sel"]).reshape(-1)
    draws = np.ascontiguousarray(k["draws"][lo:lo + p])
    rc = lib.ksched_eval_begin(ev._h, p, hp(c.req_cpu[lo:]), hp(c.req_mem[lo:]), hp(flat[lo:]), stride, None, hp(draws), 5, call.flags | PICK_UNIFORM, hp(feas), None,
                               p + 3, C.byref(dev_b), C.byref(stream))
    assert rc == _lib.OK and dev_b.value
    assert lib.ksched_eval_end(ev._h, dev_b, p + 3, hp(part)) == _lib.OK
    assert np.array_equal(feas, sub) and np.array_equal(part[:p], sub_picked) and (part[p:] == -1).all()
    assert ev.last_kernel == call.last_kernel


def two_streams_around_a_label_update(ev, call, c, sel, rng):
    """the call on stream A, a label update drawn from `rng`, the call on stream B, no host wait in between: each call sees the labels that
    were current when it was enqueued"""
    import torch
    lab = c.node_labels.copy()
    n, p = c.N, c.P
    idx = rng.choice(n, size=400, replace=False).astype(np.uint32)
    rows = rng.integers(0, lab.max(axis=1)[:, None] + 1, size=(8, idx.size)).astype(np.uint32)
    lab_after = lab.copy()
    lab_after[:, idx] = rows
    want_a, want_b = call.mask(lab, sel), call.mask(lab_after, sel)
    assert not np.array_equal(want_a, want_b)
    ev.set_nodes(c.avail_cpu, c.avail_mem, lab)
    cpu, mem, sel_t = zeros_dev(ev, p), zeros_dev(ev, p), to_dev(ev, sel, np.int32)
    a, b = torch.cuda.Stream(ev.device), torch.cuda.Stream(ev.device)
    rounds = 3
    masks_a = [ev.alloc_mask(p, pitched=True) for _ in range(rounds)]
    masks_b = [ev.alloc_mask(p, pitched=False) for _ in range(rounds)]
    for m in masks_a + masks_b:
        m.fill_(0x5A)
    torch.cuda.synchronize()
    try:
        for i in range(rounds):
            ev.eval_device(cpu, mem, sel_t, None, None, call.flags, out_feasible=masks_a[i], stream=a)
            ev.update_node_labels(idx, rows)
            ev.eval_device(cpu, mem, sel_t, None, None, call.flags, out_feasible=masks_b[i], stream=b)
            if i + 1 < rounds:
                ev.update_node_labels(idx, np.ascontiguousarray(lab[:, idx]))  # back to the first labels for the next round
        torch.cuda.synchronize()
        for i in range(rounds):
            assert np.array_equal(mask_np(masks_a[i]), want_a), f"round {i}, stream A: the labels before the update"
            assert np.array_equal(mask_np(masks_b[i]), want_b), f"round {i}, stream B: the labels after it"
    finally:
        ev.forget_stream(a)
        ev.forget_stream(b)


def edge_sizes(call, comb=COMBINE_AND, then=None):
    """no snapshot, n == 0 (plain and under `comb`), p == 0, on a fresh evaluator; then(e), where given, on the snapshot of two keys over 70 nodes"""
    import torch
    e = Evaluator(0)
    try:
        dev = torch.device("cuda", 0)
        cpu = torch.zeros(5, dtype=torch.int64, device=dev)
        sel = torch.ones(call.lead + (2, 5), dtype=torch.int32, device=dev)
        smp = torch.zeros((5, 3), dtype=torch.int32, device=dev)
        M = torch.full((5, 2), 0x5A, dtype=torch.int64, device=dev)
        B = torch.full((5,), -7, dtype=torch.int32, device=dev)
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        lib, f = e._lib, call.flags
        # before ksched_set_nodes
        assert lib.ksched_eval_device(e._h, 5, vp(cpu), vp(cpu), vp(sel), None, None, 0, f, vp(M), None, None, st) == _lib.E_STATE
        assert lib.ksched_eval_device_pitched(e._h, 5, vp(cpu), vp(cpu), vp(sel), None, vp(smp), 3, f | comb | PICK_UNIFORM, vp(M), None, vp(B), 2, st) == _lib.E_STATE
        with pytest.raises(KschedError) as err:
            e.eval(np.zeros(5, np.int64), np.zeros(5, np.int64), None, None, None, f)
        assert err.value.code == _lib.E_STATE
        # n == 0: the mask is left alone, every pod of a pick gets -1
        e.set_nodes(np.zeros(0, np.int64), np.zeros(0, np.int64))
        for cb in (0, comb):
            B.fill_(-7)
            assert lib.ksched_eval_device_pitched(e._h, 5, vp(cpu), vp(cpu), vp(sel), None, vp(smp), 3, f | cb | PICK_UNIFORM, vp(M), None, vp(B), 2, st) == _lib.OK
            torch.cuda.synchronize()
            assert (M == 0x5A).all() and (B == -1).all()
        # p == 0: a no-op
        e.set_nodes(np.zeros(70, np.int64), np.zeros(70, np.int64), np.ones((2, 70), np.uint32))
        B.fill_(-7)
        assert lib.ksched_eval_device_pitched(e._h, 0, vp(cpu), vp(cpu), vp(sel), None, vp(smp), 3, f | PICK_UNIFORM, vp(M), None, vp(B), 2, st) == _lib.OK
        assert lib.ksched_eval_device_pitched(e._h, 0, None, None, None, None, None, 0, f, vp(M), None, None, 2, st) == _lib.OK
        torch.cuda.synchronize()
        assert (M == 0x5A).all() and (B == -7).all()
        r = e.eval(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(call.lead + (2, 0), np.uint32), None, None, f)
        assert r.feasible.shape == (0, 2)
        if then is not None:
            then(e)
    finally:
        e.close()
