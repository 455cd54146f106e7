"""The mask, summary, explain, sampled-pick and best-fit kernels on the constructed inputs of tests/knife_edges.py, against that module's
plain numpy reference (pinned against the oracle by tests/test_knife_edges_host.py, which also asserts that every input sits on the edge
it aims at): requests equal to, one below and one above every element of a tile's rank search -- the slot-0 rule and each of the ten
descent levels included --, best-fit winners inside the one window of cpu ranks that is tested individually and requests on every block end
of its searches, label ids with bit 31 set at the ends of a tile's sorted list and between its entries, taint bits up to the sign bit, and
columns that reach exactly zero through on-device applies.  Every output goes into a buffer pre-filled with a sentinel.

profiles/knife_edge_checks.txt records which seeded one-line errors in the kernels these cases see and the rest of the suite does not."""
import functools

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (FIT, PICK_BESTFIT, PICK_SAMPLED, SEL, TAINT, WANT_FIT_MASK, Evaluator, _lib)
from kube_scheduler_rs_reference_amd.evaluator import EvalResult
from tests import knife_edges as ke

pytestmark = pytest.mark.gpu

SENT64, SENT32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.int32(-7)
BF_NODES = (1025, ke.bf_two_4096_blocks_n())


# ---- the cases and their expected results, computed once and left unchanged ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, *args):
    if name == "fit_ranks":
        c = ke.fit_ranks()
        return {"set": c, "rotated": ke.rotate_tile0(c)}
    if name == "bestfit_window":
        c = ke.bestfit_window(*args)
        return {"set": c, "swapped": ke.swap_window_cpu(c)}
    if name == "bestfit_orders":
        return {"set": ke.bestfit_orders(*args)}
    if name == "selector_ids":
        c = ke.selector_ids()
        return {"set": c, "relabelled": ke.relabel(c)}
    if name == "taint_bits":
        return {"set": ke.taint_bits()}
    raise KeyError(name)


_expected = {}


def expected(c, flags):
    """{"feasible", "fit"} packed, {"bestfit", "sampled", "counts"} of case `c` under `flags`, by the plain reference; cached per case object"""
    key = (id(c), flags)
    if key not in _expected:
        F, S, T = ke.term_masks(c, flags)
        feas = F & S & T
        e = {"case": c, "feasible": ke.pack(feas), "fit": ke.pack(F), "bestfit": ke.bestfit(c, feas), "counts": ke.counts(c, flags)}
        if c.samples is not None:
            e["sampled"] = ke.sampled(feas, c.samples)
        for a in e.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _expected[key] = e
    return _expected[key]


def evaluate(ev, c, flags, want_mask=True, samples=None):
    """ksched_eval into sentinel-filled buffers"""
    W = (c.N + 63) // 64
    out = EvalResult(feasible=np.full((c.P, W), SENT64, dtype=np.uint64) if want_mask else None,
                     fit=np.full((c.P, W), SENT64, dtype=np.uint64) if flags & WANT_FIT_MASK else None,
                     binding=np.full((c.P,), SENT32, dtype=np.int32) if flags & (PICK_SAMPLED | PICK_BESTFIT) else None)
    r = ev.eval(c.req_cpu, c.req_mem, c.sel, c.tol, samples, flags, want_mask=want_mask, out=out)
    assert r.feasible is out.feasible and r.fit is out.fit and r.binding is out.binding  # (the pre-filled buffers are the ones written)
    return r


def same_rows(got, want, what):
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} pods differ, first {bad[:5].tolist()}: got {got[bad[:3]].tolist()} want {want[bad[:3]].tolist()}"


def load(ev, name, phase, *args):
    """Put the case's snapshot on the device: ksched_set_nodes, then -- in the second phase -- the one update the phase is named after.
    -> the case as the device now holds it"""
    phases = case(name, *args)
    c = phases["set"]
    ev.set_kernel("auto")
    ev.set_nodes(c.cpu, c.mem, c.labels, c.taints)
    if phase == "set":
        return c
    if phase == "relabelled":
        idx, lab, c2 = phases[phase]
        ev.update_node_labels(idx, lab)
    else:
        idx, cpu, mem, c2 = phases[phase]
        ev.update_nodes(idx, cpu, mem)
    return c2


@pytest.fixture(autouse=True)
def default_options(evaluator):
    yield
    ev = evaluator
    ev.set_kernel("auto")
    for opt, v in ((_lib.OPT_FUSED_PICK, 1), (_lib.OPT_ROUND_ORDER, 0), (_lib.OPT_BESTFIT_STAGES, 0), (_lib.OPT_PICK_FROM_MASK, 0)):
        ev.set_option(opt, v)


# ---- fit_ranks: the rank search of the mask and summary kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["fused", "direct"])
@pytest.mark.parametrize("phase", ["set", "rotated"])
def test_fit_ranks_mask_and_fit_mask(evaluator, phase, kernel):
    ev = evaluator
    c = load(ev, "fit_ranks", phase)
    want = expected(c, FIT)
    ev.set_kernel(kernel)
    for order in ((0, 1, 2) if kernel == "fused" else (0,)):
        ev.set_option(_lib.OPT_ROUND_ORDER, order)
        r = evaluate(ev, c, FIT | WANT_FIT_MASK)
        assert ev.last_kernel == kernel
        same_rows(r.feasible, want["feasible"], f"{phase} {kernel} round order {order}: mask")
        same_rows(r.fit, want["fit"], f"{phase} {kernel} round order {order}: fit mask")


@pytest.mark.parametrize("phase", ["set", "rotated"])
def test_fit_ranks_summary(evaluator, phase):
    ev = evaluator
    c = load(ev, "fit_ranks", phase)
    want = expected(c, FIT)["counts"]
    for kernel in ("fused", "direct"):
        ev.set_kernel(kernel)
        got = ev.summarize(c.req_cpu, c.req_mem, None, None, FIT)
        assert ev.last_kernel == kernel
        same_rows(got, want, f"{phase} {kernel}: summary")


@pytest.mark.parametrize("phase", ["set", "rotated"])
def test_fit_ranks_explain(evaluator, phase):
    ev = evaluator
    c = load(ev, "fit_ranks", phase)
    pairs = case("fit_ranks")["set"].pairs  # (pod, the node whose value equals the request) and (pod, the node just below it), as built
    if phase == "rotated":  # the values moved one node on
        pairs = pairs.copy()
        t0 = pairs[:, 1] < ke.TILE
        pairs[t0, 1] = (pairs[t0, 1] + 1) % ke.TILE
    want = ke.reasons(c, FIT, pairs)
    got = ev.explain(c.req_cpu, c.req_mem, None, None, pairs[:, 0], pairs[:, 1], FIT)
    same_rows(got, want, f"{phase}: explain")
    assert (want == 0).sum() > 2000 and (want == 1).sum() > 2000


@pytest.mark.parametrize("ride,how", [(0, "select"), (1, "fused-tile"), (2, "fused"), (3, "fused-tile")])
@pytest.mark.parametrize("phase", ["set", "rotated"])
def test_fit_ranks_sampled_pick(evaluator, phase, ride, how):
    ev = evaluator
    c = load(ev, "fit_ranks", phase)
    smp = c.samples
    if phase == "rotated":  # point the draws at where the values now are
        smp = smp.copy()
        t0 = smp < ke.TILE
        smp[t0] = (smp[t0] + 1) % ke.TILE
    want = expected(c, FIT)
    want_b = ke.sampled(ke.feasible(c, FIT), smp)
    ev.set_kernel("fused")
    ev.set_option(_lib.OPT_FUSED_PICK, ride)
    r = evaluate(ev, c, FIT | PICK_SAMPLED, samples=smp)
    assert ev.last_kernel == "fused" and ev.last_pick == how, (ev.last_kernel, ev.last_pick)
    same_rows(r.binding, want_b, f"{phase} ride {ride}: sampled bindings")
    same_rows(r.feasible, want["feasible"], f"{phase} ride {ride}: mask beside the pick")
    assert all((want_b // ke.TILE == t).sum() > 100 for t in (0, 2)) and (want_b // ke.TILE == 1).sum() >= 10 and (want_b == -1).sum() >= 1


# ---- bestfit_window: the cpu window and the block ends of the best-fit searches -----------------------------------------------------------
@pytest.mark.parametrize("shape", ke.BF_SHAPES)
@pytest.mark.parametrize("n", BF_NODES)
def test_bestfit_window(evaluator, n, shape):
    ev = evaluator
    for phase in ("set", "swapped"):
        c = load(ev, "bestfit_window", phase, n, shape)
        want = expected(c, FIT)
        for stages in (1, 2):
            ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)
            r = evaluate(ev, c, FIT | PICK_BESTFIT, want_mask=False)
            assert ev.last_pick == "bestfit-rows", ev.last_pick
            same_rows(r.binding, want["bestfit"], f"{c.name} {phase} stages {stages}: bindings only")
            if phase == "set":
                r = evaluate(ev, c, FIT | PICK_BESTFIT)
                assert ev.last_pick == "bestfit-rows", ev.last_pick
                same_rows(r.binding, want["bestfit"], f"{c.name} stages {stages}: bindings beside a mask")
                same_rows(r.feasible, want["feasible"], f"{c.name} stages {stages}: mask beside the pick")
        if phase == "set":  # the mask-reading best fit behind the direct kernel
            ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)
            ev.set_option(_lib.OPT_PICK_FROM_MASK, 1)
            ev.set_kernel("direct")
            r = evaluate(ev, c, FIT | PICK_BESTFIT)
            assert ev.last_pick == "from-mask" and ev.last_kernel == "direct", (ev.last_pick, ev.last_kernel)
            same_rows(r.binding, want["bestfit"], f"{c.name}: from the mask")
            ev.set_option(_lib.OPT_PICK_FROM_MASK, 0)


# ---- bestfit_orders: the orders' merge sort at one run, two runs, two runs and a record, three passes ----------------------------------
@pytest.mark.parametrize("n", ke.BF_ORDER_NODES)
def test_bestfit_orders(evaluator, n):
    ev = evaluator
    c = load(ev, "bestfit_orders", "set", n)
    want = expected(c, FIT)
    for stages in (1, 2):
        ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)
        r = evaluate(ev, c, FIT | PICK_BESTFIT, want_mask=False)
        assert ev.last_pick == "bestfit-rows", ev.last_pick
        same_rows(r.binding, want["bestfit"], f"{c.name} stages {stages}: bindings only")
    ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)  # the mask-reading best fit behind the direct kernel
    ev.set_option(_lib.OPT_PICK_FROM_MASK, 1)
    ev.set_kernel("direct")
    r = evaluate(ev, c, FIT | PICK_BESTFIT)
    assert ev.last_pick == "from-mask" and ev.last_kernel == "direct", (ev.last_pick, ev.last_kernel)
    same_rows(r.binding, want["bestfit"], f"{c.name}: from the mask")
    same_rows(r.feasible, want["feasible"], f"{c.name}: the mask")


# ---- selector_ids: label ids with bit 31 set, the ends of the list keys' searches ---------------------------------------------------------
@pytest.mark.parametrize("phase", ["set", "relabelled"])
def test_selector_ids(evaluator, phase):
    ev = evaluator
    c = load(ev, "selector_ids", phase)
    if phase == "set":
        # the planned layout really keeps keys 1 and 2 as lists: the fused kernel applies although their ids would need 2^31 rows, and the index
        # is not the one of the same snapshot with two row keys in their place
        lists = ev.index_checksum()
        rows = c.labels.copy()
        rows[1:] = rows[1:] % 5 + 1
        ev.set_nodes(c.cpu, c.mem, rows, None)
        assert lists != (0, 0) and ev.index_checksum() not in ((0, 0), lists)
        ev.set_nodes(c.cpu, c.mem, c.labels, None)
        assert ev.index_checksum() == lists
    for flags in (SEL, FIT | SEL):
        want = expected(c, flags)
        for kernel in ("fused", "direct"):
            ev.set_kernel(kernel)
            r = evaluate(ev, c, flags | (WANT_FIT_MASK if flags & FIT else 0))
            assert ev.last_kernel == kernel
            same_rows(r.feasible, want["feasible"], f"{phase} {kernel} flags {flags}: mask")
            if flags & FIT:
                same_rows(r.fit, want["fit"], f"{phase} {kernel} flags {flags}: fit mask")
            got = ev.summarize(c.req_cpu, c.req_mem, c.sel, None, flags)
            assert ev.last_kernel == kernel
            same_rows(got, want["counts"], f"{phase} {kernel} flags {flags}: summary")
        ev.set_kernel("auto")
        for stages in (1, 2):  # pods that constrain key 1 or 2 are picked from the keys' sorted lists
            ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)
            r = evaluate(ev, c, flags | PICK_BESTFIT, want_mask=False)
            assert ev.last_pick == "bestfit-rows", ev.last_pick
            same_rows(r.binding, want["bestfit"], f"{phase} flags {flags} stages {stages}: best fit")
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)
        got = ev.explain(c.req_cpu, c.req_mem, c.sel, None, c.pairs[:, 0], c.pairs[:, 1], flags)
        same_rows(got, ke.reasons(c, flags, c.pairs), f"{phase} flags {flags}: explain")
    want = expected(c, FIT | SEL)["bestfit"]
    assert (want >= 0).sum() >= 40 and (want == -1).sum() >= 20


# ---- taint_bits: sixteen groups, the sign bit of the word --------------------------------------------------------------------------------
def test_taint_bits(evaluator):
    ev = evaluator
    c = load(ev, "taint_bits", "set")
    for flags in (TAINT, FIT | TAINT):
        want = expected(c, flags)
        for kernel in ("fused", "direct"):
            ev.set_kernel(kernel)
            r = evaluate(ev, c, flags | (WANT_FIT_MASK if flags & FIT else 0))
            assert ev.last_kernel == kernel
            same_rows(r.feasible, want["feasible"], f"{kernel} flags {flags}: mask")
            if flags & FIT:
                same_rows(r.fit, want["fit"], f"{kernel} flags {flags}: fit mask")
            got = ev.summarize(c.req_cpu, c.req_mem, None, c.tol, flags)
            assert ev.last_kernel == kernel
            same_rows(got, want["counts"], f"{kernel} flags {flags}: summary")
        ev.set_kernel("auto")
        for stages in (1, 2):
            ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)
            r = evaluate(ev, c, flags | PICK_BESTFIT, want_mask=False)
            assert ev.last_pick == "bestfit-rows", ev.last_pick
            same_rows(r.binding, want["bestfit"], f"flags {flags} stages {stages}: best fit")
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)
        ev.set_kernel("fused")
        for ride, how in ((0, "select"), (1, "fused")):
            ev.set_option(_lib.OPT_FUSED_PICK, ride)
            r = evaluate(ev, c, flags | PICK_SAMPLED, samples=c.samples)
            assert ev.last_pick == how, (ride, ev.last_pick)
            same_rows(r.binding, want["sampled"], f"flags {flags} ride {ride}: sampled bindings")
            same_rows(r.feasible, want["feasible"], f"flags {flags} ride {ride}: mask beside the pick")
        ev.set_option(_lib.OPT_FUSED_PICK, 1)
    assert (want["sampled"] == ke.TILE).sum() >= 5 and (want["sampled"] == -1).sum() >= 1


# ---- exact_fill: columns that reach exactly zero through applies on the device -------------------------------------------------------------
def test_exact_fill_three_rounds(evaluator, built):
    import torch

    ev = evaluator
    c, k, r1, r2 = ke.exact_fill()
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    d_cpu, d_mem, d_smp = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.samples, np.int32)
    ev.set_kernel("auto")
    ev.set_nodes(c.cpu, c.mem, None, None)
    spec = Evaluator(0)  # a second ctx that builds its index with the host code that specifies it
    try:
        spec.set_option(_lib.OPT_INDEX_BUILD, 1)
        cur = c
        for j in range(1, 4):
            want = expected(cur, FIT)
            r = evaluate(ev, cur, FIT | WANT_FIT_MASK)
            same_rows(r.feasible, want["feasible"], f"round {j}: mask before the apply")
            bind = torch.full((c.P,), int(SENT32), dtype=torch.int32, device=dev)
            status = torch.full((c.P,), int(SENT32), dtype=torch.int32, device=dev)
            ev.eval_device(d_cpu, d_mem, None, None, d_smp, FIT | PICK_SAMPLED, out_binding=bind)
            ev.apply_bindings_device(bind, d_cpu, d_mem, None, _lib.APPLY_FIRST_PER_NODE, status)
            got_cpu, got_mem = ev.read_nodes()
            same_rows(bind.cpu().numpy(), want["sampled"], f"round {j}: bindings")
            exp_cpu, exp_mem = ke.exact_fill_after(k, r1, r2, j)
            same_rows(got_cpu, exp_cpu, f"round {j}: cpu column")
            same_rows(got_mem, exp_mem, f"round {j}: memory column")
            st = status.cpu().numpy()
            live = want["sampled"][:c.N] >= 0
            assert (st[:c.N][live] == _lib.APPLY_APPLIED).all() and (st[:c.N][~live] == _lib.APPLY_UNBOUND).all()
            assert st[c.N] == _lib.APPLY_APPLIED and (st[c.N + 1:] == _lib.APPLY_DEFERRED).all()  # the zero requests, all on node 0
            cur = c.with_nodes(cpu=exp_cpu, mem=exp_mem)
            want = expected(cur, FIT)
            for kernel in ("fused", "direct"):
                ev.set_kernel(kernel)
                r = evaluate(ev, cur, FIT | WANT_FIT_MASK)
                assert ev.last_kernel == kernel
                same_rows(r.feasible, want["feasible"], f"round {j} {kernel}: mask after the apply")
                same_rows(r.fit, want["fit"], f"round {j} {kernel}: fit mask after the apply")
            ev.set_kernel("auto")
            gone = np.array([int(x) <= j for x in k])
            feas = ke.feasible(cur, FIT)
            assert not feas[:c.N][:, gone].any() and feas[c.N:].all()  # (the property this round is about holds in what was compared)
            spec.set_nodes(exp_cpu, exp_mem, None, None)
            assert ev.index_checksum() == spec.index_checksum() != (0, 0), f"round {j}: the index after the apply is not a fresh build's"
        assert not exp_cpu.any() and not exp_mem.any()
    finally:
        spec.close()
