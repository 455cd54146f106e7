"""Parity of the HIP path (through the C ABI) against the oracle -- the first gate.

Bit-exact (integer/bitmask work): every mask word and every binding must be identical.  Sizes
here are ones the encoded-level oracle finishes in seconds; BASELINE.json's full sizes are
covered by size-independent properties in test_gpu_fullsize.py.
"""
import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (FIT, PICK_BESTFIT, PICK_SAMPLED, SEL, SEL_NEVER, TAINT, WANT_FIT_MASK,
                                             KschedError, _lib, synth, unpack_mask)
from oracle import capi

pytestmark = pytest.mark.gpu

KERNELS = ["direct", "fused"]


def oracle_eval(c, flags, samples=True):
    return capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels if c.n_keys else None,
                             c.node_taints if c.n_taints else None, c.req_cpu, c.req_mem,
                             c.pod_sel if c.n_keys else None, c.pod_tol if c.n_taints else None,
                             c.samples if samples else None, flags)


def hip_eval(ev, c, flags):
    ev.set_nodes(**c.node_columns())
    pc = c.pod_columns()
    return ev.eval(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], pc["samples"], flags)


def check(ev, c, flags):
    r = hip_eval(ev, c, flags)
    feas, fit, bind = oracle_eval(c, flags)
    assert np.array_equal(r.feasible, feas), "feasible mask"
    if flags & WANT_FIT_MASK:
        assert np.array_equal(r.fit, fit), "fit mask"
    if flags & (PICK_SAMPLED | PICK_BESTFIT):
        assert np.array_equal(r.binding, bind), "binding"
    return r


@pytest.mark.parametrize("kernel", KERNELS)
def test_c1_100x20(evaluator, kernel):  # BASELINE.json configs[0]
    evaluator.set_kernel(kernel)
    check(evaluator, synth.make_config("C1"), FIT | SEL | WANT_FIT_MASK | PICK_SAMPLED)
    evaluator.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
def test_c2_10k_x_1k_fit_only(evaluator, kernel):  # BASELINE.json configs[1]
    evaluator.set_kernel(kernel)
    c = synth.make_config("C2")
    r = check(evaluator, c, FIT | PICK_SAMPLED)
    d = unpack_mask(r.feasible, c.N).mean()
    assert 0.05 < d < 0.99
    evaluator.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
def test_c3_reduced_fit_sel(evaluator, kernel):  # configs[2] at a size the oracle does in seconds: 20k x 5k
    evaluator.set_kernel(kernel)
    c = synth.make_config("C3", P=20_000)
    check(evaluator, c, FIT | SEL | WANT_FIT_MASK | PICK_SAMPLED)
    evaluator.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
def test_c5_reduced_taints_bestfit(evaluator, kernel):  # configs[4] shape reduced: 4k x 50k, all predicates
    evaluator.set_kernel(kernel)
    c = synth.make_config("C5", P=4_000)
    check(evaluator, c, FIT | SEL | TAINT | PICK_BESTFIT)
    evaluator.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("P,N", [(1, 1), (1, 64), (64, 1), (63, 65), (65, 63), (129, 1025), (1000, 4097), (257, 16 * 64 + 1)])
def test_ragged_shapes(evaluator, kernel, P, N):
    evaluator.set_kernel(kernel)
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=P * 1000 + N)
    r = check(evaluator, c, FIT | SEL | TAINT | WANT_FIT_MASK | PICK_BESTFIT)
    # padding bits of the last word are zero
    if N % 64:
        assert not (r.feasible[:, -1] >> np.uint64(N % 64)).any()
        assert not (r.fit[:, -1] >> np.uint64(N % 64)).any()
    check(evaluator, c, FIT | SEL | TAINT | PICK_SAMPLED)
    evaluator.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("flags", [FIT, SEL, TAINT, FIT | SEL, FIT | TAINT, SEL | TAINT, FIT | SEL | TAINT, 0])
def test_predicate_subsets(evaluator, kernel, flags):
    """Predicates not selected are treated as true."""
    evaluator.set_kernel(kernel)
    c = synth.make_cluster(300, 700, n_keys=8, n_taints=16, seed=77)
    ev = evaluator
    ev.set_nodes(**c.node_columns())
    pc = c.pod_columns()
    r = ev.eval(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], None, flags)
    feas, _, _ = oracle_eval(c, flags, samples=False)
    assert np.array_equal(r.feasible, feas)
    if flags == 0:
        assert unpack_mask(r.feasible, c.N).all()
    evaluator.set_kernel("auto")


def test_edge_values(evaluator):
    """Extremes of the integer domain: negative available, zero requests, i64 limits, exact fit."""
    i64 = np.iinfo(np.int64)
    avail_cpu = np.array([0, -1, 1, i64.max, i64.min, 1000, 1000, 5], dtype=np.int64)
    avail_mem = np.array([0, 0, -5, i64.max, i64.min, 1 << 40, (1 << 40) - 1, i64.max], dtype=np.int64)
    req_cpu = np.array([0, 1, 1000, i64.max, i64.min, -1, 1001, 5], dtype=np.int64)
    req_mem = np.array([0, 0, 1 << 40, i64.max, i64.min, 1, 0, i64.max], dtype=np.int64)
    ev = evaluator
    ev.set_nodes(avail_cpu, avail_mem)
    for kernel in KERNELS:
        ev.set_kernel(kernel)
        r = ev.eval(req_cpu, req_mem, flags=FIT)
        feas, _, _ = capi.eval_encoded(avail_cpu, avail_mem, None, None, req_cpu, req_mem, None, None, None, capi.FIT)
        assert np.array_equal(r.feasible, feas)
        want = (req_cpu[:, None] <= avail_cpu[None, :]) & (req_mem[:, None] <= avail_mem[None, :])
        assert np.array_equal(unpack_mask(r.feasible, 8), want)
    ev.set_kernel("auto")


def test_selector_semantics_encoded(evaluator):
    """0 = unconstrained, SEL_NEVER never matches, absent label (0) never satisfies a constraint."""
    lab = np.array([[1, 2, 0, 1], [0, 5, 5, 5]], dtype=np.uint32)  # [2 keys][4 nodes]
    big = np.full(4, 1 << 40, dtype=np.int64)
    sel = np.array([[0, 1, 2, 0, SEL_NEVER, 1, 3], [0, 0, 0, 5, 0, 5, 0]], dtype=np.uint32)  # [2][7 pods]
    zero = np.zeros(7, dtype=np.int64)
    want = np.array([[1, 1, 1, 1], [1, 0, 0, 1], [0, 1, 0, 0], [0, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], dtype=bool)
    ev = evaluator
    ev.set_nodes(big, big, lab)
    for kernel in KERNELS:
        ev.set_kernel(kernel)
        r = ev.eval(zero, zero, sel, flags=FIT | SEL)
        assert np.array_equal(unpack_mask(r.feasible, 4), want)
    ev.set_kernel("auto")


@pytest.mark.gpu
def test_result_arrays_kept_from_call_to_call(evaluator):
    """`Evaluator.eval(..., out=previous)`: the host-buffer entry point writes the caller's own result arrays again (bench.py `end_to_end.host_arrays_to_mask`);
    same arrays, new contents == the oracle; a shape that no longer fits gets fresh arrays."""
    ev = evaluator
    c1 = synth.make_cluster(P=700, N=900, n_keys=6, n_taints=0, seed=41)
    ev.set_nodes(**c1.node_columns())
    flags = FIT | SEL | PICK_SAMPLED | WANT_FIT_MASK
    pc = c1.pod_columns()
    r1 = ev.eval(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], None, pc["samples"], flags)
    first = r1.feasible.copy()
    c2 = synth.make_cluster(P=700, N=900, n_keys=6, n_taints=0, seed=42)
    pc2 = c2.pod_columns()  # other pods against the same snapshot
    r2 = ev.eval(pc2["req_cpu_milli"], pc2["req_mem_bytes"], pc2["sel_val_ids"], None, pc2["samples"], flags, out=r1)
    assert r2.feasible is r1.feasible and r2.fit is r1.fit and r2.binding is r1.binding
    feas, fit, bind = capi.eval_encoded(c1.avail_cpu, c1.avail_mem, c1.node_labels, None, c2.req_cpu, c2.req_mem, c2.pod_sel, None, c2.samples, flags)
    assert np.array_equal(r2.feasible, feas) and np.array_equal(r2.fit, fit) and np.array_equal(r2.binding, bind)
    assert not np.array_equal(first, r2.feasible)
    r3 = ev.eval(pc2["req_cpu_milli"][:100], pc2["req_mem_bytes"][:100], np.ascontiguousarray(pc2["sel_val_ids"][:, :100]), None, pc2["samples"][:100], flags, out=r2)
    assert r3.feasible is not r2.feasible and r3.feasible.shape == (100, ev.W) and np.array_equal(r3.feasible, feas[:100]) and np.array_equal(r3.binding, bind[:100])



def test_many_keys_multi_pass(evaluator):
    """More label keys than one pass of the direct kernel handles (8): 19 keys."""
    rng = np.random.default_rng(5)
    N, P, K = 500, 333, 19
    lab = rng.integers(0, 4, size=(K, N), dtype=np.uint32)
    sel = np.where(rng.random((K, P)) < 0.1, rng.integers(1, 4, size=(K, P)), 0).astype(np.uint32)
    cpu = rng.integers(0, 1000, N).astype(np.int64)
    mem = rng.integers(0, 1000, N).astype(np.int64)
    rc = rng.integers(0, 1000, P).astype(np.int64)
    rm = rng.integers(0, 1000, P).astype(np.int64)
    ev = evaluator
    ev.set_nodes(cpu, mem, lab)
    for kernel in KERNELS:
        ev.set_kernel(kernel)
        r = ev.eval(rc, rm, sel, flags=FIT | SEL | WANT_FIT_MASK)
        feas, fit, _ = capi.eval_encoded(cpu, mem, lab, None, rc, rm, sel, None, None, capi.FIT | capi.SEL | capi.WANT_FIT_MASK)
        assert np.array_equal(r.feasible, feas) and np.array_equal(r.fit, fit)
    ev.set_kernel("auto")


def test_empty_inputs(evaluator):
    ev = evaluator
    # zero nodes: empty rows, no binding (reference: choose() on an empty store, src/main.rs:56,70)
    ev.set_nodes(np.zeros(0, np.int64), np.zeros(0, np.int64))
    r = ev.eval(np.zeros(5, np.int64), np.zeros(5, np.int64), samples=np.zeros((5, 5), np.uint32), flags=FIT | PICK_SAMPLED)
    assert r.feasible.shape == (5, 0) and (r.binding == -1).all()
    r = ev.eval(np.zeros(5, np.int64), np.zeros(5, np.int64), flags=FIT | PICK_BESTFIT)
    assert (r.binding == -1).all()
    # zero pods
    ev.set_nodes(np.ones(10, np.int64), np.ones(10, np.int64))
    r = ev.eval(np.zeros(0, np.int64), np.zeros(0, np.int64), flags=FIT)
    assert r.feasible.shape == (0, 1)


def test_error_codes(evaluator):
    ev = evaluator
    ev.set_nodes(np.ones(10, np.int64), np.ones(10, np.int64))
    z = np.zeros(4, np.int64)
    with pytest.raises(KschedError) as e:
        ev.eval(z, z, flags=PICK_SAMPLED | PICK_BESTFIT, samples=np.zeros((4, 5), np.uint32))
    assert e.value.code == _lib.E_INVAL
    with pytest.raises(KschedError) as e:
        ev.eval(z, z, flags=0x1000)
    assert e.value.code == _lib.E_INVAL
    with pytest.raises(KschedError):  # label id equal to the reserved sentinel
        ev.set_nodes(np.ones(2, np.int64), np.ones(2, np.int64), np.array([[SEL_NEVER, 1]], dtype=np.uint32))
    ev.set_nodes(np.ones(10, np.int64), np.ones(10, np.int64))


def test_sampled_pick_semantics(evaluator):
    """D-P1 / D-P3 on the encoded path: first feasible draw wins, draws may repeat, none -> -1."""
    avail = np.array([1, 1, 1, 1, 1, 1, 1, 8], dtype=np.int64) * 1000
    mem = np.full(8, 1 << 30, dtype=np.int64)
    ev = evaluator
    ev.set_nodes(avail, mem)
    rc = np.array([4000, 4000, 500], dtype=np.int64)
    rm = np.array([1, 1, 1], dtype=np.int64)
    samples = np.array([[3, 3, 7, 1, 0], [0, 1, 2, 3, 4], [2, 0, 1, 3, 3]], dtype=np.uint32)
    r = ev.eval(rc, rm, samples=samples, flags=FIT | PICK_SAMPLED)
    assert r.binding.tolist() == [7, -1, 2]
    # an out-of-range draw is an infeasible draw
    samples[0] = [99, 3, 7, 1, 0]
    r = ev.eval(rc, rm, samples=samples, flags=FIT | PICK_SAMPLED)
    assert r.binding.tolist() == [7, -1, 2]


def test_bestfit_semantics(evaluator):
    """Lexicographic (mem residual, cpu residual, node index); ties -> lowest index; none -> -1."""
    cpu = np.array([8000, 4000, 4000, 2000, 9000], dtype=np.int64)
    mem = np.array([100, 50, 50, 10, 50], dtype=np.int64)
    ev = evaluator
    ev.set_nodes(cpu, mem)
    rc = np.array([1000, 3000, 8500, 100, 99999], dtype=np.int64)
    rm = np.array([20, 20, 20, 5, 1], dtype=np.int64)
    r = ev.eval(rc, rm, flags=FIT | PICK_BESTFIT)
    # pod0: feasible {0,1,2,4}: min mem 50 -> {1,2,4}; min cpu 4000 -> {1,2}; lowest index 1
    # pod1: feasible {0,1,2,4} -> 1 ; pod2: only node 4 (cpu 9000 >= 8500, mem 50 >= 20); pod3: node 3 ; pod4: none
    assert r.binding.tolist() == [1, 1, 4, 3, -1]
    _, _, want = capi.eval_encoded(cpu, mem, None, None, rc, rm, None, None, None, capi.FIT | capi.PICK_BESTFIT)
    assert r.binding.tolist() == want.tolist()


def test_bestfit_sparse_rows_fall_back_to_scan(evaluator):
    """Pods whose only feasible nodes sit deep in the best-fit order (beyond the probe window)."""
    N = 3000
    cpu = np.arange(N, dtype=np.int64) + 10
    mem = np.arange(N, dtype=np.int64)[::-1].copy() + 10
    ev = evaluator
    ev.set_nodes(cpu, mem)
    rc = np.array([N + 9, N - 100, 0, N + 10], dtype=np.int64)   # needs the largest cpu = smallest mem ... last in bf order
    rm = np.array([10, 10, N + 9, 10], dtype=np.int64)
    r = ev.eval(rc, rm, flags=FIT | PICK_BESTFIT)
    _, _, want = capi.eval_encoded(cpu, mem, None, None, rc, rm, None, None, None, capi.FIT | capi.PICK_BESTFIT)
    assert r.binding.tolist() == want.tolist()


def test_device_entry_point_matches_host_entry_point(evaluator):
    import torch
    c = synth.make_cluster(3000, 2500, n_keys=8, n_taints=16, seed=31)
    ev = evaluator
    ev.set_nodes(**c.node_columns())
    flags = FIT | SEL | TAINT | WANT_FIT_MASK | PICK_SAMPLED
    pc = c.pod_columns()
    host = ev.eval(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], pc["samples"], flags)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    feas = torch.empty((c.P, ev.W), dtype=torch.int64, device=dev)
    fit = torch.empty((c.P, ev.W), dtype=torch.int64, device=dev)
    bind = torch.empty((c.P,), dtype=torch.int32, device=dev)
    ev.eval_device(t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(c.pod_tol, np.int64),
                   t(c.samples, np.int32), flags, out_feasible=feas, out_fit=fit, out_binding=bind)
    torch.cuda.synchronize()
    assert np.array_equal(feas.cpu().numpy().view(np.uint64), host.feasible)
    assert np.array_equal(fit.cpu().numpy().view(np.uint64), host.fit)
    assert np.array_equal(bind.cpu().numpy(), host.binding)
    # pick without an output mask uses the internal scratch mask
    bind2 = torch.empty((c.P,), dtype=torch.int32, device=dev)
    ev.eval_device(t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(c.pod_tol, np.int64),
                   t(c.samples, np.int32), FIT | SEL | TAINT | PICK_SAMPLED, out_binding=bind2)
    torch.cuda.synchronize()
    assert np.array_equal(bind2.cpu().numpy(), host.binding)


def test_reasons_rebuilt_from_masks(evaluator):
    """check_node_validity's Err order (src/predicates.rs:68-74) from the two masks."""
    c = synth.make_cluster(200, 300, n_keys=8, n_taints=0, seed=41)
    ev = evaluator
    r = hip_eval(ev, c, FIT | SEL | WANT_FIT_MASK)
    feas = unpack_mask(r.feasible, c.N)
    fit = unpack_mask(r.fit, c.N)
    seen = set()
    for p in range(0, c.P, 7):
        for n in range(0, c.N, 11):
            code = ev.reason(r.feasible[p], r.fit[p], n, FIT | SEL)
            want = 0 if feas[p, n] else (1 if not fit[p, n] else 2)
            assert code == want
            seen.add(code)
    assert seen == {0, 1, 2}


def test_explain_separates_selector_from_taint(evaluator):
    """ksched_explain: per-pair reasons decided on the device, in the reference's order (resources, src/predicates.rs:68-70;
    selector, :72-74) then the taint extension -- and, unlike two masks, it tells selector and taint failures apart."""
    ev = evaluator
    c = synth.make_cluster(700, 900, n_keys=8, n_taints=16, seed=0xE8)
    ev.set_kernel("auto")
    ev.set_nodes(**c.node_columns())
    pc = c.pod_columns()
    # three single-predicate oracle masks give the expected reason of every pair
    fit, _, _ = oracle_eval(c, FIT, samples=False)
    sel, _, _ = oracle_eval(c, SEL, samples=False)
    tnt, _, _ = oracle_eval(c, TAINT, samples=False)
    bits = lambda m: unpack_mask(m, c.N)  # noqa: E731
    bf, bs, bt = bits(fit), bits(sel), bits(tnt)
    want = np.where(~bf, _lib.REASON_NOT_ENOUGH_RESOURCES,
                    np.where(~bs, _lib.REASON_NODE_SELECTOR_MISMATCH, np.where(~bt, _lib.REASON_TAINT_NOT_TOLERATED, _lib.REASON_OK)))
    rng = np.random.default_rng(5)
    pp = rng.integers(0, c.P, 20000).astype(np.uint32)
    pn = rng.integers(0, c.N, 20000).astype(np.uint32)
    got = ev.explain(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], pp, pn, FIT | SEL | TAINT)
    assert np.array_equal(got, want[pp, pn])
    assert {1, 2, 3, 0} <= set(np.unique(got).tolist()), "the sample must exercise every reason"
    # predicate subsets: a predicate that is not selected never produces its reason
    got = ev.explain(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], pp, pn, SEL | TAINT)
    want2 = np.where(~bs, _lib.REASON_NODE_SELECTOR_MISMATCH, np.where(~bt, _lib.REASON_TAINT_NOT_TOLERATED, _lib.REASON_OK))
    assert np.array_equal(got, want2[pp, pn])
    with pytest.raises(KschedError):
        ev.explain(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], [c.P], [0], FIT)  # pod out of range


def test_snapshot_replacement(evaluator):
    """set_nodes twice: the second snapshot fully replaces the first (different N and keys)."""
    ev = evaluator
    a = synth.make_cluster(100, 900, n_keys=8, n_taints=16, seed=1)
    b = synth.make_cluster(100, 130, n_keys=3, n_taints=0, seed=2)
    check(ev, a, FIT | SEL | TAINT)
    check(ev, b, FIT | SEL)
    check(ev, a, FIT | SEL | TAINT)


def test_auto_prefers_fused_and_falls_back(evaluator):
    """auto = fused when the snapshot has a bitmap index; keys whose ids are too many / too sparse for one bitmap row per id become
    lists (up to two); only a third such key leaves no index and auto falls back to the direct kernel."""
    ev = evaluator
    ev.set_kernel("auto")
    c = synth.make_cluster(200, 300, n_keys=8, n_taints=16, seed=3)
    check(ev, c, FIT | SEL | TAINT)
    assert ev.last_kernel == "fused"
    rng = np.random.default_rng(1)
    N, P = 300, 100
    big = np.full(N, 1 << 40, dtype=np.int64)
    zero = np.zeros(P, dtype=np.int64)
    for n_sparse, expect in ((2, "fused"), (3, "direct")):
        lab = rng.integers(1, 4_000_000, size=(n_sparse, N)).astype(np.uint32)
        sel = np.zeros((n_sparse, P), dtype=np.uint32)
        sel[0, ::3] = lab[0, rng.integers(0, N, size=len(sel[0, ::3]))]
        sel[n_sparse - 1, ::4] = lab[n_sparse - 1, rng.integers(0, N, size=len(sel[0, ::4]))]
        ev.set_nodes(big, big, lab)
        r = ev.eval(zero, zero, sel, flags=FIT | SEL)
        assert ev.last_kernel == expect
        feas, _, _ = capi.eval_encoded(big, big, lab, None, zero, zero, sel, None, None, capi.FIT | capi.SEL)
        assert np.array_equal(r.feasible, feas)
    ev.set_kernel("fused")
    with pytest.raises(KschedError) as e:
        ev.eval(zero, zero, sel, flags=FIT | SEL)
    assert e.value.code == _lib.E_UNSUPPORTED
    ev.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
def test_duplicate_values_and_ties(evaluator, kernel):
    """Many nodes share the same avail values (ties in the sorted order), pods sit exactly on them."""
    rng = np.random.default_rng(9)
    N, P = 2500, 700
    cpu = rng.choice(np.array([0, 1000, 1000, 2000, 4000, -500], dtype=np.int64), N)
    mem = rng.choice(np.array([0, 1 << 30, 1 << 30, 1 << 31, -1], dtype=np.int64), N)
    rc = rng.choice(np.array([0, 999, 1000, 1001, 2000, 4000, 4001, -500, -501], dtype=np.int64), P)
    rm = rng.choice(np.array([0, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 1 << 31, -1, -2], dtype=np.int64), P)
    ev = evaluator
    ev.set_kernel(kernel)
    ev.set_nodes(cpu, mem)
    r = ev.eval(rc, rm, flags=FIT)
    want = (rc[:, None] <= cpu[None, :]) & (rm[:, None] <= mem[None, :])
    assert np.array_equal(unpack_mask(r.feasible, N), want)
    ev.set_kernel("auto")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("P,N", [(300, 700), (1000, 5000), (129, 1025), (64, 64 * 16)])
def test_pitched_device_masks(evaluator, kernel, P, N):
    """ksched_eval_device_pitched: rows pitch words apart; the [P, W] view equals the packed oracle mask,
    and padding words are zero or untouched (pre-filled sentinel)."""
    import torch
    ev = evaluator
    ev.set_kernel(kernel)
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=P + N)
    ev.set_nodes(**c.node_columns())
    dev = torch.device("cuda", ev.device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    flags = FIT | SEL | TAINT | WANT_FIT_MASK | PICK_BESTFIT
    feas, fit, bind = oracle_eval(c, flags, samples=False)
    for pitched in (True, False):
        m = ev.alloc_mask(P, pitched=pitched)
        f = ev.alloc_mask(P, pitched=pitched)
        sentinel = 0x5A5A5A5A5A5A5A5A
        m.untyped_storage().fill_(0x5A)
        f.untyped_storage().fill_(0x5A)
        b = torch.empty((P,), dtype=torch.int32, device=dev)
        ev.eval_device(t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(c.pod_tol, np.int64), None,
                       flags, out_feasible=m, out_fit=f, out_binding=b)
        torch.cuda.synchronize()
        assert np.array_equal(m.cpu().numpy().view(np.uint64), feas)
        assert np.array_equal(f.cpu().numpy().view(np.uint64), fit)
        assert np.array_equal(b.cpu().numpy(), bind)
        if pitched and m.stride(0) > ev.W:
            full = torch.as_strided(m, (P, m.stride(0)), (m.stride(0), 1))
            pad = full[:, ev.W:].cpu().numpy().view(np.uint64)
            assert np.isin(pad, np.array([0, sentinel], dtype=np.uint64)).all()
    ev.set_kernel("auto")


_CHUNK_RULE = {}


def _chunk_rule_case():
    """One 50-tile cluster for the sizes below and its oracle result, computed once: a pod's mask row and binding depend on that pod alone,
    so the first P pods of the largest batch are the batch of P pods."""
    if not _CHUNK_RULE:
        c = synth.make_cluster(10_241, 50_200, n_keys=8, n_taints=0, seed=50_200)
        flags = FIT | SEL | PICK_SAMPLED
        feas, _, bind = capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels, None, c.req_cpu, c.req_mem, np.ascontiguousarray(c.pod_sel), None,
                                          np.ascontiguousarray(c.samples), flags)
        _CHUNK_RULE.update(c=c, flags=flags, feas=feas, bind=bind)
    return _CHUNK_RULE


@pytest.mark.parametrize("P", [5_120, 5_121, 10_240, 10_241])
def test_chunk_count_rule_at_fifty_tiles(evaluator, P):
    """The chunk-count rule of the fused launch (tile_launch.hpp, fused_geometry) at a size that runs in seconds: 50 200 nodes = 50 tiles, the last
    one partial; a block fills a compute unit, so 5 chunks are resident = 80 streams of 64 pods.  5 120 pods: one round per wave; 5 121: two rounds,
    the rule cuts 5 chunks to 3; 10 240: two rounds, the rule leaves 5; 10 241: three rounds, rule off.  With the rule and with KSCHED_OPT_DEBUG
    bit 31 (the largest resident chunk count): the fused kernel ran, every mask word and binding identical between the two, and == the oracle."""
    import torch
    k = _chunk_rule_case()
    c, flags = k["c"], k["flags"]
    ev = evaluator
    dev = torch.device("cuda", ev.device)
    ev.set_nodes(**c.node_columns())
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    d_cpu, d_mem, d_sel, d_smp = t(c.req_cpu[:P], np.int64), t(c.req_mem[:P], np.int64), t(c.pod_sel[:, :P], np.int32), t(c.samples[:P], np.int32)
    ev.set_kernel("auto")
    out = []
    try:
        for dbg in (0, 0x80000000):
            ev.set_option(_lib.OPT_DEBUG, dbg)
            feas = ev.alloc_mask(P, pitched=True)
            bind = torch.full((P,), -7, dtype=torch.int32, device=dev)
            ev.eval_device(d_cpu, d_mem, d_sel, None, d_smp, flags, out_feasible=feas, out_binding=bind)
            torch.cuda.synchronize()
            assert ev.last_kernel == "fused", ev.last_kernel
            out.append((feas, bind))
    finally:
        ev.set_option(_lib.OPT_DEBUG, 0)
    assert torch.equal(out[0][0], out[1][0]), "the mask differs with the chunk-count rule on / off"
    assert torch.equal(out[0][1], out[1][1]), "the bindings differ with the chunk-count rule on / off"
    for feas, bind in out:
        assert np.array_equal(feas.contiguous().cpu().numpy().view(np.uint64), k["feas"][:P])
        assert np.array_equal(bind.cpu().numpy(), k["bind"][:P])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("count", [1, 7, 200])
def test_update_nodes_matches_fresh_snapshot(evaluator, kernel, count):
    """ksched_update_nodes: patching `available` of some nodes == a fresh ksched_set_nodes
    with the patched columns == the oracle; covers both kernels, both picks, a partial last tile and a node
    listed twice (last value wins)."""
    ev = evaluator
    ev.set_kernel(kernel)
    c = synth.make_cluster(700, 2500, n_keys=8, n_taints=16, seed=1234 + count)
    ev.set_nodes(**c.node_columns())
    rng = np.random.default_rng(count)
    idx = rng.choice(c.N, size=count, replace=False).astype(np.uint32)
    idx[-1] = c.N - 1  # the partial last tile
    # every patched node flips: one that some pod could use becomes over-committed, the others become huge
    old, _, _ = oracle_eval(c, FIT | SEL | TAINT)
    usable = unpack_mask(old, c.N)[:, idx].any(axis=0)
    new_cpu = np.where(usable, -1 - rng.integers(0, 8000, size=count), 1 << 50).astype(np.int64)
    new_mem = np.where(usable, c.avail_mem[idx] - rng.integers(0, 1 << 34, size=count), 1 << 60).astype(np.int64)
    if count > 1:  # duplicate entry: the later one must win
        idx[0] = idx[1]
    ev.update_nodes(idx, new_cpu, new_mem)
    cpu, mem = c.avail_cpu.copy(), c.avail_mem.copy()
    for i, n in enumerate(idx):
        cpu[n], mem[n] = new_cpu[i], new_mem[i]
    pc = c.pod_columns()
    for pick in (PICK_SAMPLED, PICK_BESTFIT):
        flags = FIT | SEL | TAINT | WANT_FIT_MASK | pick
        r = ev.eval(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], pc["samples"], flags)
        feas, fit, bind = capi.eval_encoded(cpu, mem, c.node_labels, c.node_taints, c.req_cpu, c.req_mem, c.pod_sel, c.pod_tol,
                                            c.samples, flags)
        assert np.array_equal(r.feasible, feas) and np.array_equal(r.fit, fit) and np.array_equal(r.binding, bind)
    # and it really changed something
    assert not np.array_equal(old, feas)
    # errors: index out of range, null arrays
    with pytest.raises(KschedError) as e:
        ev.update_nodes(np.array([c.N], np.uint32), np.zeros(1, np.int64), np.zeros(1, np.int64))
    assert e.value.code == _lib.E_INVAL
    ev.set_kernel("auto")


@pytest.mark.parametrize("pick", [PICK_SAMPLED, PICK_BESTFIT])
def test_pick_device_equals_fused_call(evaluator, pick):
    """ksched_pick_device on a mask written by an earlier call == requesting the pick in that call == the oracle."""
    import torch
    ev = evaluator
    c = synth.make_cluster(3000, 2600, n_keys=8, n_taints=16, seed=55)
    ev.set_nodes(**c.node_columns())
    dev = torch.device("cuda", ev.device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    cpu, mem, sel, tol, smp = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(c.pod_tol, np.int64), t(c.samples, np.int32)
    preds = FIT | SEL | TAINT
    _, _, want = oracle_eval(c, preds | pick)
    for pitched in (True, False):
        mask = ev.alloc_mask(c.P, pitched=pitched)
        ev.eval_device(cpu, mem, sel, tol, None, preds, out_feasible=mask)
        b = torch.full((c.P,), -7, dtype=torch.int32, device=dev)
        ev.pick_device(mask, pick | FIT, b, req_mem_bytes=mem, samples=smp if pick == PICK_SAMPLED else None)
        torch.cuda.synchronize()
        assert np.array_equal(b.cpu().numpy(), want)
    with pytest.raises(KschedError) as e:  # both picks / no pick
        ev.pick_device(mask, PICK_SAMPLED | PICK_BESTFIT, b, req_mem_bytes=mem, samples=smp)
    assert e.value.code == _lib.E_INVAL


@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_steps_equal_sequential(evaluator, depth):
    """PipelinedScheduler over a ksched_pipe on the GPU: mask kernel of step i+1 on one stream, pick of step i on another,
    `depth` slots.  Every step is a different batch (pods rotate); every step's bindings == the oracle for that batch."""
    import torch
    from kube_scheduler_rs_reference_amd.dist import PipelinedScheduler
    ev = evaluator
    c = synth.make_cluster(5000, 3000, n_keys=8, n_taints=0, seed=77)
    ev.set_nodes(**c.node_columns())
    dev = torch.device("cuda", ev.device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    steps = 6
    rolled = [np.roll(np.arange(c.P), 37 * j) for j in range(steps)]
    batches = [dict(cpu=t(c.req_cpu[r], np.int64), mem=t(c.req_mem[r], np.int64), sel=t(c.pod_sel[:, r], np.int32),
                    smp=t(c.samples[r], np.int32)) for r in rolled]
    torch.cuda.synchronize()
    pipe = ev.pipe(depth)
    sched = PipelinedScheduler(c.P, dev, depth=depth, pipe=pipe)
    masks = [ev.alloc_mask(c.P) for _ in range(depth)]

    def run(slot, out):
        b = batches[state["j"]]
        pipe.submit(slot, b["cpu"], b["mem"], b["sel"], None, b["smp"], FIT | SEL | PICK_SAMPLED, masks[slot], out)

    state = {"j": 0}
    got = []
    pend = []
    for j in range(steps):
        state["j"] = j
        pend.append(sched.step(run))
        if len(pend) >= depth:
            got.append(pend.pop(0).wait().clone())
    got += [p.wait().clone() for p in pend]
    sched.drain()
    torch.cuda.synchronize()
    _, _, base = oracle_eval(c, FIT | SEL | PICK_SAMPLED)
    for j in range(steps):
        assert np.array_equal(got[j].cpu().numpy(), base[rolled[j]]), f"step {j}"
    # the masks of the last `depth` steps are still in their slots and equal the oracle's
    feas, _, _ = oracle_eval(c, FIT | SEL)
    for j in range(steps - depth, steps):
        assert np.array_equal(masks[j % depth].cpu().numpy().view(np.uint64), feas[rolled[j]]), f"mask of step {j}"
    pipe.close()


@pytest.mark.parametrize("two_stream,every", [(False, 1), (True, 1), (False, 3), (True, 3)])
def test_pipelined_allgather_over_rccl_one_rank(evaluator, two_stream, every):
    """The N > 1 code path on the one GPU there is: a one-rank "nccl" (= RCCL) process group, asynchronous
    all_gather_into_tensor behind the pick (on the pipe's pick stream when two_stream), slots reused over 6 steps."""
    import socket
    import torch
    import torch.distributed as dist
    from kube_scheduler_rs_reference_amd.dist import PipelinedScheduler
    ev = evaluator
    c = synth.make_cluster(4000, 2100, n_keys=8, n_taints=0, seed=91)
    ev.set_nodes(**c.node_columns())
    dev = torch.device("cuda", ev.device)
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
        steps, depth = 6, 2
        rolled = [np.roll(np.arange(c.P), 11 * j) for j in range(steps)]
        batches = [dict(cpu=t(c.req_cpu[r], np.int64), mem=t(c.req_mem[r], np.int64), sel=t(c.pod_sel[:, r], np.int32),
                        smp=t(c.samples[r], np.int32)) for r in rolled]
        torch.cuda.synchronize()
        pipe = ev.pipe(depth * every) if two_stream else None  # one pipe slot per step in flight
        sched = PipelinedScheduler(c.P, dev, depth=depth, pipe=pipe, gather_always=True, gather_every=every)
        masks = [ev.alloc_mask(c.P) for _ in range(depth * every)]
        state = {"j": 0}

        def run(slot, out):
            b = batches[state["j"]]
            if pipe is not None:
                pipe.submit(slot, b["cpu"], b["mem"], b["sel"], None, b["smp"], FIT | SEL | PICK_SAMPLED, masks[slot], out)
            else:
                ev.eval_device(b["cpu"], b["mem"], b["sel"], None, b["smp"], FIT | SEL | PICK_SAMPLED, out_feasible=masks[0], out_binding=out)

        got, pend = [], []
        for j in range(steps):
            state["j"] = j
            pend.append(sched.step(run))
            if len(pend) >= (depth - 1) * every + 1:
                got.append(pend.pop(0).wait().clone())
        got += [p.wait().clone() for p in pend]
        sched.drain()
        torch.cuda.synchronize()
        _, _, base = oracle_eval(c, FIT | SEL | PICK_SAMPLED)
        for j in range(steps):
            assert np.array_equal(got[j].cpu().numpy(), base[rolled[j]]), f"step {j}"
        if pipe is not None:
            pipe.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("two_stream,every", [(False, 1), (True, 1), (True, 3), (False, 2)])
def test_pipelined_allgather_through_the_c_abi_one_rank(evaluator, two_stream, every):
    """The N > 1 data path with the C ABI's own RCCL communicator (AbiComm = ksched_comm_create + ksched_allgather_bindings):
    no torch.distributed process group exists in this test at all.  Slots reused over 7 steps, gather groups of 1 / 2 / 3."""
    import torch
    from kube_scheduler_rs_reference_amd.dist import AbiComm, PipelinedScheduler, ShardedScheduler
    ev = evaluator
    c = synth.make_cluster(4000, 2100, n_keys=8, n_taints=0, seed=92)
    ev.set_kernel("auto")
    ev.set_nodes(**c.node_columns())
    dev = torch.device("cuda", ev.device)
    comm = AbiComm(ev)
    assert (comm.rank, comm.world) == (0, 1)
    try:
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
        steps, depth = 7, 2
        rolled = [np.roll(np.arange(c.P), 13 * j) for j in range(steps)]
        batches = [dict(cpu=t(c.req_cpu[r], np.int64), mem=t(c.req_mem[r], np.int64), sel=t(c.pod_sel[:, r], np.int32),
                        smp=t(c.samples[r], np.int32)) for r in rolled]
        torch.cuda.synchronize()
        pipe = ev.pipe(depth * every) if two_stream else None
        sched = PipelinedScheduler(c.P, dev, depth=depth, pipe=pipe, gather_always=True, gather_every=every, comm=comm)
        masks = [ev.alloc_mask(c.P) for _ in range(depth * every)]
        state = {"j": 0}

        def run(slot, out):
            b = batches[state["j"]]
            if pipe is not None:
                pipe.submit(slot, b["cpu"], b["mem"], b["sel"], None, b["smp"], FIT | SEL | PICK_SAMPLED, masks[slot], out)
            else:
                ev.eval_device(b["cpu"], b["mem"], b["sel"], None, b["smp"], FIT | SEL | PICK_SAMPLED, out_feasible=masks[0], out_binding=out)

        got, pend = [], []
        for j in range(steps):
            state["j"] = j
            pend.append(sched.step(run))
            if len(pend) >= (depth - 1) * every + 1:
                got.append(pend.pop(0).wait().clone())
        got += [p.wait().clone() for p in pend]
        sched.drain()
        torch.cuda.synchronize()
        _, _, base = oracle_eval(c, FIT | SEL | PICK_SAMPLED)
        for j in range(steps):
            assert np.array_equal(got[j].cpu().numpy(), base[rolled[j]]), f"step {j}"
        # the sequential form through the same communicator
        seq = ShardedScheduler(c.P, dev, comm=comm)
        b = batches[0]
        out = seq.step(lambda o: ev.eval_device(b["cpu"], b["mem"], b["sel"], None, b["smp"], FIT | SEL | PICK_SAMPLED, out_feasible=masks[0], out_binding=o))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), base[rolled[0]])
        if pipe is not None:
            pipe.close()
    finally:
        comm.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_sampled_pick_direct_equals_pick_from_mask(evaluator, kernel):
    """KSCHED_PICK_SAMPLED two ways: candidates tested straight from the columns (default; the reference's own order of
    work, src/main.rs:53-66) and candidates' bits read back from the mask (KSCHED_OPT_PICK_FROM_MASK) -- both == oracle,
    with taints, > 8 label keys, out-of-range draws, more than 5 and more than 8 attempts, and bindings-only requests."""
    ev = evaluator
    ev.set_kernel(kernel)
    rng = np.random.default_rng(17)
    for (P, N, K, attempts) in [(2000, 1500, 8, 5), (700, 900, 13, 5), (500, 300, 8, 11), (300, 64, 3, 1), (64, 2000, 8, 8)]:
        c = synth.make_cluster(P, N, n_keys=min(K, 8), n_taints=16, seed=P + K)
        lab, sel = c.node_labels, c.pod_sel
        if K > 8:  # extra keys beyond the generator's eight
            lab = np.concatenate([lab, rng.integers(0, 3, size=(K - 8, N), dtype=np.uint32)])
            sel = np.concatenate([sel, np.where(rng.random((K - 8, P)) < 0.2, rng.integers(1, 4, size=(K - 8, P)), 0).astype(np.uint32)])
        samples = rng.integers(0, N + 3, size=(P, attempts), dtype=np.uint32)  # a few draws are out of range = infeasible
        ev.set_nodes(c.avail_cpu, c.avail_mem, lab, c.node_taints)
        flags = FIT | SEL | TAINT | PICK_SAMPLED
        _, _, want = capi.eval_encoded(c.avail_cpu, c.avail_mem, lab, c.node_taints, c.req_cpu, c.req_mem, sel, c.pod_tol, samples, flags)
        for from_mask in (0, 1):  # candidates tested from the columns / candidates' bits read back from the mask
            ev.set_option(_lib.OPT_PICK_FROM_MASK, from_mask)
            r = ev.eval(c.req_cpu, c.req_mem, sel, c.pod_tol, samples, flags)
            assert np.array_equal(r.binding, want), (P, N, K, attempts, from_mask)
            feas, _, _ = capi.eval_encoded(c.avail_cpu, c.avail_mem, lab, c.node_taints, c.req_cpu, c.req_mem, sel, c.pod_tol, None, FIT | SEL | TAINT)
            assert np.array_equal(r.feasible, feas)
            r2 = ev.eval(c.req_cpu, c.req_mem, sel, c.pod_tol, samples, flags, want_mask=False)  # bindings only
            assert r2.feasible is None and np.array_equal(r2.binding, want)
        # predicate subsets reach the select kernel too
        ev.set_option(_lib.OPT_PICK_FROM_MASK, 0)
        for sub in (FIT, SEL, TAINT, FIT | TAINT, 0):
            _, _, w2 = capi.eval_encoded(c.avail_cpu, c.avail_mem, lab, c.node_taints, c.req_cpu, c.req_mem, sel, c.pod_tol, samples, sub | PICK_SAMPLED)
            r = ev.eval(c.req_cpu, c.req_mem, sel, c.pod_tol, samples, sub | PICK_SAMPLED, want_mask=False)
            assert np.array_equal(r.binding, w2), (P, N, K, attempts, sub)
    ev.set_option(_lib.OPT_PICK_FROM_MASK, 0)
    ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)
    ev.set_kernel("auto")


@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("kernel", KERNELS)
def test_bestfit_direct_equals_bestfit_from_mask(evaluator, kernel, stages):
    """KSCHED_PICK_BESTFIT two ways: first set bit of the AND of bitmaps kept in best-fit order (default, no mask read) and
    every candidate's bit looked up in the mask (KSCHED_OPT_PICK_FROM_MASK) -- both == oracle; with taints, > 8 label keys, predicate subsets, rows whose only feasible nodes sit beyond the direct window,
    and after ksched_update_nodes (the order changes)."""
    ev = evaluator
    ev.set_kernel(kernel)
    ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)  # 1: a wave per pod; 2: a lane per pod first (the default only from 24576 pods on)
    rng = np.random.default_rng(23)
    for (P, N, K) in [(1500, 6000, 8), (600, 2500, 12), (200, 100, 3), (64, 1, 8)]:
        c = synth.make_cluster(P, N, n_keys=min(K, 8), n_taints=16, seed=3 * P + K)
        lab, sel = c.node_labels, c.pod_sel
        if K > 8:
            lab = np.concatenate([lab, rng.integers(0, 3, size=(K - 8, N), dtype=np.uint32)])
            sel = np.concatenate([sel, np.where(rng.random((K - 8, P)) < 0.2, rng.integers(1, 4, size=(K - 8, P)), 0).astype(np.uint32)])
        cpu, mem = c.avail_cpu.copy(), c.avail_mem.copy()
        req_cpu = c.req_cpu.copy()
        req_cpu[::7] = np.sort(cpu)[-max(1, N // 400)]  # these pods fit only the few largest nodes: deep in the best-fit order
        ev.set_nodes(cpu, mem, lab, c.node_taints)
        for step in range(2):
            for flags in (FIT | SEL | TAINT, FIT, SEL | TAINT, FIT | SEL):
                _, _, want = capi.eval_encoded(cpu, mem, lab, c.node_taints, req_cpu, c.req_mem, sel, c.pod_tol, None, flags | PICK_BESTFIT)
                for from_mask in (0, 1):
                    ev.set_option(_lib.OPT_PICK_FROM_MASK, from_mask)
                    r = ev.eval(req_cpu, c.req_mem, sel, c.pod_tol, None, flags | PICK_BESTFIT)
                    assert np.array_equal(r.binding, want), (P, N, K, flags, from_mask, step)
                    r = ev.eval(req_cpu, c.req_mem, sel, c.pod_tol, None, flags | PICK_BESTFIT, want_mask=False)  # bindings only
                    assert np.array_equal(r.binding, want), (P, N, K, flags, from_mask, step, "no mask")
            # a few nodes change: the best-fit order and the columns kept in that order are rebuilt
            idx = rng.choice(N, size=min(N, 9), replace=False).astype(np.uint32)
            cpu[idx] = rng.integers(0, 200_000, size=idx.size)
            mem[idx] = rng.integers(0, 1 << 38, size=idx.size)
            ev.set_option(_lib.OPT_PICK_FROM_MASK, 0)
            ev.update_nodes(idx, cpu[idx], mem[idx])
    ev.set_option(_lib.OPT_PICK_FROM_MASK, 0)
    ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)
    ev.set_kernel("auto")


def test_pipe_wait_mask_orders_a_consumer_stream(evaluator):
    """ksched_pipe_wait_mask: the pick does not read the mask, so the pipe's two streams are unordered and a finished pick says
    nothing about the mask kernel.  A consumer stream ordered by wait_mask (and a host wait) sees the complete mask == oracle."""
    import torch
    ev = evaluator
    c = synth.make_cluster(30000, 5000, n_keys=8, n_taints=0, seed=505)
    ev.set_nodes(**c.node_columns())
    dev = torch.device("cuda", ev.device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    cpu, mem, sel, smp = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(c.samples, np.int32)
    feas, _, bind = oracle_eval(c, FIT | SEL | PICK_SAMPLED)
    pipe = ev.pipe(2)
    masks = [ev.alloc_mask(c.P) for _ in range(2)]
    outs = [torch.empty((c.P,), dtype=torch.int32, device=dev) for _ in range(2)]
    consumer = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for rep in range(3):
        slot = rep % 2
        masks[slot].zero_()
        torch.cuda.synchronize()
        pipe.submit(slot, cpu, mem, sel, None, smp, FIT | SEL | PICK_SAMPLED, masks[slot], outs[slot])
        pipe.wait_mask(slot, stream=consumer)
        pipe.wait(slot, stream=consumer)
        with torch.cuda.stream(consumer):
            m_copy, b_copy = masks[slot].clone(), outs[slot].clone()
        consumer.synchronize()  # only the consumer: the pipe's streams are not touched by the host
        assert np.array_equal(m_copy.cpu().numpy().view(np.uint64), feas), rep
        assert np.array_equal(b_copy.cpu().numpy(), bind), rep
    masks[0].zero_()
    torch.cuda.synchronize()
    pipe.submit(0, cpu, mem, sel, None, smp, FIT | SEL | PICK_SAMPLED, masks[0], outs[0])
    pipe.wait_mask(0, host=True)
    assert np.array_equal(masks[0].cpu().numpy().view(np.uint64), feas)
    pipe.close()


def test_evaluations_on_two_streams_share_the_ctx_scratch(evaluator):
    """Two caller streams alternate bindings-only best-fit evaluations (two stages: the hand-over lists live in ctx-owned scratch)
    and fit-mask-only evaluations (the feasible mask goes to a ctx-owned scratch mask): the library orders the streams' use of
    that memory itself.  Every result == oracle; then one stream is forgotten and destroyed and the other carries on."""
    import torch
    ev = evaluator
    ev.set_option(_lib.OPT_BESTFIT_STAGES, 2)
    c = synth.make_cluster(20000, 6000, n_keys=8, n_taints=16, seed=811)
    ev.set_nodes(**c.node_columns())
    dev = torch.device("cuda", ev.device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    flags = FIT | SEL | TAINT
    rolled = [np.roll(np.arange(c.P), 101 * j) for j in range(6)]
    batches = [dict(cpu=t(c.req_cpu[r], np.int64), mem=t(c.req_mem[r], np.int64), sel=t(c.pod_sel[:, r], np.int32),
                    tol=t(c.pod_tol[r], np.int64)) for r in rolled]
    _, fit, want = oracle_eval(c, flags | PICK_BESTFIT | _lib.WANT_FIT_MASK)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    outs = [torch.empty((c.P,), dtype=torch.int32, device=dev) for _ in rolled]
    fits = [ev.alloc_mask(c.P) for _ in rolled]
    torch.cuda.synchronize()
    for j, b in enumerate(batches):  # no host wait in between: the kernels of consecutive calls are in flight together
        s = streams[j % 2]
        ev.eval_device(b["cpu"], b["mem"], b["sel"], b["tol"], None, flags | PICK_BESTFIT, out_binding=outs[j], stream=s)
        ev.eval_device(b["cpu"], b["mem"], b["sel"], b["tol"], None, flags | _lib.WANT_FIT_MASK, out_fit=fits[j], stream=streams[(j + 1) % 2])
    torch.cuda.synchronize()
    for j, r in enumerate(rolled):
        assert np.array_equal(outs[j].cpu().numpy(), want[r]), f"bindings of call {j}"
        assert np.array_equal(fits[j].cpu().numpy().view(np.uint64), fit[r]), f"fit mask of call {j}"
    # the stream that used the scratch last goes away (ksched_forget_stream first, as the header asks); the other one carries on
    ev.eval_device(batches[0]["cpu"], batches[0]["mem"], batches[0]["sel"], batches[0]["tol"], None, flags | PICK_BESTFIT, out_binding=outs[0], stream=streams[1])
    ev.forget_stream(streams[1])
    del streams[1]
    ev.eval_device(batches[1]["cpu"], batches[1]["mem"], batches[1]["sel"], batches[1]["tol"], None, flags | PICK_BESTFIT, out_binding=outs[1], stream=streams[0])
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), want[rolled[0]]) and np.array_equal(outs[1].cpu().numpy(), want[rolled[1]])
    ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)


def test_eval_in_two_halves_equals_ksched_eval(evaluator):
    """ABI 4: ksched_eval_begin (copies in + evaluation enqueued, bindings left on the device, padded with -1) + ksched_eval_end (one copy,
    one wait) == ksched_eval, for a shard addressed INSIDE a larger batch (selector columns with the whole batch's stride), with and without
    masks, and for an empty shard (p = 0: `capacity` rows of -1)."""
    import ctypes as C
    from kube_scheduler_rs_reference_amd import _lib as L
    c = synth.make_config("C3", P=3000, N=700)
    ev = evaluator
    ev.set_nodes(**c.node_columns())
    lib, h = ev._lib, ev._h
    flags = FIT | SEL | PICK_SAMPLED
    W = ev.W
    want_feas, want_fit, want_b = capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels, None, c.req_cpu, c.req_mem, c.pod_sel, None, c.samples, flags | WANT_FIT_MASK)
    P, K = c.P, c.n_keys
    sel = np.ascontiguousarray(c.pod_sel, dtype=np.uint32)
    smp = np.ascontiguousarray(c.samples, dtype=np.uint32)
    cpu, mem = np.ascontiguousarray(c.req_cpu, dtype=np.int64), np.ascontiguousarray(c.req_mem, dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for lo, hi, masks in ((0, P, True), (700, 1811, True), (1811, P, False), (5, 5, False)):
        p = hi - lo
        cap = p + 37
        feas = np.full((max(p, 1), W), 0xAB, dtype=np.uint64)
        fit = np.full((max(p, 1), W), 0xCD, dtype=np.uint64)
        dev_b, stream = C.c_void_p(), C.c_void_p()
        rc = lib.ksched_eval_begin(h, p, C.c_void_p(cpu.ctypes.data + 8 * lo), C.c_void_p(mem.ctypes.data + 8 * lo), C.c_void_p(sel.ctypes.data + 4 * lo), P, None,
                                   C.c_void_p(smp.ctypes.data + 4 * 5 * lo), 5, flags | (WANT_FIT_MASK if masks else 0), vp(feas) if masks else None,
                                   vp(fit) if masks else None, cap, C.byref(dev_b), C.byref(stream))
        assert rc == 0, lib.ksched_last_error(h)
        assert dev_b.value and stream.value
        got = np.full((cap,), 12345, dtype=np.int32)
        assert lib.ksched_eval_end(h, dev_b, cap, vp(got)) == 0
        assert np.array_equal(got[:p], want_b[lo:hi]) and (got[p:] == -1).all(), (lo, hi)
        if masks:
            assert np.array_equal(feas[:p], want_feas[lo:hi]) and np.array_equal(fit[:p], want_fit[lo:hi])
    # a selector stride shorter than the shard is refused; so is a pick with nowhere to go
    dev_b, stream = C.c_void_p(), C.c_void_p()
    assert lib.ksched_eval_begin(h, 10, vp(cpu), vp(mem), vp(sel), 9, None, vp(smp), 5, flags, None, None, 10, C.byref(dev_b), C.byref(stream)) == L.E_INVAL
    assert lib.ksched_eval_begin(h, 10, vp(cpu), vp(mem), vp(sel), P, None, vp(smp), 5, flags, None, None, 10, None, C.byref(stream)) == L.E_INVAL
    g = C.c_void_p()
    assert lib.ksched_gather_buffer(h, 4096, C.byref(g)) == 0 and g.value
    g2 = C.c_void_p()
    assert lib.ksched_gather_buffer(h, 100, C.byref(g2)) == 0 and g2.value == g.value  # grown on demand, reused


@pytest.mark.parametrize("N,distinct", [(1025, 3), (2049, 7), (3001, 7), (5000, 2), (4097, 4097)])
def test_bestfit_orders_with_ragged_sizes_and_duplicate_keys(evaluator, N, distinct):
    """the best-fit structures' two orders come from the hand-written merge sort (k_sort_runs + k_merge_pass).  Node counts that are not
    a multiple of a run (1024) and `available` columns with only a handful of distinct values -- long runs of equal (mem, cpu) keys, ordered by the
    node index alone -- must give the oracle's best-fit binding for every pod (the tie-break IS the order), one stage and two stages."""
    from kube_scheduler_rs_reference_amd import PICK_BESTFIT
    ev = evaluator
    r = np.random.default_rng(N * 31 + distinct)
    vals_c = r.integers(500, 9000, distinct).astype(np.int64)
    vals_m = r.integers(1 << 20, 1 << 34, distinct).astype(np.int64)
    pick = r.integers(0, distinct, N)
    cpu, mem = vals_c[pick], vals_m[r.integers(0, distinct, N)]
    P = 30_000
    rc = r.integers(100, 9500, P).astype(np.int64)
    rm = r.integers(1 << 19, 1 << 34, P).astype(np.int64)
    ev.set_nodes(cpu, mem, None, None)
    want = capi.eval_encoded(cpu, mem, None, None, rc, rm, None, None, None, FIT | PICK_BESTFIT)
    try:
        for stages in (1, 2):
            ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)
            got = ev.eval(rc, rm, None, None, None, FIT | PICK_BESTFIT)
            assert np.array_equal(got.binding, want[2]), stages
            assert np.array_equal(got.feasible, want[0])
    finally:
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)


@pytest.mark.parametrize("P,N", [(1, 1), (300, 70), (2000, 1500), (40_000, 3000)])
def test_pick_from_host_masks_equals_the_pick_of_the_evaluation(evaluator, P, N):
    """ksched_pick (host-pointer twin of ksched_pick_device, new in ABI 5): the sampled and the best-fit pick from masks the HOST holds -- what the
    mirror uses for a pod whose selector needs more than one call (the groups' masks ANDed on the host, the pick by the device).  From the masks an
    evaluation returned it must give that evaluation's bindings; from an ANDed pair of masks the bindings of the conjunction (oracle)."""
    ev = evaluator
    c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=P * 13 + N)
    ev.set_nodes(**c.node_columns())
    for pick in (PICK_SAMPLED, PICK_BESTFIT):
        want = oracle_eval(c, FIT | SEL | pick)
        got = ev.eval(c.req_cpu, c.req_mem, c.pod_sel, None, c.samples if pick == PICK_SAMPLED else None, FIT | SEL | pick)
        assert np.array_equal(got.binding, want[2]) and np.array_equal(got.feasible, want[0])
        again = ev.pick(got.feasible, FIT | SEL | pick, req_mem_bytes=c.req_mem, samples=c.samples if pick == PICK_SAMPLED else None)
        assert np.array_equal(again, want[2]), pick
        # the conjunction of two half-selectors: masks of keys 0..3 and of keys 4..7, ANDed on the host
        lo, hi = c.pod_sel.copy(), c.pod_sel.copy()
        lo[4:], hi[:4] = 0, 0
        m_lo = ev.eval(c.req_cpu, c.req_mem, lo, None, None, FIT | SEL).feasible
        m_hi = ev.eval(c.req_cpu, c.req_mem, hi, None, None, FIT | SEL).feasible
        both = ev.pick(m_lo & m_hi, FIT | SEL | pick, req_mem_bytes=c.req_mem, samples=c.samples if pick == PICK_SAMPLED else None)
        assert np.array_equal(m_lo & m_hi, want[0]) and np.array_equal(both, want[2]), pick
    with pytest.raises(KschedError):
        ev.pick(np.zeros((P, ev.W), dtype=np.uint64), PICK_SAMPLED | PICK_BESTFIT, samples=c.samples)
    with pytest.raises(KschedError):
        ev.pick(np.zeros((P, ev.W), dtype=np.uint64), FIT, samples=c.samples)
