"""ksched_apply_bindings_device / ksched_read_nodes (ABI 7) on the MI355X.

Every expected column and status comes from `restate` (oracle/oracle_ref.py apply_bindings_exact) -- a plain restatement with exact
Python integers of the rule the header states (SubAssign, src/util.rs:31-36, over the eligible accepted pods) -- and every expected mask
and binding from the oracle (capi.eval_encoded) on those columns.  The index after an apply is compared with a fresh ksched_set_nodes of
the expected columns.
"""
import numpy as np
import pytest
import torch

from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, PICK_SAMPLED, SEL, TAINT, Evaluator, KschedError, _lib, synth
from oracle import capi
from oracle.oracle_ref import apply_bindings_exact as restate  # (tests/apply_sharded_worker.py imports it from here too)

pytestmark = pytest.mark.gpu
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DEV = torch.device("cuda:0")


def t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


@pytest.fixture(scope="module")
def ev(built):
    e = Evaluator(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref(built):
    """a second ctx: the fresh ksched_set_nodes whose index an applied snapshot must equal"""
    e = Evaluator(0)
    yield e
    e.close()


def fresh_checksum(ref, cols, cpu, mem):
    ref.set_nodes(cpu, mem, cols["label_val_ids"], cols["taints"])
    return ref.index_checksum()


def apply(ev, bindings, req_cpu, req_mem, ok=None, flags=0):
    st = torch.full((len(bindings),), -7, dtype=torch.int32, device=DEV)
    ev.apply_bindings_device(t(bindings, np.int32), t(req_cpu, np.int64), t(req_mem, np.int64), None if ok is None else t(ok, np.uint8),
                             flags, st)
    torch.cuda.current_stream().synchronize()
    return st.cpu().numpy()


def random_bindings(rng, n, p):
    b = rng.integers(0, n, p).astype(np.int32)
    b[rng.random(p) < 0.1] = -1
    b[rng.random(p) < 0.05] = 0 if n == 1 else int(rng.integers(0, n))  # many pods onto one node
    b[rng.random(p) < 0.01] = n + int(rng.integers(0, 5))  # past the last node
    ok = (rng.random(p) > 0.1).astype(np.uint8)
    return b, ok


@pytest.mark.parametrize("N", [1, 1024, 1025, 5000, 50_000])
@pytest.mark.parametrize("flags", [0, _lib.APPLY_FIRST_PER_NODE], ids=["all", "first-per-node"])
def test_round_trip(ev, ref, N, flags):
    P = min(max(3 * N + 7, 500), 60_000)
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=0xA9 + N)
    cols = c.node_columns()
    ev.set_nodes(**cols)
    rng = np.random.default_rng(N + flags)
    b, ok = random_bindings(rng, N, P)
    st = apply(ev, b, c.req_cpu, c.req_mem, ok, flags)
    cpu, mem, want = restate(c.avail_cpu, c.avail_mem, b, c.req_cpu, c.req_mem, ok, flags)
    got_cpu, got_mem = ev.read_nodes()
    assert np.array_equal(got_cpu, cpu) and np.array_equal(got_mem, mem)
    assert np.array_equal(st, want)
    assert (want == _lib.APPLY_APPLIED).any() and (want == _lib.APPLY_UNBOUND).any() and (want == _lib.APPLY_NOT_OK).any()
    assert ev.index_checksum() == fresh_checksum(ref, cols, cpu, mem)
    lo = N // 3
    sub = ev.read_nodes(lo, N - lo)
    assert np.array_equal(sub[0], cpu[lo:]) and np.array_equal(sub[1], mem[lo:])


def test_first_per_node_accepts_exactly_the_lowest_eligible_pod(ev):
    N, P = 300, 5000
    c = synth.make_cluster(P, N, n_keys=0, seed=77)
    ev.set_nodes(**c.node_columns())
    rng = np.random.default_rng(5)
    b, ok = random_bindings(rng, N, P)
    st = apply(ev, b, c.req_cpu, c.req_mem, ok, _lib.APPLY_FIRST_PER_NODE)
    for node in range(N):
        elig = np.nonzero((b == node) & (ok != 0))[0]
        if len(elig):
            assert st[elig[0]] == _lib.APPLY_APPLIED
            assert (st[elig[1:]] == _lib.APPLY_DEFERRED).all()
    assert (st == _lib.APPLY_DEFERRED).sum() > 1000


def sequential_rule(bindings):
    """reconcile_batch_sequential's rule for one round, every POST landing: per node the first pod of the round; later ones retry"""
    taken, accepted, deferred = set(), [], []
    for j, b in enumerate(bindings.tolist()):
        if b < 0:
            continue
        if b in taken:
            deferred.append(j)
        else:
            taken.add(b)
            accepted.append(j)
    return accepted, deferred


def test_no_over_commit_rounds_match_the_sequential_rule(ev):
    """rounds of [sampled pick on the device -> apply FIRST_PER_NODE -> retry the DEFERRED pods] against the same rounds restated on the host
    (the oracle's picks on the host's columns, the sequential rule, SubAssign)"""
    N, P = 400, 6000
    c = synth.make_cluster(P, N, n_keys=8, seed=99)
    cols = c.node_columns()
    ev.set_nodes(**cols)
    rng = np.random.default_rng(11)
    flags = FIT | SEL | PICK_SAMPLED
    cpu, mem = c.avail_cpu.copy(), c.avail_mem.copy()
    pending = np.arange(P)
    accepted_dev, accepted_host = set(), set()
    for _ in range(6):
        if len(pending) == 0:
            break
        smp = rng.integers(0, N, (len(pending), 5)).astype(np.uint32)
        rc, rm, sel = c.req_cpu[pending], c.req_mem[pending], np.ascontiguousarray(c.pod_sel[:, pending])
        rc_t, rm_t = t(rc, np.int64), t(rm, np.int64)
        outb = torch.empty((len(pending),), dtype=torch.int32, device=DEV)
        st = torch.empty_like(outb)
        ev.eval_device(rc_t, rm_t, t(sel, np.int32), None, t(smp, np.int32), flags, out_binding=outb)
        ev.apply_bindings_device(outb, rc_t, rm_t, flags=_lib.APPLY_FIRST_PER_NODE, status_out=st)
        b_dev, st = outb.cpu().numpy(), st.cpu().numpy()
        # the host's round
        b_host = capi.eval_encoded(cpu, mem, c.node_labels, None, rc, rm, sel, None, smp, flags, want_mask=False)[2]
        assert np.array_equal(b_dev, b_host)
        acc, dfr = sequential_rule(b_host)
        cpu, mem, _ = restate(cpu, mem, np.where(np.isin(np.arange(len(pending)), acc), b_host, -1), rc, rm)
        assert sorted(np.nonzero(st == _lib.APPLY_APPLIED)[0].tolist()) == acc
        assert sorted(np.nonzero(st == _lib.APPLY_DEFERRED)[0].tolist()) == dfr
        accepted_dev |= set(pending[st == _lib.APPLY_APPLIED].tolist())
        accepted_host |= set(pending[acc].tolist())
        pending = pending[dfr]
    assert accepted_dev == accepted_host and len(accepted_host) > N // 2
    got = ev.read_nodes()
    assert np.array_equal(got[0], cpu) and np.array_equal(got[1], mem)


def test_eval_apply_eval_on_one_stream_at_c3(built):
    """five steps of [eval_device (mask + sampled pick) -> apply_bindings_device] on one torch stream, no host sync in between: every
    step's mask (every word) and bindings equal the oracle on the columns the steps before it left"""
    c = synth.make_config("C3")
    flags = FIT | SEL | PICK_SAMPLED
    rng = np.random.default_rng(3)
    steps = 5
    samples = [rng.integers(0, c.N, (c.P, 5)).astype(np.uint32) for _ in range(steps)]
    with Evaluator(0) as e:
        e.set_nodes(**c.node_columns())
        rc_t, rm_t, sel_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32)
        smp_t = [t(s, np.int32) for s in samples]
        masks = [torch.empty((c.P, e.W), dtype=torch.int64, device=DEV) for _ in range(steps)]
        binds = [torch.empty((c.P,), dtype=torch.int32, device=DEV) for _ in range(steps)]
        torch.cuda.synchronize()
        for k in range(steps):
            e.eval_device(rc_t, rm_t, sel_t, None, smp_t[k], flags, out_feasible=masks[k], out_binding=binds[k])
            e.apply_bindings_device(binds[k], rc_t, rm_t)
        torch.cuda.synchronize()
        cpu, mem = c.avail_cpu, c.avail_mem
        for k in range(steps):
            feas, _, bind = capi.eval_encoded(cpu, mem, c.node_labels, None, c.req_cpu, c.req_mem, c.pod_sel, None, samples[k], flags)
            assert np.array_equal(masks[k].cpu().numpy().view(np.uint64), feas), f"step {k}: mask"
            got_b = binds[k].cpu().numpy()
            assert np.array_equal(got_b, bind), f"step {k}: bindings"
            if k == 0:
                assert (got_b >= 0).sum() > 1000
            cpu, mem, _ = restate(cpu, mem, got_b, c.req_cpu, c.req_mem)
        got = e.read_nodes()
        assert np.array_equal(got[0], cpu) and np.array_equal(got[1], mem)


def test_bestfit_after_apply_c5_shard(built):
    """125 000 pods x 50 000 nodes with taints: the best-fit order is built, an apply marks it stale, the next best-fit picks equal the
    oracle on the new columns (a sample of the rows: every pod's pick depends on the snapshot alone)"""
    c = synth.make_config("C5", P=125_000)
    base = FIT | SEL | TAINT
    rows = np.random.default_rng(8).choice(c.P, 4000, replace=False)
    rows.sort()
    with Evaluator(0) as e:
        e.set_nodes(**c.node_columns())
        rc_t, rm_t, sel_t, tol_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(c.pod_tol, np.int64)
        b0 = torch.empty((c.P,), dtype=torch.int32, device=DEV)
        e.eval_device(rc_t, rm_t, sel_t, tol_t, None, base | PICK_BESTFIT, out_binding=b0)  # builds the best-fit order
        bs = torch.empty_like(b0)
        e.eval_device(rc_t, rm_t, sel_t, tol_t, t(c.samples, np.int32), base | PICK_SAMPLED, out_binding=bs)
        e.apply_bindings_device(bs, rc_t, rm_t)
        b1 = torch.empty_like(b0)
        e.eval_device(rc_t, rm_t, sel_t, tol_t, None, base | PICK_BESTFIT, out_binding=b1)
        torch.cuda.synchronize()
        cpu, mem, _ = restate(c.avail_cpu, c.avail_mem, bs.cpu().numpy(), c.req_cpu, c.req_mem)
        assert not np.array_equal(cpu, c.avail_cpu)
        sel_r = np.ascontiguousarray(c.pod_sel[:, rows])
        want0 = capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels, c.node_taints, c.req_cpu[rows], c.req_mem[rows], sel_r, c.pod_tol[rows],
                                  None, base | PICK_BESTFIT, want_mask=False)[2]
        want1 = capi.eval_encoded(cpu, mem, c.node_labels, c.node_taints, c.req_cpu[rows], c.req_mem[rows], sel_r, c.pod_tol[rows],
                                  None, base | PICK_BESTFIT, want_mask=False)[2]
        assert np.array_equal(b0.cpu().numpy()[rows], want0)
        got1 = b1.cpu().numpy()[rows]
        assert np.array_equal(got1, want1)
        assert not np.array_equal(want0, want1)


def test_release_restores_the_snapshot_bit_for_bit(ev):
    c = synth.make_cluster(20_000, 7000, n_keys=8, n_taints=16, seed=1234)
    cols = c.node_columns()
    ev.set_nodes(**cols)
    before = ev.index_checksum()
    b, ok = random_bindings(np.random.default_rng(1), c.N, c.P)
    st = apply(ev, b, c.req_cpu, c.req_mem, ok)
    assert ev.index_checksum() != before
    st2 = apply(ev, b, c.req_cpu, c.req_mem, ok, _lib.APPLY_RELEASE)
    assert np.array_equal(st, st2)
    got = ev.read_nodes()
    assert np.array_equal(got[0], c.avail_cpu) and np.array_equal(got[1], c.avail_mem)
    assert ev.index_checksum() == before


def test_overflow_leaves_the_node_and_reports_its_pods(ev, ref):
    N = 2100
    rng = np.random.default_rng(21)
    cpu = rng.integers(0, 64_000, N).astype(np.int64)
    mem = rng.integers(0, 1 << 40, N).astype(np.int64)
    big = 1 << 62
    cpu[:8] = [I64_MAX - 5, I64_MIN + 5, 0, I64_MAX, I64_MIN, 1, -1, I64_MAX - (1 << 40)]
    mem[8:16] = [I64_MAX - 5, I64_MIN + 5, 0, I64_MAX, I64_MIN, 1, -1, I64_MIN + (1 << 40)]
    cols = dict(avail_cpu_milli=cpu, avail_mem_bytes=mem, label_val_ids=rng.integers(0, 4, (2, N)).astype(np.uint32), taints=None)
    P = 9000
    b = rng.integers(0, N, P).astype(np.int32)
    rc = rng.integers(-1000, 4000, P).astype(np.int64)
    rm = rng.integers(-(1 << 20), 1 << 32, P).astype(np.int64)
    # pods of both signs and huge magnitudes onto the edge nodes; some sums leave int64, some only pass outside it on the way
    k = 0
    for node in range(16):
        for v in (big, big, -big, -big, 7, -7, big, -big - 3, (1 << 31) + 1, -(1 << 33)):
            b[k], rc[k], rm[k] = node, v if node < 8 else rc[k], v if node >= 8 else rm[k]
            k += 1
    b[k:k + 6] = 2
    rc[k:k + 6] = [big, big, big, -big, -big, -big]  # node 2 (cpu 0): 3 * 2^62 on the way, 0 at the end
    results = []
    for _ in range(3):
        ev.set_nodes(**cols)
        st = apply(ev, b, rc, rm)
        results.append((st, *ev.read_nodes(), ev.index_checksum()))
    ncpu, nmem, want = restate(cpu, mem, b, rc, rm)
    st, gc, gm, chk = results[0]
    assert np.array_equal(st, want)
    assert np.array_equal(gc, ncpu) and np.array_equal(gm, nmem)
    assert (want == _lib.APPLY_OVERFLOW).sum() >= 10 and (want == _lib.APPLY_APPLIED).sum() > 8000
    ovf_nodes = set(b[want == _lib.APPLY_OVERFLOW].tolist())
    assert 2 not in ovf_nodes and len(ovf_nodes) >= 3
    for node in ovf_nodes:
        assert gc[node] == cpu[node] and gm[node] == mem[node]
    for r in results[1:]:
        assert np.array_equal(r[0], st) and np.array_equal(r[1], gc) and np.array_equal(r[2], gm) and r[3] == chk
    assert chk == fresh_checksum(ref, cols, ncpu, nmem)


@pytest.mark.parametrize("own_stream", [0, 1])
def test_ordering_between_streams(built, own_stream):
    """an evaluation enqueued on stream A before an apply enqueued on stream B reads the old snapshot; evaluations enqueued afterwards,
    on A and on B, read the new one"""
    c = synth.make_config("C3")
    flags = FIT | SEL | PICK_SAMPLED
    with Evaluator(0) as e:
        e.set_option(_lib.OPT_SNAPSHOT_STREAM, own_stream)
        e.set_nodes(**c.node_columns())
        A, B = torch.cuda.Stream(), torch.cuda.Stream()
        rc_t, rm_t, sel_t, smp_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(c.samples, np.int32)
        bind_in = t(np.random.default_rng(4).integers(-1, c.N, c.P).astype(np.int32), np.int32)
        outs = [(torch.empty((c.P, e.W), dtype=torch.int64, device=DEV), torch.empty((c.P,), dtype=torch.int32, device=DEV)) for _ in range(3)]
        torch.cuda.synchronize()
        e.eval_device(rc_t, rm_t, sel_t, None, smp_t, flags, out_feasible=outs[0][0], out_binding=outs[0][1], stream=A)
        e.apply_bindings_device(bind_in, rc_t, rm_t, stream=B)
        e.eval_device(rc_t, rm_t, sel_t, None, smp_t, flags, out_feasible=outs[1][0], out_binding=outs[1][1], stream=A)
        e.eval_device(rc_t, rm_t, sel_t, None, smp_t, flags, out_feasible=outs[2][0], out_binding=outs[2][1], stream=B)
        torch.cuda.synchronize()
        old = capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels, None, c.req_cpu, c.req_mem, c.pod_sel, None, c.samples, flags)
        cpu, mem, _ = restate(c.avail_cpu, c.avail_mem, bind_in.cpu().numpy(), c.req_cpu, c.req_mem)
        new = capi.eval_encoded(cpu, mem, c.node_labels, None, c.req_cpu, c.req_mem, c.pod_sel, None, c.samples, flags)
        for (m, b), (feas, _, bind), what in zip(outs, (old, new, new), ("before, A", "after, A", "after, B")):
            assert np.array_equal(m.cpu().numpy().view(np.uint64), feas), what
            assert np.array_equal(b.cpu().numpy(), bind), what
        assert not np.array_equal(old[2], new[2])
        e.forget_stream(A)
        e.forget_stream(B)


def test_errors(built):
    with Evaluator(0) as e:
        one64, one32 = torch.zeros((1,), dtype=torch.int64, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)
        with pytest.raises(KschedError) as ei:
            e.apply_bindings_device(one32, one64, one64)
        assert ei.value.code == _lib.E_STATE
        with pytest.raises(KschedError) as ei:
            e.read_nodes(0, 1)
        assert ei.value.code == _lib.E_STATE
        e.set_nodes(np.array([5], dtype=np.int64), np.array([5], dtype=np.int64))
        with pytest.raises(KschedError) as ei:
            e.apply_bindings_device(one32, one64, one64, flags=0x4)
        assert ei.value.code == _lib.E_INVAL
        lib = e._lib
        assert lib.ksched_apply_bindings_device(e._h, 1, None, None, None, None, 0, None, None) == _lib.E_INVAL
        assert lib.ksched_apply_bindings_device(e._h, 0, None, None, None, None, 0, None, None) == _lib.OK
        with pytest.raises(KschedError) as ei:
            e.read_nodes(0, 2)
        assert ei.value.code == _lib.E_INVAL
        with pytest.raises(ValueError):
            e.apply_bindings_device(one32, one64, torch.zeros((2,), dtype=torch.int64, device=DEV))
        assert [x.tolist() for x in e.read_nodes()] == [[5], [5]]
