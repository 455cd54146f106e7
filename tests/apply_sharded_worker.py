"""Child process of tests/test_gpu_apply_sharded.py: ksched_apply_bindings_sharded* with n ranks on one GPU.

    python -m tests.apply_sharded_worker <case> '<json spec>'

The n > 1 cases run against the test build of the library (tests/cpp/hooks/libksched_hip.so, $KSCHED_TEST_HOOKS=1) with the RCCL
stand-in (tests/cpp/libfake_rccl.so) that lets one GPU hold every rank; n = 1 runs the shipped library over the real RCCL.  A case
prints "ok <case>" as its last line when all its checks passed (an assertion ends the process with its message otherwise).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, PICK_SAMPLED, SEL, TAINT, Evaluator, KschedError, _lib, synth
from kube_scheduler_rs_reference_amd.dist import AbiComm, LocalClique, shard_bounds
from oracle import capi
from tests.test_gpu_apply_bindings import random_bindings, restate

DEV = torch.device("cuda:0")
FPN, REL = _lib.APPLY_FIRST_PER_NODE, _lib.APPLY_RELEASE


def t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def cuts(rng, P, n, kind):
    """row boundaries [n + 1] of n shards of P pods: ragged (random cut points), or ragged with the middle (or only) shard empty"""
    b = [0] + sorted(int(x) for x in rng.integers(0, P + 1, n - 1)) + [P]
    if kind == "empty":
        if n == 1:
            return [0, 0]  # a one-rank clique with nothing to apply still runs the call
        m = n // 2
        b[m] = b[m + 1]  # (shard m - 1 takes its rows: every row stays in exactly one shard)
    return b


def batch(seed, N, P, overflow):
    """bindings, ok and requests of one batch; with `overflow`, pods 0..7 carry requests of 2^62 bound to nodes 0 and 1"""
    rng = np.random.default_rng(seed)
    b, ok = random_bindings(rng, N, P)
    c = synth.make_cluster(P, max(N, 1), n_keys=0, seed=seed)
    rc, rm = c.req_cpu.copy(), c.req_mem.copy()
    big = rng.random(P) < 0.02
    rc[big] = rng.integers(1 << 33, 1 << 40, int(big.sum()))  # nonzero high halves
    if overflow and P >= 8:
        for i in range(8):
            b[i] = i % min(N, 2)
            ok[i] = 1
            if i % 2 == 0:
                rc[i] = 1 << 62
            rm[i] = -(1 << 62) if i % 3 == 0 else (1 << 62)
    return b, ok, rc, rm


class Ranks:
    """n evaluators on device 0 as one clique, and a reference evaluator that applies the concatenated batch"""

    def __init__(self, n, cols):
        self.evs = [Evaluator(0) for _ in range(n)]
        self.ref = Evaluator(0)
        self.cols = cols
        for e in self.evs + [self.ref]:
            e.set_nodes(**cols)
        self.clique = LocalClique(self.evs)

    def apply(self, bounds, b, ok, rc, rm, flags, use_ok=True):
        n = len(self.evs)
        sl = [slice(bounds[r], bounds[r + 1]) for r in range(n)]
        st = [torch.full((s.stop - s.start,), -7, dtype=torch.int32, device=DEV) for s in sl]
        self.clique.apply_bindings([t(b[s], np.int32) for s in sl], [t(rc[s], np.int64) for s in sl], [t(rm[s], np.int64) for s in sl],
                                   [bounds[r] for r in range(n)], ok=[t(ok[s], np.uint8) for s in sl] if use_ok else None, flags=flags,
                                   status_out=st)
        w = slice(bounds[0], bounds[-1])  # the concatenation of the shards (empty when the only shard is)
        want = torch.full((w.stop - w.start,), -7, dtype=torch.int32, device=DEV)
        self.ref.apply_bindings_device(t(b[w], np.int32), t(rc[w], np.int64), t(rm[w], np.int64), t(ok[w], np.uint8) if use_ok else None,
                                       flags, want)
        torch.cuda.synchronize()
        return [s.cpu().numpy() for s in st], want.cpu().numpy()

    def check_equal(self, what):
        """every rank's columns and index checksum == the reference's; -> the reference's columns"""
        cols, ck = self.ref.read_nodes(), self.ref.index_checksum()
        for r, e in enumerate(self.evs):
            got = e.read_nodes()
            assert np.array_equal(got[0], cols[0]) and np.array_equal(got[1], cols[1]), f"{what}: rank {r} columns"
            assert e.index_checksum() == ck, f"{what}: rank {r} index checksum"
        return cols

    def close(self):
        self.clique.close()
        for e in self.evs + [self.ref]:
            e.close()


def case_equal(spec):
    """replicas == one ctx's ksched_apply_bindings_device over the concatenated rows (itself == the exact-integer rule), for every node
    count of spec["nodes"] and every flag set, with and without ok, ragged shards and an empty shard, nodes driven to overflow"""
    n = spec["n"]
    k = 0
    for N in spec["nodes"]:
        P = min(max(2 * N + 11, 700), 100_000)
        c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=0x5A + N)
        cols = c.node_columns()
        if N >= 2:  # node 1 close to the int64 ends: the 2^62 requests of `batch` overflow it whichever way they go
            cols["avail_cpu_milli"] = cols["avail_cpu_milli"].copy()
            cols["avail_mem_bytes"] = cols["avail_mem_bytes"].copy()
            cols["avail_cpu_milli"][1] = -(1 << 62)
            cols["avail_mem_bytes"][1] = 1 << 62
        R = Ranks(n, cols)
        prev = (cols["avail_cpu_milli"], cols["avail_mem_bytes"])
        for flags in (0, FPN, REL, FPN | REL):
            k += 1
            use_ok, kind, ovf = k % 2 == 0, ("ragged", "empty")[k % 3 == 0], k % 4 != 2
            b, ok, rc, rm = batch(1000 * N + flags, N, P, ovf)
            bounds = cuts(np.random.default_rng(k), P, n, kind)
            st, want = R.apply(bounds, b, ok, rc, rm, flags, use_ok)
            what = f"n={n} N={N} flags={flags} ok={use_ok} shards={kind} overflow={ovf}"
            cpu, mem = R.check_equal(what)
            for r in range(n):
                assert np.array_equal(st[r], want[bounds[r]:bounds[r + 1]]), f"{what}: rank {r} status"
            w = slice(bounds[0], bounds[-1])
            exp = restate(prev[0], prev[1], b[w], rc[w], rm[w], ok[w] if use_ok else None, flags)
            assert np.array_equal(exp[0], cpu) and np.array_equal(exp[1], mem) and np.array_equal(exp[2], want), f"{what}: exact rule"
            if ovf and N >= 2 and not flags & FPN and w.stop > 8:
                assert (want == _lib.APPLY_OVERFLOW).any(), f"{what}: no overflow was provoked"
            prev = (cpu, mem)
        R.close()
    print(f"{k} sharded applies")


def case_scratch(spec):
    """a single-ctx apply after a sharded one (and the reverse) gives what it gives on a fresh ctx: the scratch is idle after either"""
    n, N, P = spec["n"], 5000, 40_000
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=91)
    cols = c.node_columns()
    batches = [batch(11, N, P, False), batch(12, N, P, False)]
    bounds = cuts(np.random.default_rng(3), P, n, "ragged")
    for order in ("sharded-then-single", "single-then-sharded"):
        R = Ranks(n, cols)
        fresh = Evaluator(0)
        fresh.set_nodes(**cols)
        for step, (b, ok, rc, rm) in enumerate(batches):
            if (step == 0) == (order == "sharded-then-single"):
                R.apply(bounds, b, ok, rc, rm, FPN)
            else:
                for e in R.evs + [R.ref]:
                    e.apply_bindings_device(t(b, np.int32), t(rc, np.int64), t(rm, np.int64), t(ok, np.uint8), FPN)
            fresh.apply_bindings_device(t(b, np.int32), t(rc, np.int64), t(rm, np.int64), t(ok, np.uint8), FPN)
            torch.cuda.synchronize()
            now = R.check_equal(f"{order} step {step}")
            got = fresh.read_nodes()
            assert np.array_equal(got[0], now[0]) and np.array_equal(got[1], now[1]), f"{order} step {step}: fresh ctx"
            assert fresh.index_checksum() == R.ref.index_checksum(), f"{order} step {step}: fresh ctx index"
        fresh.close()
        R.close()


def case_chain(spec):
    """per rank: evaluate its rows -> ksched_allgather_bindings_local -> sharded apply of its rows of the gathered table -> evaluate
    again, three rounds; bindings (and the sampled pick's mask rows) equal the oracle on the snapshot the rounds before left"""
    n, mode = spec["n"], spec["mode"]
    if mode == "sampled":
        c = synth.make_config("C3")
        flags = FIT | SEL | PICK_SAMPLED
    else:
        c = synth.make_config("C5", P=125_000)
        flags = FIT | SEL | TAINT | PICK_BESTFIT
    P, N = c.P, c.N
    rounds = 3
    rng = np.random.default_rng(17)
    samples = [rng.integers(0, N, (P, 5)).astype(np.uint32) for _ in range(rounds)]
    evs = [Evaluator(0) for _ in range(n)]
    for e in evs:
        e.set_nodes(**c.node_columns())
    clique = LocalClique(evs)
    lo = [shard_bounds(P, n, r)[0] for r in range(n)]
    hi = [shard_bounds(P, n, r)[1] for r in range(n)]
    cpr = shard_bounds(P, n, 0)[2]
    W = evs[0].W
    rc_t = [t(c.req_cpu[lo[r]:hi[r]], np.int64) for r in range(n)]
    rm_t = [t(c.req_mem[lo[r]:hi[r]], np.int64) for r in range(n)]
    sel_t = [t(c.pod_sel[:, lo[r]:hi[r]], np.int32) for r in range(n)]
    tol_t = [t(c.pod_tol[lo[r]:hi[r]], np.int64) if flags & TAINT else None for r in range(n)]
    cpu, mem = c.avail_cpu, c.avail_mem
    rows = np.sort(np.random.default_rng(8).choice(P, 4000, replace=False))
    for k in range(rounds):
        local = [torch.full((cpr,), -1, dtype=torch.int32, device=DEV) for _ in range(n)]
        gathered = [torch.empty((n * cpr,), dtype=torch.int32, device=DEV) for _ in range(n)]
        masks = []
        for r, e in enumerate(evs):
            m = torch.empty((hi[r] - lo[r], W), dtype=torch.int64, device=DEV) if mode == "sampled" else None
            smp = t(samples[k][lo[r]:hi[r]], np.int32) if mode == "sampled" else None
            e.eval_device(rc_t[r], rm_t[r], sel_t[r], tol_t[r], smp, flags, out_feasible=m, out_binding=local[r][:hi[r] - lo[r]])
            masks.append(m)
        clique.allgather_bindings(gathered, local)
        clique.apply_bindings([gathered[r][r * cpr:r * cpr + hi[r] - lo[r]] for r in range(n)], rc_t, rm_t, lo)
        torch.cuda.synchronize()
        tables = [g.cpu().numpy() for g in gathered]
        for r in range(1, n):
            assert np.array_equal(tables[r], tables[0]), f"round {k}: rank {r}'s gathered table"
        got_b = np.concatenate([tables[0][r * cpr:r * cpr + hi[r] - lo[r]] for r in range(n)])
        if mode == "sampled":
            feas, _, bind = capi.eval_encoded(cpu, mem, c.node_labels, None, c.req_cpu, c.req_mem, c.pod_sel, None, samples[k], flags)
            assert np.array_equal(got_b, bind), f"round {k}: bindings"
            got_m = np.concatenate([m.cpu().numpy().view(np.uint64) for m in masks])
            assert np.array_equal(got_m, feas), f"round {k}: mask rows"
        else:  # (a sample of the rows: every pod's pick depends on the snapshot alone)
            bind = capi.eval_encoded(cpu, mem, c.node_labels, c.node_taints, c.req_cpu[rows], c.req_mem[rows],
                                     np.ascontiguousarray(c.pod_sel[:, rows]), c.pod_tol[rows], None, flags, want_mask=False)[2]
            assert np.array_equal(got_b[rows], bind), f"round {k}: best-fit bindings"
        assert (got_b >= 0).sum() > 1000, f"round {k}: too few pods bound to show anything"
        cpu, mem, _ = restate(cpu, mem, got_b, c.req_cpu, c.req_mem)
        for r, e in enumerate(evs):
            g = e.read_nodes()
            assert np.array_equal(g[0], cpu) and np.array_equal(g[1], mem), f"round {k}: rank {r} snapshot"
    assert not np.array_equal(cpu, c.avail_cpu)
    clique.close()
    for e in evs:
        e.close()


def expect_error(code, fn, what):
    try:
        fn()
    except KschedError as x:
        assert x.code == code, f"{what}: {x}"
        return x
    raise AssertionError(f"{what}: no error")


def case_failure(spec):
    """$FAKE_RCCL_FAIL_ALLGATHER (set by the parent) makes the second all-gather call of the first sharded apply fail on the host side:
    KSCHED_E_RCCL, every ctx refuses work with KSCHED_E_STATE until ksched_set_nodes, the aborted clique refuses further calls, a new
    clique works"""
    n, N, P = 3, 5000, 30_000
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=5)
    cols = c.node_columns()
    R = Ranks(n, cols)
    b, ok, rc, rm = batch(7, N, P, False)
    bounds = cuts(np.random.default_rng(1), P, n, "ragged")
    x = expect_error(_lib.E_RCCL, lambda: R.apply(bounds, b, ok, rc, rm, FPN), "the injected failure")
    assert "aborted" in str(x), x
    torch.cuda.synchronize()
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    for r, e in enumerate(R.evs):
        mask = torch.empty((P, e.W), dtype=torch.int64, device=DEV)
        expect_error(_lib.E_STATE, lambda: e.eval_device(rc_t, rm_t, flags=FIT, out_feasible=mask), f"rank {r}: evaluation")
        expect_error(_lib.E_STATE, lambda: e.read_nodes(), f"rank {r}: read_nodes")
        expect_error(_lib.E_STATE, lambda: e.apply_bindings_device(t(b, np.int32), rc_t, rm_t), f"rank {r}: apply")
    empty32, empty64 = t(b[:0], np.int32), t(rc[:0], np.int64)
    expect_error(_lib.E_INVAL, lambda: R.clique.apply_bindings([empty32] * n, [empty64] * n, [empty64] * n, [0] * n), "the aborted clique")
    R.clique.close()
    for e in R.evs:
        e.set_nodes(**cols)
    R.ref.set_nodes(**cols)
    R.clique = LocalClique(R.evs)
    st, want = R.apply(bounds, b, ok, rc, rm, FPN)
    R.check_equal("a new clique")
    for r in range(n):
        assert np.array_equal(st[r], want[bounds[r]:bounds[r + 1]]), f"a new clique: rank {r} status"
    R.close()


def case_errors(spec):
    """argument errors of both forms (a ctx and a comm on different devices needs a second GPU: not covered on a one-GPU box)"""
    import ctypes as C
    lib = _lib.load()
    N, P = 2000, 3000
    c = synth.make_cluster(P, N, n_keys=0, seed=3)
    evs = [Evaluator(0) for _ in range(2)]
    for e in evs:
        e.set_nodes(**c.node_columns())
    clique = LocalClique(evs)
    b = t(np.zeros(P, np.int32), np.int32)
    rq = t(np.ones(P, np.int64), np.int64)
    vp = lambda x: C.cast(x, C.c_void_p)  # noqa: E731
    ptrs = lambda *xs: (C.c_void_p * len(xs))(*xs)  # noqa: E731
    u32s = lambda *xs: (C.c_uint32 * len(xs))(*xs)  # noqa: E731
    h0, h1 = evs[0]._h.value, evs[1]._h.value
    comms = clique._comms

    def call(ctxs, cms, counts=(P, 0), lows=(0, P), bind=(b.data_ptr(), None), flags=0):
        return lib.ksched_apply_bindings_sharded_local(None if ctxs is None else vp(ptrs(*ctxs)), None if cms is None else vp(cms), 2,
                                                       vp(u32s(*counts)), vp(u32s(*lows)), vp(ptrs(*bind)),
                                                       vp(ptrs(rq.data_ptr(), rq.data_ptr())), vp(ptrs(rq.data_ptr(), rq.data_ptr())),
                                                       None, flags, None, None)

    cases = [
        ("NULL ctxs", _lib.E_INVAL, lambda: call(None, comms)),
        ("NULL comms", _lib.E_INVAL, lambda: call((h0, h1), None)),
        ("a NULL ctx", _lib.E_INVAL, lambda: call((h0, None), comms)),
        ("one ctx twice", _lib.E_INVAL, lambda: call((h0, h0), comms)),
        ("unknown flags", _lib.E_INVAL, lambda: call((h0, h1), comms, flags=0x80)),
        ("NULL bindings with count > 0", _lib.E_INVAL, lambda: call((h0, h1), comms, bind=(None, None))),
        ("global pod index past 0xFFFFFFFE", _lib.E_INVAL, lambda: call((h0, h1), comms, counts=(P, 1), lows=(0, 0xFFFFFFFF),
                                                                        bind=(b.data_ptr(), b.data_ptr()))),
        ("per-process form, NULL ctx", _lib.E_INVAL, lambda: lib.ksched_apply_bindings_sharded(None, comms[0], 0, 0, None, None, None, None, 0,
                                                                                              None, None)),
        ("per-process form, NULL comm", _lib.E_INVAL, lambda: lib.ksched_apply_bindings_sharded(evs[0]._h, None, 0, 0, None, None, None, None,
                                                                                               0, None, None)),
        ("per-process form, unknown flags", _lib.E_INVAL, lambda: lib.ksched_apply_bindings_sharded(evs[0]._h, comms[0], 0, 0, None, None, None,
                                                                                                   None, 0x04, None, None)),
    ]
    for what, code, fn in cases:
        rc = fn()
        assert rc == code, f"{what}: {rc} != {code}"
    evs[1].set_nodes(**synth.make_cluster(P, N + 1, n_keys=0, seed=4).node_columns())
    rc = call((h0, h1), comms)
    assert rc == _lib.E_INVAL, f"different node counts: {rc}"
    fresh = Evaluator(0)
    clique2 = LocalClique([evs[0], fresh])
    rc = call((h0, fresh._h.value), clique2._comms)
    assert rc == _lib.E_STATE, f"a ctx without a snapshot: {rc}"
    g = evs[0].read_nodes()  # nothing above changed a snapshot
    assert np.array_equal(g[0], c.avail_cpu) and np.array_equal(g[1], c.avail_mem)
    clique2.close()
    clique.close()
    for e in evs + [fresh]:
        e.close()


def case_rank(spec):
    """one process of the per-process form (dist.AbiComm over the stand-in's clique of processes); rank 0 also runs the single-ctx
    reference.  The results go to <dir>/rank<r>.npz for the parent to compare."""
    import torch.distributed as dist
    rank, world, d = spec["rank"], spec["world"], spec["dir"]
    dist.init_process_group("gloo", init_method=f"file://{os.path.join(d, 'store')}", rank=rank, world_size=world)
    N, P = 5000, 40_000
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=44)
    cols = c.node_columns()
    e = Evaluator(0)
    e.set_nodes(**cols)
    comm = AbiComm(e)
    ref = None
    if rank == 0:
        ref = Evaluator(0)
        ref.set_nodes(**cols)
    out = {}
    for k, flags in enumerate((FPN, 0, FPN | REL)):
        b, ok, rc, rm = batch(300 + k, N, P, False)
        bounds = cuts(np.random.default_rng(k), P, world, "empty" if k == 2 else "ragged")
        s = slice(bounds[rank], bounds[rank + 1])
        st = torch.full((s.stop - s.start,), -7, dtype=torch.int32, device=DEV)
        comm.apply_bindings(t(b[s], np.int32), t(rc[s], np.int64), t(rm[s], np.int64), bounds[rank], ok=t(ok[s], np.uint8), flags=flags,
                            status_out=st)
        torch.cuda.synchronize()
        out[f"cpu{k}"], out[f"mem{k}"] = e.read_nodes()
        out[f"st{k}"] = st.cpu().numpy()
        out[f"sum{k}"] = np.array(e.index_checksum(), dtype=np.uint64)
        out[f"lo{k}"] = np.array([s.start, s.stop])
        if ref is not None:
            want = torch.full((P,), -7, dtype=torch.int32, device=DEV)
            ref.apply_bindings_device(t(b, np.int32), t(rc, np.int64), t(rm, np.int64), t(ok, np.uint8), flags, want)
            torch.cuda.synchronize()
            out[f"ref_cpu{k}"], out[f"ref_mem{k}"] = ref.read_nodes()
            out[f"ref_st{k}"] = want.cpu().numpy()
            out[f"ref_sum{k}"] = np.array(ref.index_checksum(), dtype=np.uint64)
    np.savez(os.path.join(d, f"rank{rank}.npz"), **out)
    comm.close()
    e.close()
    if ref is not None:
        ref.close()
    dist.destroy_process_group()


def walk_paths(spec, begin, matrix, apply, end):
    """case_paths' sequence with the replicas behind callables (tests/apply_paths_worker.walk_single's arrangement; walked without a GPU
    by tests/test_apply_paths_host.py): begin(S, what) loads every replica; matrix(q, S, cpu, mem, what, rng, hand_on=,
    input_condition=) runs replica q's reduced matrix and -> the bindings of the pick `hand_on` names; apply(S, cpu, mem, bounds, b, ok,
    flags, use_ok, what) -> (cpu, mem, statuses) after the sharded apply; end() closes the replicas.
    Per snapshot round 0 applies real bindings, round 1 random ones.  Which pick hands the real ones on goes by the node count: above
    5000 nodes the spread pick, from 1025 on the sampled and the uniform pick (one per kind, swapped with the number of ranks), below
    1025 each of the three in turn over the kinds and n = 1, 2, 3 -- so every pick hands on in both classes of node counts.  At every
    snapshot from 1025 nodes on, the columns from before the apply of real bindings must change at least one restated spread binding
    (apply_paths_worker.stale_spread_bindings): a replica left behind by the gathered commit cannot pass.  One exception, stated where it is
    asserted: a RELEASE of the spread pick's own bindings above 5000 nodes, which counts in its node count's sum only."""
    from tests.apply_paths_worker import PICKS, snapshot, stale_spread_bindings
    n = spec["n"]
    k = 0
    changed = {}
    for ki, kind in enumerate(("taints", "list-key")):
        for N in spec["nodes"]:
            P = 1500 if N <= 5000 else 600
            S = snapshot(kind, N, P, 0x5B + N)
            begin(S, f"n={n} {kind} N={N}")
            cpu, mem = S["cpu"], S["mem"]
            rng = np.random.default_rng(N + n)
            if N > 5000:  # 600 pods: only an apply of the spread pick's own bindings moves a column its next evaluation ranks by
                hand_on = "spread"
            elif N >= 1025:
                hand_on = ("sampled", "uniform")[(ki + n) % 2]
            else:
                hand_on = PICKS[(ki + n) % len(PICKS)]
            bind = matrix(0, S, cpu, mem, f"{kind} N={N} before any apply", rng, hand_on=hand_on, input_condition=N >= 1025, terms_condition=N >= 63)
            for r in range(2):
                k += 1
                flags, use_ok = (0, FPN, REL, FPN | REL)[k % 4], k % 3 != 0
                b, ok = random_bindings(rng, N, P) if r else (bind, (rng.random(P) > 0.2).astype(np.uint8))
                bounds = cuts(rng, P, n, "ragged")
                what = f"n={n} {kind} N={N} round {r} flags={flags} ok={use_ok}"
                cpu0, mem0 = cpu, mem
                cpu, mem, want = apply(S, cpu, mem, bounds, b, ok, flags, use_ok, what)
                assert (want == _lib.APPLY_APPLIED).any(), f"{what}: nothing applied"
                if r == 0:
                    stale = stale_spread_bindings(S, cpu, mem, cpu0, mem0)
                    print(f"{what} ({hand_on} bindings): the columns from before this apply would change {stale} of {P} spread bindings (d = 5)")
                    changed[N] = changed.get(N, 0) + stale
                    # per snapshot wherever it can hold.  The one exception: RELEASE of the spread pick's OWN bindings above 5000 nodes gives
                    # every winner more, so its next evaluation ranks as before -- restated, 0 or 1 of 600 pods change there, and as few with
                    # 1000 or 1500 pods (a larger P does not help); that snapshot counts only in its node count's sum below
                    release_of_own = hand_on == "spread" and bool(flags & REL) and N > 5000
                    assert stale > 0 or N < 1025 or release_of_own, \
                        f"{what}: no spread binding depends on what this apply of {hand_on} bindings changed (only a RELEASE of the spread pick's own bindings above 5000 nodes may show none)"
                for q in range(n):
                    matrix(q, S, cpu, mem, f"{what} rank {q}", rng, hand_on=None)
            end()
    # and summed over a node count's rounds (both kinds), which covers the excepted snapshot's node count through the other kind
    for N, total in changed.items():
        assert total > 0 or N < 1025, f"n={n} N={N}: no spread binding depends on what this node count's applies of real bindings changed"
    return k


def case_paths(spec):
    """after each sharded apply every replica runs the reduced evaluation matrix of tests/apply_paths_worker.py against the oracle on the
    restated columns: the "select" pick, the riding pick in its waves form, ksched_explain, the direct kernel and (list key) best fit from
    the key's lists -- the paths that read the node records the gathered commit writes -- and the uniform and the spread pick; the spread
    pick ranks by the columns that commit has just written on every replica (walk_paths); and check_matrix's pack legs (the pack pick reads
    the same columns through a kernel of its own) and combining chains (KSCHED_COMBINE_*, KSCHED_COMBINE_SOFT: each evaluates into the
    replica's scratch mask), against tests/pack_ref.py, tests/combine_ref.py and tests/soft_ref.py; and its operator and tagged selector
    legs (KSCHED_SELOP_EXISTS / _GT / _LT, KSCHED_SELOP_TAGGED): the bare masks, the plain table under the tagged call against the
    oracle, and the selector chain whose last link's pick reads the columns the gathered commit has just written, against
    tests/selop_ref.py and tests/seltag_ref.py -- all five picks of that link are reached in every run (asserted); and its legs of the
    terms call (KSCHED_SEL_TERMS): the bare mask of the three-term table against tests/selterms_ref.py, one term against the tagged mask,
    the padded plain table against the oracle, and the terms chain whose soft last link carries each of the five picks in turn on the
    columns the gathered commit has just written (likewise asserted)"""
    from tests.apply_paths_worker import check_matrix
    n = spec["n"]
    seen = set()
    R = [None]

    def begin(S, what):
        R[0] = Ranks(n, dict(avail_cpu_milli=S["cpu"], avail_mem_bytes=S["mem"], label_val_ids=S["lab"], taints=S["tnt"]))

    def apply(S, cpu, mem, bounds, b, ok, flags, use_ok, what):
        st, want = R[0].apply(bounds, b, ok, S["rc"], S["rm"], flags, use_ok)
        got = R[0].check_equal(what)
        cpu, mem, exp = restate(cpu, mem, b, S["rc"], S["rm"], ok if use_ok else None, flags)
        assert np.array_equal(got[0], cpu) and np.array_equal(got[1], mem) and np.array_equal(exp, want), f"{what}: exact rule"
        for q in range(n):
            assert np.array_equal(st[q], want[bounds[q]:bounds[q + 1]]), f"{what}: rank {q} status"
        return cpu, mem, want

    k = walk_paths(spec, begin, lambda q, S, cpu, mem, what, rng, **kw: check_matrix(R[0].evs[q], S, cpu, mem, seen, what, rng, reduced=True, **kw),
                   apply, lambda: R[0].close())
    from tests.apply_paths_worker import LAST_LINKS
    # (check_matrix's pack legs, combining chains, selector chains and terms chains run on every replica too: the soft chain's, the selector
    # chain's and the terms chain's last link take each pick in turn)
    want = {"select", "fused", "bestfit-rows", "uniform", "spread", "pack"}
    for chain in ("chain", "selchain", "termchain"):
        want |= {f"{chain}-{p}" for p in LAST_LINKS}
    assert want <= seen, f"picks reached {sorted(seen)}, missing {sorted(want - seen)}"
    print(f"{k} sharded applies, picks reached {sorted(seen)}")


def case_large(spec):
    """two ranks whose shards are each longer than one stride of the pod kernels' grid (2048 x 256 threads)"""
    n, N = 2, 5000
    half = 2048 * 256 + 20_000
    P = 2 * half + 123
    c = synth.make_cluster(700, N, n_keys=8, n_taints=16, seed=0x1B)
    R = Ranks(n, c.node_columns())
    cpu, mem = c.avail_cpu, c.avail_mem
    rng = np.random.default_rng(2)
    for flags in (0, FPN, FPN | REL):
        b, ok, rc, rm = batch(900 + flags, N, P, False)
        b[(b >= 0) & (b < 16)] = 16  # nodes 0 .. 7 are named by rank 0's last rows only, nodes 8 .. 15 by rank 1's last rows only
        b[half - 4000:half] = rng.integers(0, 8, 4000)
        b[P - 4000:] = rng.integers(8, 16, 4000)
        bounds = [0, half + int(rng.integers(-100, 100)), P]
        st, want = R.apply(bounds, b, ok, rc, rm, flags)
        what = f"P={P} flags={flags}"
        got = R.check_equal(what)
        cpu, mem, exp = restate(cpu, mem, b, rc, rm, ok, flags)
        assert np.array_equal(got[0], cpu) and np.array_equal(got[1], mem) and np.array_equal(exp, want), f"{what}: exact rule"
        for q in range(n):
            assert np.array_equal(st[q], want[bounds[q]:bounds[q + 1]]), f"{what}: rank {q} status"
        assert (want[2048 * 256:bounds[1]] == _lib.APPLY_APPLIED).any() and (want[bounds[1] + 2048 * 256:] == _lib.APPLY_APPLIED).any(), what
    R.close()


def case_empty(spec):
    """an apply to a snapshot of no nodes with status_out, through the clique and on one ctx: the statuses are the exact rule's (all of them
    final after the accumulate pass), and every ctx evaluates right after"""
    n, P = spec["n"], 700
    none = np.zeros(0, np.int64)
    R = Ranks(n, {"avail_cpu_milli": none, "avail_mem_bytes": none})
    rng = np.random.default_rng(17)
    for k, flags in enumerate((0, FPN, REL, FPN | REL)):
        b = rng.integers(-3, 4, P).astype(np.int32)  # unbound, or past the (absent) last node
        ok = (rng.random(P) > 0.3).astype(np.uint8)
        rc, rm = rng.integers(0, 1 << 40, P), rng.integers(-(1 << 40), 1 << 40, P)
        use_ok, bounds = k % 2 == 0, cuts(rng, P, n, ("ragged", "empty")[k // 2])
        st, want = R.apply(bounds, b, ok, rc, rm, flags, use_ok)
        what = f"n={n} N=0 flags={flags} ok={use_ok}"
        R.check_equal(what)
        exp = restate(none, none, b, rc, rm, ok if use_ok else None, flags)
        assert np.array_equal(exp[2], want), f"{what}: exact rule"
        for r in range(n):
            assert np.array_equal(st[r], want[bounds[r]:bounds[r + 1]]), f"{what}: rank {r} status"
    z = np.zeros(5, np.int64)
    for e in R.evs + [R.ref]:
        res = e.eval(z, z, samples=np.zeros((5, 5), np.uint32), flags=FIT | PICK_SAMPLED)
        assert res.feasible.shape == (5, 0) and (res.binding == -1).all(), "evaluation after the apply"
    R.close()


CASES = {"equal": case_equal, "scratch": case_scratch, "chain": case_chain, "failure": case_failure, "errors": case_errors,
         "rank": case_rank, "paths": case_paths, "large": case_large, "empty": case_empty}

if __name__ == "__main__":
    name = sys.argv[1]
    CASES[name](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
    print(f"ok {name}")
