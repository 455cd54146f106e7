"""ksched_apply_bindings_device with KSCHED_APPLY_WHILE_FIT on the MI355X: per node, the eligible pods in pod order while they still fit.

Every expected column and status comes from tests/admit_ref.py (the contract of include/ksched.h in Python integers; pinned by hand-worked
answers in tests/test_admit_restatement.py), every expected mask and binding after an apply from the oracle (capi.eval_encoded) or the
picks' and the summary's restatements on those columns.  The index after an apply is compared with a fresh ksched_set_nodes of the expected
columns.  A library without the flag answers KSCHED_E_INVAL to every apply here.
"""
import numpy as np
import pytest
import torch

from kube_scheduler_rs_reference_amd import (FIT, PICK_BESTFIT, PICK_SAMPLED, PICK_SPREAD, SEL, TAINT, Evaluator, KschedError, _lib, synth)
from oracle import capi
from tests import summary_ref
from tests.admit_ref import (APPLIED, BAD_NODE, DEFERRED, I64_MAX, I64_MIN, NOT_OK, OVERFLOW, UNBOUND, admitted_behind_deferred,
                             apply_while_fit_exact, longest_segment)
from tests.spread_ref import spread_pick_blocks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WF = 0x08  # KSCHED_APPLY_WHILE_FIT (tests/test_admit_abi.py pins the three faces to it)
SENTINEL = -7


def t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def i64(a):
    return np.array(a, dtype=np.int64).reshape(-1)


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


def apply(ev, bindings, req_cpu, req_mem, ok=None, flags=WF):
    st = torch.full((len(bindings),), SENTINEL, dtype=torch.int32, device=DEV)
    ev.apply_bindings_device(t(bindings, np.int32), t(req_cpu, np.int64), t(req_mem, np.int64), None if ok is None else t(ok, np.uint8),
                             flags, st)
    torch.cuda.current_stream().synchronize()
    return st.cpu().numpy()


def random_bindings(rng, n, p):  # (as tests/test_gpu_apply_bindings.py makes them)
    b = rng.integers(0, n, p).astype(np.int32)
    b[rng.random(p) < 0.1] = -1
    b[rng.random(p) < 0.05] = 0 if n == 1 else int(rng.integers(0, n))  # many pods onto one node
    b[rng.random(p) < 0.01] = n + int(rng.integers(0, 5))  # past the last node
    ok = (rng.random(p) > 0.1).astype(np.uint8)
    return b, ok


def labelled(rng, cpu, mem):
    """node columns with two label keys: the snapshot gets a bitmap index, so the checksums say something"""
    return dict(avail_cpu_milli=i64(cpu), avail_mem_bytes=i64(mem), label_val_ids=rng.integers(0, 4, (2, len(cpu))).astype(np.uint32), taints=None)


def check(ev, ref, cols, b, rc, rm, ok=None):
    """set_nodes -> apply WHILE_FIT -> columns, every status and the index against the restatement; -> (cpu, mem, status) expected"""
    b, rc, rm = np.array(b, dtype=np.int32).reshape(-1), i64(rc), i64(rm)
    ok = None if ok is None else np.array(ok, dtype=np.uint8).reshape(-1)
    ev.set_nodes(**cols)
    before = ev.index_checksum()
    assert before != (0, 0)
    st = apply(ev, b, rc, rm, ok)
    cpu, mem, want = apply_while_fit_exact(cols["avail_cpu_milli"], cols["avail_mem_bytes"], b, rc, rm, ok)
    got_cpu, got_mem = ev.read_nodes()
    bad = np.nonzero(st != want)[0]
    assert len(bad) == 0, f"status of pods {bad[:10].tolist()}: got {st[bad[:10]].tolist()}, want {want[bad[:10]].tolist()}"
    assert np.array_equal(got_cpu, cpu) and np.array_equal(got_mem, mem)
    assert ev.index_checksum() == fresh_checksum(ref, cols, cpu, mem)
    return cpu, mem, want


# ---- 1. round trip ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 1024, 1025, 5000, 50_000])
def test_round_trip(ev, ref, N):
    P = min(max(3 * N + 7, 500), 60_000)
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=0xA9 + N)
    cols = c.node_columns()
    ev.set_nodes(**cols)
    b, ok = random_bindings(np.random.default_rng(N + 8), N, P)
    cpu, mem, want = apply_while_fit_exact(c.avail_cpu, c.avail_mem, b, c.req_cpu, c.req_mem, ok)
    # the inputs say something: every status but OVERFLOW, a segment longer than one chunk, the skip rule seen
    counts = np.bincount(want, minlength=6)
    print(f"N={N} P={P} status counts {counts.tolist()} longest segment {longest_segment(b, N, ok)} "
          f"admitted behind a deferred pod {admitted_behind_deferred(b, want)}")
    assert all(counts[s] > 0 for s in (APPLIED, UNBOUND, NOT_OK, DEFERRED, BAD_NODE))
    assert longest_segment(b, N, ok) > 64 and admitted_behind_deferred(b, want) > 0
    st = apply(ev, b, c.req_cpu, c.req_mem, ok)
    got_cpu, got_mem = ev.read_nodes()
    assert np.array_equal(st, want)  # (and so no sentinel is left)
    assert np.array_equal(got_cpu, cpu) and np.array_equal(got_mem, mem)
    assert ev.index_checksum() == fresh_checksum(ref, cols, cpu, mem)


# ---- 2. knife edges of the walk and the sort ----------------------------------------------------------------------------------------

def test_segment_lengths_around_the_chunk_and_the_sort_run(ev, ref):
    """one node per length 1, 63, 64, 65, 128, 129 and 1025, their pods shuffled among one another and among ineligible ones; every node has
    room for about half of what is asked of it, in requests of two sizes: admitted and deferred pods alternate inside the chunks"""
    rng = np.random.default_rng(201)
    lengths = [1, 63, 64, 65, 128, 129, 1025]
    b = np.concatenate([np.full(L, k, dtype=np.int32) for k, L in enumerate(lengths)] + [np.full(300, -1, dtype=np.int32),
                                                                                      np.full(40, len(lengths) + 2, dtype=np.int32)])
    rng.shuffle(b)
    p = len(b)
    rc = np.where(rng.random(p) < 0.3, rng.integers(100, 200, p), rng.integers(1, 5, p))  # (the large ones stop fitting long before the small)
    rm = rng.integers(1, 1 << 34, p)
    ok = (rng.random(p) > 0.1).astype(np.uint8)
    cpu = [max(1, int(rc[(b == k) & (ok != 0)].sum()) // 2) for k in range(len(lengths))]
    cols = labelled(rng, cpu, [1 << 50] * len(lengths))
    _, _, want = check(ev, ref, cols, b, rc, rm, ok)
    assert admitted_behind_deferred(b, want) > 100 and set(want.tolist()) == {APPLIED, UNBOUND, NOT_OK, DEFERRED, BAD_NODE}


@pytest.mark.parametrize("neg", [0, 1], ids=["shrink-only", "with-negative-requests"])
@pytest.mark.parametrize("f", [0, 63, 64])
def test_first_failing_lane(ev, ref, f, neg):
    """130 pods of 1 on one node with room for all of them, but pod f asks for more than the node has: it alone is deferred.  Without a
    negative request in its chunk the lane is deferred at the step's start; with one in each chunk the ballot has to name it"""
    rng = np.random.default_rng(f)
    rc = np.ones(130, dtype=np.int64)
    rc[f] = 5000
    if neg:
        rc[[5, 70]] = -1
    cpu, _, want = check(ev, ref, labelled(rng, [1000, 7], [1000, 7]), np.zeros(130, dtype=np.int32), rc, np.ones(130, dtype=np.int64))
    assert want[f] == DEFERRED and (np.delete(want, f) == APPLIED).all() and cpu.tolist() == [1000 - 129 + 4 * neg, 7]


@pytest.mark.parametrize("k", [63, 64, 65, 128])
def test_a_node_that_fills_at_and_around_a_chunk_boundary(ev, ref, k):
    """room for exactly k pods of 200 equal ones: the first failing lane is a chunk's last (k = 63), the next chunk's first (64, 128: the node
    is exactly full at the boundary) or its second (65)"""
    rng = np.random.default_rng(k)
    cpu, mem, want = check(ev, ref, labelled(rng, [k * 3], [k * 5]), np.zeros(200, dtype=np.int32), np.full(200, 3), np.full(200, 5))
    assert want.tolist() == [APPLIED] * k + [DEFERRED] * (200 - k) and cpu.tolist() == [0] and mem.tolist() == [0]


def test_a_herd_on_one_node(ev, ref):
    """20 000 pods of equal request onto one node that is full after 100: the chunks behind that are deferred at once"""
    rng = np.random.default_rng(7)
    P = 20_000
    cpu, _, want = check(ev, ref, labelled(rng, [5, 1000, 5], [1 << 40] * 3), np.ones(P, dtype=np.int32), np.full(P, 10), np.full(P, 1 << 20))
    assert want[:100].tolist() == [APPLIED] * 100 and (want[100:] == DEFERRED).all() and cpu.tolist() == [5, 0, 5]


@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 2048, 2049, 4097])
def test_sort_run_and_merge_boundaries_in_descending_node_order(ev, ref, P):
    """two pods per node, the batch in descending node order (the sort turns all of it round), ineligible pods interleaved; every node has
    room for one of its two pods"""
    rng = np.random.default_rng(P)
    N = (P + 1) // 2
    b = ((P - 1 - np.arange(P)) // 2).astype(np.int32)
    b[np.arange(P) % 11 == 5] = -1
    ok = (np.arange(P) % 7 != 3).astype(np.uint8)
    rc = rng.integers(6, 10, P)
    _, _, want = check(ev, ref, labelled(rng, [10] * N, [1 << 30] * N), b, rc, np.ones(P, dtype=np.int64), ok)
    if P > 1:
        assert (want == DEFERRED).sum() > P // 4 and (want == APPLIED).sum() > P // 4


def test_both_sides_of_the_tile_edge(ev, ref):
    """nodes 1023 and 1024 -- the last of tile 0 and the first of tile 1 -- are the only ones touched"""
    rng = np.random.default_rng(1023)
    N, P = 2048, 300
    cols = labelled(rng, rng.integers(100, 200, N), rng.integers(1 << 20, 1 << 30, N))
    b = np.where(np.arange(P) % 2 == 0, 1023, 1024).astype(np.int32)
    cpu, _, want = check(ev, ref, cols, b, np.full(P, 7), np.full(P, 1))
    assert cpu[1023] < 7 and cpu[1024] < 7 and (want == DEFERRED).sum() > 200
    untouched = np.ones(N, dtype=bool)
    untouched[[1023, 1024]] = False
    assert np.array_equal(cpu[untouched], cols["avail_cpu_milli"][untouched])


# ---- 3. the int64 ends and the signs ------------------------------------------------------------------------------------------------

KNOWN = [  # (what, cpu, mem, bindings, req_cpu, req_mem, statuses worked by hand, cpu after, mem after)
    ("zero on zero, zero on minus one", [0, -1, 0], [0, 0, -1], [0, 1, 2], [0, 0, 0], [0, 0, 0], [APPLIED, DEFERRED, DEFERRED], [0, -1, 0], [0, 0, -1]),
    ("a negative request revives nobody", [4], [4], [0, 0, 0], [6, -3, 6], [1, 0, 1], [DEFERRED, APPLIED, APPLIED], [1], [3]),
    ("exactly INT64_MAX", [I64_MAX - 2], [0], [0], [-2], [0], [APPLIED], [I64_MAX], [0]),
    ("one past INT64_MAX, and the node goes on", [I64_MAX - 2, 5], [7, I64_MAX], [0, 0, 1, 1, 1], [-3, 4, 1, 1, 5], [1, 1, -1, 2, 0],
     [OVERFLOW, APPLIED, OVERFLOW, APPLIED, DEFERRED], [I64_MAX - 6, 4], [6, I64_MAX - 2]),
    ("INT64_MIN off zero", [0], [0], [0, 0], [I64_MIN, I64_MIN], [0, 0], [OVERFLOW, OVERFLOW], [0], [0]),
    ("INT64_MIN off INT64_MIN", [I64_MIN], [0], [0, 0], [I64_MIN, I64_MAX], [0, 0], [APPLIED, DEFERRED], [0], [0]),
    ("INT64_MAX off INT64_MAX, twice", [I64_MAX], [I64_MAX], [0, 0, 0], [I64_MAX, I64_MAX, 0], [I64_MAX, 0, 0], [APPLIED, DEFERRED, APPLIED], [0], [0]),
    ("nothing fits INT64_MIN but INT64_MIN", [I64_MIN], [I64_MIN], [0, 0, 0, 0], [0, I64_MAX, -1, I64_MIN], [0, 0, 0, I64_MIN],
     [DEFERRED, DEFERRED, DEFERRED, APPLIED], [0], [0]),
    ("one resource fits, the other does not", [10, 10], [10, 10], [0, 1, 0, 1], [5, 11, 5, 1], [11, 5, 10, 1],
     [DEFERRED, DEFERRED, APPLIED, APPLIED], [5, 9], [0, 9]),
]


@pytest.mark.parametrize("case", KNOWN, ids=[k[0] for k in KNOWN])
def test_int64_ends_and_signs(ev, ref, case):
    _, cpu, mem, b, rc, rm, st, cpu_after, mem_after = case
    c, m, want = check(ev, ref, labelled(np.random.default_rng(1), cpu, mem), b, rc, rm)
    assert want.tolist() == st and c.tolist() == cpu_after and m.tolist() == mem_after  # (the restatement against the hand-worked answer)


def test_sums_that_leave_int64_inside_a_chunk(ev, ref):
    """64 pods of 2^62 and -2^62 in turn on a node near INT64_MAX, and 70 pods of -2^61 on one at 0: the prefix of a chunk passes 2^63 several
    times over while every state of the walk stays inside int64; the run is repeated: same bits"""
    rng = np.random.default_rng(62)
    big = 1 << 62
    b = [0] * 64 + [1] * 70 + [2] * 64
    rc = [big, -big] * 32 + [-(1 << 61)] * 70 + [big] * 64
    rm = [-big, big] * 32 + [0] * 70 + [1] * 64
    cols = labelled(rng, [I64_MAX - 5, 0, I64_MAX], [big, 0, 10])
    first = check(ev, ref, cols, b, rc, rm)
    assert set(first[2].tolist()) == {APPLIED, DEFERRED, OVERFLOW}
    second = check(ev, ref, cols, b, rc, rm)
    assert all(np.array_equal(x, y) for x, y in zip(first, second))


# ---- 4. no over-commit, in rounds ---------------------------------------------------------------------------------------------------

def test_no_over_commit_rounds(ev):
    """six rounds of [sampled pick on the device -> apply WHILE_FIT -> retry the DEFERRED pods] against the same rounds on the host (the
    oracle's picks on the host's columns, then tests/admit_ref.py)"""
    N, P = 400, 6000
    c = synth.make_cluster(P, N, n_keys=8, seed=99)
    ev.set_nodes(**c.node_columns())
    rng = np.random.default_rng(11)
    flags = FIT | SEL | PICK_SAMPLED
    cpu, mem = c.avail_cpu.copy(), c.avail_mem.copy()
    floor_cpu, floor_mem = np.minimum(cpu, 0), np.minimum(mem, 0)
    pending = np.arange(P)
    admitted = []
    for rnd in range(6):
        if len(pending) == 0:  # (a deferred pod is evaluated again: it is admitted, deferred once more, or finds no node and leaves)
            break
        smp = rng.integers(0, N, (len(pending), 5)).astype(np.uint32)
        rc, rm, sel = c.req_cpu[pending], c.req_mem[pending], np.ascontiguousarray(c.pod_sel[:, pending])
        rc_t, rm_t = t(rc, np.int64), t(rm, np.int64)
        outb = torch.empty((len(pending),), dtype=torch.int32, device=DEV)
        st = torch.full((len(pending),), SENTINEL, dtype=torch.int32, device=DEV)
        ev.eval_device(rc_t, rm_t, t(sel, np.int32), None, t(smp, np.int32), flags, out_binding=outb)
        ev.apply_bindings_device(outb, rc_t, rm_t, flags=WF, status_out=st)
        b_dev, st = outb.cpu().numpy(), st.cpu().numpy()
        b_host = capi.eval_encoded(cpu, mem, c.node_labels, None, rc, rm, sel, None, smp, flags, want_mask=False)[2]
        assert np.array_equal(b_dev, b_host), f"round {rnd}: bindings"
        cpu, mem, want = apply_while_fit_exact(cpu, mem, b_host, rc, rm)
        assert np.array_equal(st, want), f"round {rnd}: statuses"
        got = ev.read_nodes()
        assert np.array_equal(got[0], cpu) and np.array_equal(got[1], mem), f"round {rnd}: columns"
        assert (got[0] >= floor_cpu).all() and (got[1] >= floor_mem).all(), f"round {rnd}: a node went below what it had"
        admitted.append(int((st == APPLIED).sum()))
        if rnd == 0:
            nodes = len(set(b_host[b_host >= 0].tolist()))
            print(f"round 1: {admitted[0]} admitted, {int((st == DEFERRED).sum())} deferred, {nodes} distinct nodes bound")
            assert admitted[0] == int((want == APPLIED).sum()) and admitted[0] > 4 * nodes
        pending = pending[st == DEFERRED]
    print(f"admitted per round {admitted}")
    assert len(admitted) >= 2 and admitted[1] > 0


# ---- 5. ordering --------------------------------------------------------------------------------------------------------------------

def test_eval_admit_eval_without_a_host_sync(built):
    """eval (mask + sampled pick) on stream A, apply WHILE_FIT of its bindings on A, eval on stream B, nothing waited for in between: the first
    mask is the oracle's on the old columns, the second the oracle's on the admitted ones"""
    N, P = 5000, 20_000
    c = synth.make_cluster(P, N, n_keys=8, seed=55)
    flags = FIT | SEL | PICK_SAMPLED
    smp = np.random.default_rng(5).integers(0, N, (P, 5)).astype(np.uint32)
    with Evaluator(0) as e:
        e.set_nodes(**c.node_columns())
        A, B = torch.cuda.Stream(), torch.cuda.Stream()
        rc_t, rm_t, sel_t, smp_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32), t(smp, np.int32)
        outs = [(torch.empty((P, e.W), dtype=torch.int64, device=DEV), torch.empty((P,), dtype=torch.int32, device=DEV)) for _ in range(2)]
        st = torch.full((P,), SENTINEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        e.eval_device(rc_t, rm_t, sel_t, None, smp_t, flags, out_feasible=outs[0][0], out_binding=outs[0][1], stream=A)
        e.apply_bindings_device(outs[0][1], rc_t, rm_t, flags=WF, status_out=st, stream=A)
        e.eval_device(rc_t, rm_t, sel_t, None, smp_t, flags, out_feasible=outs[1][0], out_binding=outs[1][1], stream=B)
        torch.cuda.synchronize()
        old = capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels, None, c.req_cpu, c.req_mem, c.pod_sel, None, smp, flags)
        assert np.array_equal(outs[0][0].cpu().numpy().view(np.uint64), old[0]) and np.array_equal(outs[0][1].cpu().numpy(), old[2])
        cpu, mem, want = apply_while_fit_exact(c.avail_cpu, c.avail_mem, old[2], c.req_cpu, c.req_mem)
        assert np.array_equal(st.cpu().numpy(), want) and (want == DEFERRED).sum() > 100
        new = capi.eval_encoded(cpu, mem, c.node_labels, None, c.req_cpu, c.req_mem, c.pod_sel, None, smp, flags)
        assert np.array_equal(outs[1][0].cpu().numpy().view(np.uint64), new[0]) and np.array_equal(outs[1][1].cpu().numpy(), new[2])
        assert not np.array_equal(old[0], new[0])
        e.forget_stream(A)
        e.forget_stream(B)


# ---- 6. the evaluation paths after an admit -----------------------------------------------------------------------------------------

def test_evaluation_paths_after_an_admit(built):
    """the fused and the direct kernel, the best-fit pick (its order is stale and rebuilt), the spread pick (it reads the columns' values) and
    ksched_summarize, each once after an apply WHILE_FIT, against the oracle or their restatements on the admitted columns"""
    N, P, Q = 4097, 3 * 4097 + 7, 1500
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=4097)
    base = FIT | SEL | TAINT
    rq = dict(rc=c.req_cpu[:Q], rm=c.req_mem[:Q], sel=np.ascontiguousarray(c.pod_sel[:, :Q]), tol=c.pod_tol[:Q])
    draws = np.random.default_rng(6).integers(0, 1 << 32, (Q, 5), dtype=np.uint64).astype(np.uint32)

    def oracle(cpu, mem, flags, samples=None):
        return capi.eval_encoded(cpu, mem, c.node_labels, c.node_taints, rq["rc"], rq["rm"], rq["sel"], rq["tol"], samples, flags)

    with Evaluator(0) as e:
        e.set_nodes(**c.node_columns())
        before = e.eval(rq["rc"], rq["rm"], rq["sel"], rq["tol"], None, base | PICK_BESTFIT)  # builds the best-fit order
        assert np.array_equal(before.binding, oracle(c.avail_cpu, c.avail_mem, base | PICK_BESTFIT)[2])
        b, ok = random_bindings(np.random.default_rng(4097), N, P)
        st = apply(e, b, c.req_cpu, c.req_mem, ok)
        cpu, mem, want = apply_while_fit_exact(c.avail_cpu, c.avail_mem, b, c.req_cpu, c.req_mem, ok)
        assert np.array_equal(st, want) and (want == DEFERRED).sum() > 100 and (want == APPLIED).sum() > 1000
        feas, _, best = oracle(cpu, mem, base | PICK_BESTFIT)
        assert not np.array_equal(feas, oracle(c.avail_cpu, c.avail_mem, base)[0])
        for kernel, name in ((_lib.KERNEL_FUSED, "fused"), (_lib.KERNEL_DIRECT, "direct")):
            e.set_option(_lib.OPT_KERNEL, kernel)
            got = e.eval(rq["rc"], rq["rm"], rq["sel"], rq["tol"], None, base)
            assert name in e.last_kernel, e.last_kernel
            assert np.array_equal(got.feasible, feas), name
        e.set_option(_lib.OPT_KERNEL, _lib.KERNEL_AUTO)
        got = e.eval(rq["rc"], rq["rm"], rq["sel"], rq["tol"], None, base | PICK_BESTFIT)
        assert np.array_equal(got.binding, best) and not np.array_equal(best, before.binding)
        got = e.eval(rq["rc"], rq["rm"], rq["sel"], rq["tol"], draws, base | PICK_SPREAD)
        assert np.array_equal(got.binding, spread_pick_blocks(feas, draws, N, mem, cpu))
        assert not np.array_equal(got.binding, spread_pick_blocks(feas, draws, N, c.avail_mem, c.avail_cpu))  # (stale values would show)
        counts = e.summarize(rq["rc"], rq["rm"], rq["sel"], rq["tol"], base)
        assert np.array_equal(counts, summary_ref.expected_counts(cpu, mem, c.node_labels, c.node_taints, rq["rc"], rq["rm"], rq["sel"], rq["tol"], base))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(built):
    c = synth.make_cluster(500, 1500, n_keys=8, seed=15)
    b = np.random.default_rng(15).integers(0, c.N, c.P).astype(np.int32)
    b_t, rc_t, rm_t = t(b, np.int32), t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    with Evaluator(0) as e:
        with pytest.raises(KschedError) as ei:  # before ksched_set_nodes
            e.apply_bindings_device(b_t, rc_t, rm_t, flags=WF)
        assert ei.value.code == _lib.E_STATE
        e.set_nodes(**c.node_columns())
        chk = e.index_checksum()
        for flags in (WF | _lib.APPLY_RELEASE, WF | _lib.APPLY_FIRST_PER_NODE, WF | 0x04, WF | 0x80, 0x04, 0x80, WF | 0x10):
            st = torch.full((c.P,), SENTINEL, dtype=torch.int32, device=DEV)
            with pytest.raises(KschedError) as ei:
                e.apply_bindings_device(b_t, rc_t, rm_t, flags=flags, status_out=st)
            assert ei.value.code == _lib.E_INVAL, hex(flags)
            got = e.read_nodes()
            assert np.array_equal(got[0], c.avail_cpu) and np.array_equal(got[1], c.avail_mem) and e.index_checksum() == chk, hex(flags)
            assert (st.cpu().numpy() == SENTINEL).all(), hex(flags)
        lib = e._lib
        assert lib.ksched_apply_bindings_device(e._h, 1, None, None, None, None, WF, None, None) == _lib.E_INVAL
        assert lib.ksched_apply_bindings_device(e._h, 0, None, None, None, None, WF, None, None) == _lib.OK  # p == 0: a no-op
        got = e.read_nodes()
        assert np.array_equal(got[0], c.avail_cpu) and np.array_equal(got[1], c.avail_mem) and e.index_checksum() == chk
        e.apply_bindings_device(b_t, rc_t, rm_t, flags=WF)  # status_out NULL
        cpu, mem, _ = apply_while_fit_exact(c.avail_cpu, c.avail_mem, b, c.req_cpu, c.req_mem)
        got = e.read_nodes()
        assert np.array_equal(got[0], cpu) and np.array_equal(got[1], mem) and not np.array_equal(cpu, c.avail_cpu)


def test_an_empty_snapshot_and_a_call_that_admits_nothing(ev, ref):
    """no node: every bound pod is BAD_NODE; and a call whose pods all ask for nothing, or for too much, leaves columns and index as they were"""
    ev.set_nodes(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    st = apply(ev, np.array([0, -1, 3], dtype=np.int32), i64([1, 1, 1]), i64([1, 1, 1]))
    assert st.tolist() == [BAD_NODE, UNBOUND, BAD_NODE]
    rng = np.random.default_rng(3)
    cols = labelled(rng, rng.integers(10, 20, 1500), rng.integers(10, 20, 1500))
    ev.set_nodes(**cols)
    chk = ev.index_checksum()
    b = rng.integers(0, 1500, 4000).astype(np.int32)
    rc = np.where(np.arange(4000) % 2 == 0, 0, 100).astype(np.int64)
    _, _, want = check(ev, ref, cols, b, rc, rc)
    assert set(want.tolist()) == {APPLIED, DEFERRED} and ev.index_checksum() == chk
