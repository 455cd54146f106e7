"""The best-fit pick on the pods that are hard for it -- the AND of their rows is sparse: several selective label keys, a value no
node carries (decided in the first stage without a scan), a cpu request only a handful of nodes can hold, no feasible node at all
(the scan runs to the end of the snapshot) -- at snapshot sizes where the scan spans several wave rounds, one and two stages, every
hand-over point of the first stage; all against the oracle."""
import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, SEL, SEL_NEVER, TAINT, _lib, synth
from oracle import capi

pytestmark = pytest.mark.gpu


def want_of(c, sel, req_cpu, req_mem, flags):
    return capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels, c.node_taints, req_cpu, req_mem, sel, c.pod_tol, None, flags | PICK_BESTFIT)[2]


@pytest.mark.parametrize("N", [700, 5_000, 40_000, 70_001])
def test_sparse_and_infeasible_pods_one_and_two_stages(evaluator, N):
    ev = evaluator
    P = 3000
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=1000 + N)
    rng = np.random.default_rng(N)
    sel = c.pod_sel.copy()
    req_cpu, req_mem = c.req_cpu.copy(), c.req_mem.copy()
    card = c.node_labels.max(axis=1)
    # sparse ANDs: every third pod constrains the three most selective keys with values nodes do carry
    for k in (5, 6, 7):
        sel[k, ::3] = rng.integers(1, int(card[k]) + 1, size=sel[k, ::3].shape)
    sel[7, 1::50] = SEL_NEVER                      # a value no node carries
    sel[6, 2::50] = np.uint32(int(card[6]) + 7)    # an id beyond the key's largest
    req_cpu[3::11] = np.sort(c.avail_cpu)[-3]       # only the few largest nodes can hold these
    req_cpu[4::97] = c.avail_cpu.max() + 1         # nothing can
    req_mem[5::89] = c.avail_mem.max() + 1
    ev.set_nodes(**c.node_columns())
    try:
        for flags in (FIT | SEL | TAINT, FIT | SEL, SEL | TAINT, FIT):
            want = want_of(c, sel, req_cpu, req_mem, flags)
            for stages in (2, 1):
                ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)
                # bits 12-15: the first stage hands over after this many 64-byte blocks of candidate words (default 2); bit 11: unused since round 3
                for dbg in ((0, 1 << 12, 2 << 12, 3 << 12, 5 << 12, 15 << 12) if stages == 2 else (0,)):
                    ev.set_option(_lib.OPT_DEBUG, dbg)
                    r = ev.eval(req_cpu, req_mem, sel, c.pod_tol, None, flags | PICK_BESTFIT, want_mask=False)
                    assert np.array_equal(r.binding, want), (N, flags, stages, hex(dbg), int((r.binding != want).sum()))
        assert (want_of(c, sel, req_cpu, req_mem, FIT | SEL | TAINT) == -1).sum() > P // 100  # the case this test is about exists
    finally:
        ev.set_option(_lib.OPT_DEBUG, 0)
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)


@pytest.mark.parametrize("what", ["nothing_fits", "only_the_largest_nodes"])
def test_every_pod_handed_over(evaluator, what):
    """Every pod of the batch is still undecided after the first stage (its cpu request excludes all, or all but the few largest, nodes): the
    hand-over sub-lists fill to their capacity and the second stage's grid (a quarter of it) walks them; all against the oracle."""
    ev = evaluator
    P, N = 20_000, 20_000
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=4242)
    req_cpu = np.full(P, c.avail_cpu.max() + (1 if what == "nothing_fits" else 0), dtype=np.int64)
    req_mem = np.minimum(c.req_mem, np.sort(c.avail_mem)[N // 4])  # (so that `start` is early and the scan is long)
    sel = np.zeros_like(c.pod_sel)
    ev.set_nodes(**c.node_columns())
    try:
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 2)
        for flags in (FIT | TAINT, FIT):
            want = want_of(c, sel, req_cpu, req_mem, flags)
            for _ in range(4):  # (the counter sets rotate over three slots)
                r = ev.eval(req_cpu, req_mem, sel, c.pod_tol, None, flags | PICK_BESTFIT, want_mask=False)
                assert np.array_equal(r.binding, want), (what, flags, int((r.binding != want).sum()))
            assert ((want == -1).all() if what == "nothing_fits" else (want >= 0).any())
    finally:
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)


def test_two_stage_pick_after_snapshot_updates_many_calls(evaluator):
    """ksched_update_nodes marks the best-fit structures stale; the hand-over counters (128 sub-lists) rotate over three sets (each call zeroes
    the next call's set instead of a memset launch): many consecutive two-stage calls stay == oracle."""
    ev = evaluator
    c = synth.make_cluster(2000, 9000, n_keys=8, n_taints=16, seed=77)
    rng = np.random.default_rng(5)
    cpu, mem = c.avail_cpu.copy(), c.avail_mem.copy()
    ev.set_nodes(cpu, mem, c.node_labels, c.node_taints)
    ev.set_option(_lib.OPT_BESTFIT_STAGES, 2)
    try:
        for step in range(7):
            want = capi.eval_encoded(cpu, mem, c.node_labels, c.node_taints, c.req_cpu, c.req_mem, c.pod_sel, c.pod_tol, None, FIT | SEL | TAINT | PICK_BESTFIT)[2]
            r = ev.eval(c.req_cpu, c.req_mem, c.pod_sel, c.pod_tol, None, FIT | SEL | TAINT | PICK_BESTFIT, want_mask=False)
            assert np.array_equal(r.binding, want), step
            idx = rng.choice(c.N, size=400, replace=False).astype(np.uint32)
            cpu[idx] = rng.integers(0, 64_000, size=idx.size)
            mem[idx] = rng.integers(0, 1 << 37, size=idx.size)
            ev.update_nodes(idx, cpu[idx], mem[idx])
    finally:
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)


def handed_over(c, req_mem, sel, want, lane_blocks):
    """Which pods the first stage of the two-stage pick hands over, worked out on the host.  A lane looks at the best-fit positions from
    `start` (the first whose memory holds the pod) to the end of the lane_blocks-th 512-position block counted from start's; it hands the
    pod over when the oracle's winner lies beyond that edge (or there is none) and the edge is not the end of the rows (whole 64-byte
    lines of 512 positions).  A required label value no node carries is decided at once."""
    N = c.N
    rows_end = (((N + 63) // 64 + 7) & ~7) * 64
    order = np.lexsort((np.arange(N), c.avail_cpu, c.avail_mem))  # ascending (mem, cpu, node)
    rank = np.empty(N, dtype=np.int64)
    rank[order] = np.arange(N)
    start = np.searchsorted(c.avail_mem[order], req_mem, side="left")
    edge = ((start >> 9) + lane_blocks) * 512
    pos = np.where(want >= 0, rank[np.maximum(want, 0)], N)
    never = ((sel != 0) & (sel > c.node_labels.max(axis=1)[:, None])).any(axis=0)
    return (start < N) & ~never & (edge < rows_end) & (pos >= edge)


def test_handover_buffer_grows_between_two_stage_calls(evaluator):
    """The hand-over buffer of the two-stage pick is reallocated while its counter sets rotate: its mask region grows past 512 pods and
    moves the records behind it, the sub-lists' records grow past 8192 pods, and a fresh allocation zeroes all counters and restarts the
    rotation at set 0.  The batches are prefixes of one 9000-pod batch (a pod's binding does not depend on the rest of its batch: the
    oracle's bindings of a prefix are the prefix of its bindings); every third pod asks for the third-largest cpu.  At 700 nodes a row
    is 16 words, which the first stage's default two 64-byte blocks cover whole -- it would hand nothing over -- so the hand-over point
    is set to ONE block (OPT_DEBUG bits 12-15 = 1): pods whose memory fits within the first 512 best-fit positions and whose winner,
    if any, lies beyond them go to the second stage.  handed_over() checks that premise for every call.  (The snapshot has no list key:
    the mask region is sized but not written.)  The bindings are written into a buffer pre-filled with a sentinel, so a pod the second
    stage never reaches shows."""
    import torch

    ev = evaluator
    P, N = 9000, 700
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=1000 + N)
    req_cpu = c.req_cpu.copy()
    req_cpu[::3] = np.sort(c.avail_cpu)[-3]
    flags = FIT | SEL | TAINT
    want = want_of(c, c.pod_sel, req_cpu, c.req_mem, flags)
    handed = handed_over(c, c.req_mem, c.pod_sel, want, lane_blocks=1)
    assert not handed_over(c, c.req_mem, c.pod_sel, want, lane_blocks=2).any()  # (why the hand-over point is moved)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    ev.set_nodes(**c.node_columns())
    ev.set_option(_lib.OPT_BESTFIT_STAGES, 2)
    ev.set_option(_lib.OPT_DEBUG, 1 << 12)
    try:
        for call, p in enumerate((64, 64, 600, 64, 9000, 9000, 64, 64, 64)):
            assert handed[:p].sum() >= p // 4, (p, int(handed[:p].sum()))  # the second stage has pods in every call ...
            assert p == 64 or (handed[:p] & (want[:p] >= 0)).sum() >= 6      # ... and binds some of them in the larger ones
            out = torch.full((p,), -7, dtype=torch.int32, device=dev)
            ev.eval_device(t(req_cpu[:p], np.int64), t(c.req_mem[:p], np.int64), t(c.pod_sel[:, :p], np.int32), t(c.pod_tol[:p], np.int64), None,
                           flags | PICK_BESTFIT, out_binding=out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert ev.last_pick == "bestfit-rows", (call, p, ev.last_pick)
            assert np.array_equal(got, want[:p]), (call, p, int((got != want[:p]).sum()), int((got == -7).sum()))
    finally:
        ev.set_option(_lib.OPT_DEBUG, 0)
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)


@pytest.mark.parametrize("N", [1, 8, 9, 64, 65, 512, 513])
def test_level_array_boundaries(evaluator, N):
    """Snapshots at the sizes where the lane-per-pod searches gain a level array (more than 8, 64, 512 nodes) and below the first one:
    one and two stages against the oracle, from the rows (never the from-mask route: the snapshots have a bitmap index)."""
    ev = evaluator
    P = 200
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=2000 + N)
    ev.set_nodes(**c.node_columns())
    try:
        for flags in (FIT | SEL | TAINT, FIT):
            want = want_of(c, c.pod_sel, c.req_cpu, c.req_mem, flags)
            for stages in (1, 2):
                ev.set_option(_lib.OPT_BESTFIT_STAGES, stages)
                r = ev.eval(c.req_cpu, c.req_mem, c.pod_sel, c.pod_tol, None, flags | PICK_BESTFIT, want_mask=False)
                assert ev.last_pick == "bestfit-rows", (N, flags, stages, ev.last_pick)
                assert np.array_equal(r.binding, want), (N, flags, stages, int((r.binding != want).sum()))
    finally:
        ev.set_option(_lib.OPT_BESTFIT_STAGES, 0)
