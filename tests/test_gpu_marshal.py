"""The pointers and the row pitch the Python binding hands to the library, checked on the GPU at the smallest shapes at which a wrong one
shows: 130 nodes = 3 mask words, rows of a library mask 16 words apart (ksched_mask_pitch), so packed and pitched rows differ and the
padding is live; 0, 1 and 9 pods (one unit of eight plus one).  Every device entry point, in its unbound and its bound form, into a
library mask, a pitched and a packed torch buffer, against the oracle; and a refused call leaves the pipe as it was.

The mask kernels may write zeros into a row's padding words (tests/test_gpu_parity.py::test_pitched_device_masks), so the padding is
"zero or untouched" and the out-of-bounds check proper is a guard region behind the last row (and behind the last binding).

No pods: an empty torch tensor has no address (data_ptr() is 0) and the library refuses a pick that has no binding buffer, whatever the
pod count (check_eval_args, ksched_pick_device).  So with 0 pods every form that picks raises KschedError(E_INVAL) -- the library's own
refusal, the shapes are right -- and must leave every buffer as it was; the summaries, which take no pick, succeed.
"""
import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, PICK_SAMPLED, PICK_UNIFORM, SEL, TAINT, KschedError, _lib, synth
from oracle import capi
from tests.uniform_ref import uniform_pick

pytestmark = pytest.mark.gpu

N, PODS, PREDS = 130, [0, 1, 9], FIT | SEL | TAINT
PICKS = {"sampled": PICK_SAMPLED, "bestfit": PICK_BESTFIT, "uniform": PICK_UNIFORM}
LAYOUTS = ["library", "pitched", "packed"]
GUARD_ROWS, FILL, SENTINEL, UNSET = 2, 0x5A, 0x5A5A5A5A5A5A5A5A, -7
_CASES = {}


def case(P):
    """the cluster, the oracle's mask, and per pick the draws and the expected bindings: computed once per pod count"""
    if P not in _CASES:
        c = synth.make_cluster(P, N, n_keys=2, n_taints=3, seed=1300 + P)
        enc = lambda smp, flags: capi.eval_encoded(c.avail_cpu, c.avail_mem, c.node_labels, c.node_taints, c.req_cpu, c.req_mem,  # noqa: E731
                                                   np.ascontiguousarray(c.pod_sel), c.pod_tol, smp, flags)
        feas = enc(None, PREDS)[0]
        draws = np.random.default_rng(P).integers(0, 1 << 32, size=(P, 5), dtype=np.uint64).astype(np.uint32)
        smp = {"sampled": np.ascontiguousarray(c.samples), "bestfit": None, "uniform": draws}
        want = {"sampled": enc(smp["sampled"], PREDS | PICK_SAMPLED)[2], "bestfit": enc(None, PREDS | PICK_BESTFIT)[2],
                "uniform": uniform_pick(feas, draws[:, 0], N)}
        for a in (feas, *want.values()):
            a.setflags(write=False)
        _CASES[P] = dict(c=c, feas=feas, smp=smp, want=want)
    return _CASES[P]


@pytest.fixture
def ev(evaluator):
    evaluator.set_kernel("auto")
    evaluator.set_option(_lib.OPT_PIPE_MODE, 0)
    return evaluator


def dev_of(ev):
    import torch
    return torch.device("cuda", ev.device)


def to_dev(ev, a, dt):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C").view(dt)).to(dev_of(ev))


def batch(ev, k, pick):
    c = k["c"]
    return (to_dev(ev, c.req_cpu, np.int64), to_dev(ev, c.req_mem, np.int64), to_dev(ev, c.pod_sel, np.int32), to_dev(ev, c.pod_tol, np.int64),
            to_dev(ev, k["smp"][pick], np.int32))


def picked(P, run):
    """run() for a batch of P pods whose flags carry a pick (see the module's docstring for no pods)"""
    if P > 0:
        return run()
    with pytest.raises(KschedError) as e:
        run()
    assert e.value.code == _lib.E_INVAL


class Mask:
    """A [P, W] mask view in one layout over sentinel-filled memory: `library` = Evaluator.alloc_mask (rows at ksched_mask_pitch, no room for a
    guard), `pitched` / `packed` = a torch buffer with rows at that pitch / W words apart and GUARD_ROWS further rows behind the last one."""

    def __init__(self, ev, P, layout):
        import torch
        self.P, self.W = P, ev.W
        if layout == "library":
            self.view = ev.alloc_mask(P)
            self.view.untyped_storage().fill_(FILL)
            self.pitch, self.buf = int(ev._lib.ksched_mask_pitch(ev.n)), None
        else:
            self.pitch = int(ev._lib.ksched_mask_pitch(ev.n)) if layout == "pitched" else ev.W
            self.buf = torch.empty((P + GUARD_ROWS, self.pitch), dtype=torch.int64, device=dev_of(ev))
            self.buf.untyped_storage().fill_(FILL)
            self.view = self.buf[:P, :ev.W]
        if P > 1:
            assert self.view.stride(0) == self.pitch

    def check(self, feas, what):
        import torch
        assert np.array_equal(self.view.contiguous().cpu().numpy().view(np.uint64), feas), f"{what}: mask"
        if self.buf is not None:
            assert (self.buf[self.P:].cpu().numpy().view(np.uint64) == SENTINEL).all(), f"{what}: rows behind the last one were written"
            rows = self.buf[:self.P]
        else:
            rows = torch.as_strided(self.view, (self.P, self.pitch), (self.pitch, 1))
        pad = rows[:, self.W:].cpu().numpy().view(np.uint64)
        assert np.isin(pad, np.array([0, SENTINEL], dtype=np.uint64)).all(), f"{what}: padding words"


class Guarded:
    """a tensor of `shape` in front of four further rows, everything filled with `fill`: the rows behind it are the guard"""

    def __init__(self, ev, shape, dtype, fill):
        import torch
        self.buf = torch.full((shape[0] + 4,) + tuple(shape[1:]), fill, dtype=dtype, device=dev_of(ev))
        self.view, self.fill, self.rows = self.buf[:shape[0]], fill, shape[0]

    def check(self, want, what):
        got = self.buf.cpu().numpy()
        assert np.array_equal(got[:self.rows].view(want.dtype), want), what
        assert (got[self.rows:] == self.fill).all(), f"{what}: written behind its end"


def test_the_shapes_are_the_ones_that_tell(ev):
    ev.set_nodes(**case(9)["c"].node_columns())
    assert ev.W == 3 and ev._lib.ksched_mask_pitch(N) == 16 and ev.alloc_mask(9).stride(0) == 16 and ev.alloc_mask(9, pitched=False).stride(0) == 3


@pytest.mark.parametrize("P", PODS)
@pytest.mark.parametrize("pick", list(PICKS))
def test_masks_and_bindings_of_every_entry_point(ev, pick, P):
    """eval_device, bind_eval_device(...)(0, 0), Pipe.submit and Pipe.bind(...)(slot), each waited for, into each mask layout"""
    import torch
    k = case(P)
    ev.set_nodes(**k["c"].node_columns())
    flags = PREDS | PICKS[pick]
    d = batch(ev, k, pick)
    pipe = ev.pipe(2)
    try:
        def through_pipe(submit, slot):
            submit()
            pipe.wait(slot, host=True)
            pipe.wait_mask(slot, host=True)
        forms = {
            "eval_device": lambda m, b: ev.eval_device(*d, flags, out_feasible=m, out_binding=b),
            "bind_eval_device": lambda m, b: ev.bind_eval_device(*d, flags, out_feasible=[m], out_bindings=[b])(0, 0),
            "Pipe.submit": lambda m, b: through_pipe(lambda: pipe.submit(1, *d, flags, m, b), 1),
            "Pipe.bind": lambda m, b: through_pipe(lambda: pipe.bind(*d, flags, [m, m], [b, b])(0), 0),
        }
        for layout in LAYOUTS:
            for name, run in forms.items():
                what = f"{name}, {layout} mask, {P} pods, {pick}"
                m, b = Mask(ev, P, layout), Guarded(ev, (P,), torch.int32, UNSET)
                picked(P, lambda: run(m.view, b.view))
                torch.cuda.synchronize()
                m.check(k["feas"], what)
                b.check(k["want"][pick], f"{what}: bindings")
    finally:
        pipe.close()


@pytest.mark.parametrize("P", PODS)
def test_pick_device_and_summarize_device(ev, P):
    """the pick alone from a mask in each layout == Evaluator.pick == the oracle; the summary table == Evaluator.summarize"""
    import torch
    k = case(P)
    c = k["c"]
    ev.set_nodes(**c.node_columns())
    mem = to_dev(ev, c.req_mem, np.int64)
    for layout in LAYOUTS:
        m = Mask(ev, P, layout)
        m.view.copy_(to_dev(ev, k["feas"], np.int64))
        for pick, bit in PICKS.items():
            what = f"pick_device, {layout} mask, {P} pods, {pick}"
            b = Guarded(ev, (P,), torch.int32, UNSET)
            picked(P, lambda: ev.pick_device(m.view, bit | FIT, b.view, req_mem_bytes=mem, samples=to_dev(ev, k["smp"][pick], np.int32)))
            torch.cuda.synchronize()
            b.check(k["want"][pick], what)
            assert np.array_equal(ev.pick(k["feas"], bit | FIT, req_mem_bytes=c.req_mem, samples=k["smp"][pick]), k["want"][pick]), f"{what}: Evaluator.pick"
        m.check(k["feas"], f"pick_device, {layout} mask")  # (read only)
    table = Guarded(ev, (P, _lib.SUMMARY_WORDS), torch.int32, UNSET)
    pc = c.pod_columns()
    want = ev.summarize(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], PREDS)
    assert want.shape == (P, _lib.SUMMARY_WORDS) and (want.sum(axis=1) == N).all()
    assert np.array_equal(want[:, 0], np.array([bin(int(w)).count("1") for w in k["feas"].reshape(-1)], dtype=np.uint32).reshape(P, ev.W).sum(axis=1))
    assert ev.summarize_device(*batch(ev, k, "bestfit")[:4], PREDS, out=table.view) is table.view
    torch.cuda.synchronize()
    table.check(want, f"summarize_device, {P} pods")


def test_a_refused_submit_does_no_damage(ev):
    """A [P, W - 1] mask and a [P - 1] binding buffer are refused before any library call; the slot then serves a valid submit."""
    import torch
    P = 9
    k = case(P)
    ev.set_nodes(**k["c"].node_columns())
    flags = PREDS | PICK_SAMPLED
    d = batch(ev, k, "sampled")
    pipe = ev.pipe(2)
    try:
        m, b = Mask(ev, P, "pitched"), Guarded(ev, (P,), torch.int32, UNSET)
        with pytest.raises(ValueError, match="mask"):
            pipe.submit(0, *d, flags, m.buf[:P, :ev.W - 1], b.view)
        with pytest.raises(ValueError, match="binding"):
            pipe.submit(0, *d, flags, m.view, b.view[:P - 1])
        with pytest.raises(ValueError, match="binding"):
            pipe.bind(*d, flags, [m.view], [b.view[:P - 1]])
        torch.cuda.synchronize()
        assert (m.buf.cpu().numpy().view(np.uint64) == SENTINEL).all() and (b.buf.cpu().numpy() == UNSET).all(), "a refused call wrote something"
        pipe.submit(0, *d, flags, m.view, b.view)
        pipe.wait(0, host=True)
        pipe.wait_mask(0, host=True)
        torch.cuda.synchronize()
        m.check(k["feas"], "the submit after the refusals")
        b.check(k["want"]["sampled"], "the submit after the refusals: bindings")
    finally:
        pipe.close()
