"""The binding's argument checks (kube_scheduler_rs_reference_amd/_marshal.py) without a GPU and without ksched_create.

The C ABI takes bare pointers, so these checks are what stands between a wrong shape and an out-of-bounds device access.  A stand-in
tensor (a CPU torch tensor that reports itself as a CUDA tensor) reaches every rule; a recording stub in place of the loaded library
shows that a refused call reaches no library function and that a valid one passes exactly the expected pointers, counts and pitch.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from kube_scheduler_rs_reference_amd import _lib as L
from kube_scheduler_rs_reference_amd import _marshal as M
from kube_scheduler_rs_reference_amd.dist import AbiComm, LocalClique
from kube_scheduler_rs_reference_amd.evaluator import Evaluator, Pipe, _apply_args

N_KEYS, N_NODES, W, A = 2, 130, 3, 5  # 130 nodes = 3 mask words; 5 draws per pod
PREDS = L.FIT | L.SEL | L.TAINT


class FakeCuda:
    """A CPU torch tensor seen as a CUDA tensor of device `index`; `strides` overrides what stride() reports."""

    def __init__(self, t, index=0, is_cuda=True, strides=None):
        self.t, self.is_cuda, self.device, self._strides = t, is_cuda, SimpleNamespace(index=index), strides
        self.dtype, self.shape = t.dtype, t.shape

    def stride(self, dim=None):
        s = self._strides or self.t.stride()
        return tuple(s) if dim is None else s[dim]

    def is_contiguous(self):
        return self.t.is_contiguous() if self._strides is None else False

    def data_ptr(self):
        return self.t.data_ptr()


def dev(shape, dtype, **kw):
    return FakeCuda(torch.zeros(tuple(shape), dtype=dtype), **kw)


def strided(shape, dtype):
    """the same shape with every second element of the last dimension: column stride 2"""
    return FakeCuda(torch.zeros(tuple(shape[:-1]) + (2 * shape[-1],), dtype=dtype)[..., ::2])


def pitched(p, w, pitch, dtype=torch.int64):
    return FakeCuda(torch.zeros((max(p, 1), pitch), dtype=dtype)[:p, :w])


# ---- 1. the rules, role by role ------------------------------------------------------------------------------------------------------
def roles(p):
    """(argument name, accepted dtypes, a refused dtype, shape, check(tensor) -> address) for every role a device tensor can play"""
    good_mask = dev((p, W), torch.int64)
    one = lambda name, kind, shape: (lambda t: M.device_ptr(t, name, kind, shape, 0))  # noqa: E731
    return [
        ("req_cpu_milli", (torch.int64,), torch.int32, (p,), one("req_cpu_milli", "i64", (p,))),
        ("req_mem_bytes", (torch.int64,), torch.uint64, (p,), one("req_mem_bytes", "i64", (p,))),
        ("sel_val_ids", (torch.int32, torch.uint32), torch.int64, (N_KEYS, p), one("sel_val_ids", "u32", (N_KEYS, p))),
        ("tolerations", (torch.int64, torch.uint64), torch.int32, (p,), one("tolerations", "u64", (p,))),
        ("samples", (torch.int32, torch.uint32), torch.int64, (p, A), lambda t: M.draws(t, "samples", L.PICK_SAMPLED, p, 0)[0].value),
        ("out_feasible", (torch.int64, torch.uint64), torch.int32, (p, W), lambda t: M.mask_rows(p, W, 0, ("out_feasible", t))[0][0]),
        ("out_fit", (torch.int64, torch.uint64), torch.float64, (p, W),
         lambda t: M.mask_rows(p, W, 0, ("out_feasible", good_mask), ("out_fit", t))[0][1]),
        ("out_binding", (torch.int32,), torch.uint32, (p,), one("out_binding", "i32", (p,))),
        ("ok", (torch.uint8, torch.bool), torch.int8, (p,), one("ok", "u8", (p,))),
        ("status_out", (torch.int32,), torch.int64, (p,), one("status_out", "i32", (p,))),
        ("out", (torch.int32, torch.uint32), torch.int64, (p, L.SUMMARY_WORDS), one("out", "u32", (p, L.SUMMARY_WORDS))),
        ("local", (torch.int32,), torch.int64, (p,), one("local", "i32", (p,))),
        ("gathered", (torch.int32,), torch.int16, (2 * p,), one("gathered", "i32", (2 * p,))),
    ]


ROLE_NAMES = [r[0] for r in roles(2)]
MASK_ROLES = ("out_feasible", "out_fit")


@pytest.mark.parametrize("p", [1, 2, 9])
@pytest.mark.parametrize("role", ROLE_NAMES)
def test_valid_tensor_gives_its_address(role, p):
    name, dtypes, _, shape, check = roles(p)[ROLE_NAMES.index(role)]
    for dt in dtypes:
        t = dev(shape, dt)
        assert check(t) == t.data_ptr() != 0
    assert role == "samples" or check(None) is None, "an absent tensor is a null pointer"


def violations(name, dtypes, bad_dtype, shape):
    dt = dtypes[0]
    out = {"not CUDA": dev(shape, dt, is_cuda=False), "other device": dev(shape, dt, index=1), "wrong dtype": dev(shape, bad_dtype),
           "wrong rank": dev(shape + (1,), dt), "one row more": dev((shape[0] + 1,) + shape[1:], dt),
           "one row fewer": dev((shape[0] - 1,) + shape[1:], dt), "last dimension short by one": dev(shape[:-1] + (shape[-1] - 1,), dt),
           "column stride 2": strided(shape, dt)}
    if name in MASK_ROLES:
        out["flattened"] = dev((shape[0] * shape[1],), dt)
        out["rows closer than W"] = FakeCuda(torch.zeros(shape, dtype=dt), strides=(W - 1, 1))
    if name == "samples":  # any number of draws per pod but none
        del out["last dimension short by one"]
        out["zero columns"] = dev((shape[0], 0), dt)
    return out


@pytest.mark.parametrize("role", ROLE_NAMES)
def test_each_violated_rule_is_refused_by_name(role):
    """not CUDA, other device, non-contiguous (masks: column stride 2), wrong dtype, wrong rank, wrong shape by one"""
    name, dtypes, bad_dtype, shape, check = roles(2)[ROLE_NAMES.index(role)]
    for what, t in violations(name, dtypes, bad_dtype, shape).items():
        with pytest.raises(ValueError, match=name):
            check(t)
            pytest.fail(f"{name}: {what} was accepted")


def test_masks_of_one_call_share_one_pitch():
    a, b = pitched(2, W, 16), pitched(2, W, 16)
    assert M.mask_rows(2, W, 0, ("out_feasible", a), ("out_fit", b)) == ([a.data_ptr(), b.data_ptr()], 16)
    with pytest.raises(ValueError, match="out_fit"):
        M.mask_rows(2, W, 0, ("out_feasible", a), ("out_fit", dev((2, W), torch.int64)))
    # a single row has no pitch of its own: a pitched and a packed one-row mask go together, at pitch W
    a1, b1 = pitched(1, W, 16), dev((1, W), torch.int64)
    assert M.mask_rows(1, W, 0, ("out_feasible", a1), ("out_fit", b1)) == ([a1.data_ptr(), b1.data_ptr()], W)


@pytest.mark.parametrize("p,w,pitch,want", [(0, 3, 16, 3), (1, 3, 16, 3), (2, 3, 3, 3), (2, 3, 16, 16), (9, 3, 16, 16), (9, 3, 3, 3),
                                            (2, 0, 1, 1), (1, 0, 1, 0), (0, 0, 1, 0)])
def test_mask_pitch_at_the_edge_shapes(p, w, pitch, want):
    """p = 0 / 1 / 2 / 9, W = 0 (no nodes) / 3 packed / 3 at pitch 16; for p <= 1 the pitch is W whatever the tensor's strides say"""
    m = pitched(p, w, pitch)
    ptrs, got = M.mask_rows(p, w, 0, ("mask", m))
    assert got == want and ptrs == [m.data_ptr() or None]
    assert M.mask_rows(p, w, 0, ("mask", None)) == ([None], w)


def test_one_row_mask_with_a_nonsense_stride():
    t = torch.zeros((1, W), dtype=torch.int64)
    for s0 in (0, 1, 10 ** 9):
        assert M.mask_rows(1, W, 0, ("mask", FakeCuda(t, strides=(s0, 1)))) == ([t.data_ptr()], W)


@pytest.mark.parametrize("pick", [L.PICK_SAMPLED, L.PICK_UNIFORM])
def test_draws_are_required_exactly_with_a_drawing_pick(pick):
    p = 2
    good = dev((p, A), torch.int32)
    for device, smp in ((0, good), (None, np.zeros((p, A), np.uint32))):
        ptr, attempts, _ = M.draws(smp, "samples", PREDS | pick, p, device)
        assert attempts == A and ptr.value == (smp.data_ptr() if device == 0 else smp.ctypes.data)
        with pytest.raises(ValueError, match="samples"):
            M.draws(None, "samples", PREDS | pick, p, device)
        # without a drawing pick nothing reads them: no draws, or draws of any shape, give attempts = 0
        assert M.draws(None, "samples", PREDS | L.PICK_BESTFIT, p, device)[:2] == (None, 0)
        assert M.draws(smp, "samples", PREDS, p + 1, device)[1] == 0
    for bad in (np.zeros((p, 0), np.uint32), np.zeros((p - 1, A), np.uint32), np.zeros((p + 1, A), np.uint32), np.zeros((p * A,), np.uint32)):
        with pytest.raises(ValueError, match="samples"):
            M.draws(bad, "samples", pick, p)
    assert M.draws(np.zeros((p, 2 * A), np.uint32)[:, ::2].tolist(), "samples", pick, p)[1] == A  # lists and strided arrays are converted


def test_apply_args_are_the_device_check():
    ev = SimpleNamespace(device=0)
    p = 3
    t = {n: dev((p,), dt) for n, dt in (("b", torch.int32), ("c", torch.int64), ("m", torch.int64), ("ok", torch.bool), ("st", torch.int32))}
    assert _apply_args(ev, t["b"], t["c"], t["m"], t["ok"], t["st"]) == (p, *[t[n].data_ptr() for n in ("b", "c", "m", "ok", "st")])
    assert _apply_args(ev, t["b"], t["c"], t["m"], None, None)[4:] == (None, None)
    for name, args in (("req_mem", (t["b"], t["c"], dev((p - 1,), torch.int64), None, None)), ("ok", (t["b"], t["c"], t["m"], dev((p,), torch.int32), None)),
                       ("status_out", (t["b"], t["c"], t["m"], None, dev((p,), torch.int32, index=1))), ("bindings", (dev((p, 1), torch.int32), t["c"], t["m"], None, None))):
        with pytest.raises(ValueError, match=name):
            _apply_args(ev, *args)


# ---- 2. the entry points over a recording stub ---------------------------------------------------------------------------------------
class Recorder:
    """Stands where the loaded library stands: every function records (name, argument values) and returns KSCHED_OK."""

    def __init__(self):
        self.calls, self.arrays = [], []

    def __getattr__(self, name):
        def fn(*args):
            if name == "ksched_allgather_bindings_local":  # its per-rank pointer arrays live only as long as the call
                self.arrays = [list(C.cast(args[i], C.POINTER(C.c_void_p * args[1])).contents) for i in (2, 3)]
            self.calls.append((name, tuple(a.value if isinstance(a, C._SimpleCData) else a for a in args)))
            return 0
        return fn


H, HP, HC, STREAM = 0x1000, 0x2000, 0x3000, SimpleNamespace(cuda_stream=0x77)


def make_evaluator():
    ev = Evaluator.__new__(Evaluator)
    ev._lib, ev._h, ev.device, ev.n, ev.n_keys = Recorder(), H, 0, N_NODES, N_KEYS
    return ev


def make_pipe(ev):
    pipe = Pipe.__new__(Pipe)
    pipe.ev, pipe.depth, pipe._lib, pipe._h = ev, 2, ev._lib, HP
    return pipe


def make_comm(ev, world=2):
    comm = AbiComm.__new__(AbiComm)
    comm._lib, comm._ev, comm._h, comm.rank, comm.world = ev._lib, ev, HC, 0, world
    return comm


def device_args(p, pick=L.PICK_SAMPLED, pitch=16):
    a = dict(cpu=dev((p,), torch.int64), mem=dev((p,), torch.int64), sel=dev((N_KEYS, p), torch.int32), tol=dev((p,), torch.uint64),
             smp=dev((p, A), torch.uint32), mask=pitched(p, W, pitch), fit=pitched(p, W, pitch), bind=dev((p,), torch.int32),
             table=dev((p, L.SUMMARY_WORDS), torch.int32), flags=PREDS | pick)
    a["attempts"] = A if pick & M.DRAWS else 0
    a["pitch"] = pitch if p > 1 else W
    return a


def ptrs(a, *names):
    return tuple(a[n].data_ptr() or None for n in names)


def calls_of(ev):
    return [c for c in ev._lib.calls if c[0] != "ksched_destroy"]


@pytest.mark.parametrize("pick", [L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_UNIFORM])
@pytest.mark.parametrize("p", [0, 1, 2, 9])
def test_device_entry_points_pass_exactly_the_checked_arguments(p, pick):
    ev = make_evaluator()
    a = device_args(p, pick)
    batch = (a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"])
    head = (p, *ptrs(a, "cpu", "mem", "sel", "tol", "smp"), a["attempts"], a["flags"])
    ev.eval_device(*batch, a["flags"], out_feasible=a["mask"], out_fit=a["fit"], out_binding=a["bind"], stream=STREAM)
    want = ("ksched_eval_device_pitched", (H, *head, *ptrs(a, "mask", "fit", "bind"), a["pitch"], STREAM.cuda_stream))
    assert calls_of(ev) == [want]
    ev.bind_eval_device(*batch, a["flags"], out_feasible=[a["mask"]], out_fit=a["fit"], out_bindings=[a["bind"]], stream=STREAM)(0, 0)
    assert calls_of(ev) == [want, want], "the bound and the unbound form pass the same argument tuple"

    pipe = make_pipe(ev)
    want = ("ksched_pipe_submit", (HP, 1, *head, *ptrs(a, "mask"), a["pitch"], *ptrs(a, "bind")))
    pipe.submit(1, *batch, a["flags"], a["mask"], a["bind"])
    pipe.bind(*batch, a["flags"], [a["fit"], a["mask"]], [None, a["bind"]])(1)
    assert calls_of(ev)[2:] == [want, want]

    ev.summarize_device(a["cpu"], a["mem"], a["sel"], a["tol"], PREDS, out=a["table"], stream=STREAM)
    assert calls_of(ev)[4:] == [("ksched_summarize_device", (H, *head[:5], PREDS, *ptrs(a, "table"), STREAM.cuda_stream))]
    ev.pick_device(a["mask"], pick | L.FIT, a["bind"], req_mem_bytes=a["mem"], samples=a["smp"], stream=STREAM)
    assert calls_of(ev)[5:] == [("ksched_pick_device", (H, p, *ptrs(a, "mask"), a["pitch"], *ptrs(a, "mem", "smp"), a["attempts"], pick | L.FIT,
                                                        *ptrs(a, "bind"), STREAM.cuda_stream))]


def test_no_label_keys_and_no_selectors():
    ev = make_evaluator()
    ev.n_keys = 0
    a = device_args(2, L.PICK_BESTFIT, pitch=W)
    ev.eval_device(a["cpu"], a["mem"], None, None, None, L.FIT | L.PICK_BESTFIT, out_binding=a["bind"], stream=STREAM)
    assert calls_of(ev) == [("ksched_eval_device_pitched", (H, 2, *ptrs(a, "cpu", "mem"), None, None, None, 0, L.FIT | L.PICK_BESTFIT,
                                                            None, None, *ptrs(a, "bind"), W, STREAM.cuda_stream))]
    with pytest.raises(ValueError, match="sel_val_ids"):
        ev.eval_device(a["cpu"], a["mem"], a["sel"], None, None, L.FIT, out_binding=a["bind"], stream=STREAM)


def bad_device_arguments(p):
    """argument name -> a tensor of that role that breaks one rule"""
    return {"cpu": dev((p,), torch.int32), "mem": dev((p,), torch.int64, is_cuda=False), "sel": dev((N_KEYS, p), torch.int64),
            "tol": dev((p,), torch.int64, index=1), "smp": dev((p - 1, A), torch.int32), "mask": pitched(p, W - 1, 16), "bind": dev((p - 1,), torch.int32)}


NAMES = {"cpu": "req_cpu_milli", "mem": "req_mem_bytes", "sel": "sel_val_ids", "tol": "tolerations", "smp": "samples", "mask": "mask|feasible", "bind": "binding"}


@pytest.mark.parametrize("which", ["cpu", "mem", "sel", "tol", "smp", "mask", "bind"])
def test_device_entry_points_refuse_one_bad_argument_before_any_call(which):
    p = 9
    ev = make_evaluator()
    pipe = make_pipe(ev)
    good = device_args(p)
    a = dict(good, **{which: bad_device_arguments(p)[which]})
    batch = (a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"])
    name = NAMES[which]
    entry_points = [
        lambda: ev.eval_device(*batch, a["flags"], out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
        lambda: ev.bind_eval_device(*batch, a["flags"], out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM),
        lambda: pipe.submit(0, *batch, a["flags"], a["mask"], a["bind"]),
        lambda: pipe.bind(*batch, a["flags"], [a["mask"]], [a["bind"]]),
    ]
    if which in ("cpu", "mem", "sel", "tol"):
        entry_points.append(lambda: ev.summarize_device(a["cpu"], a["mem"], a["sel"], a["tol"], PREDS, out=a["table"], stream=STREAM))
    if which in ("mem", "smp", "mask", "bind"):
        entry_points.append(lambda: ev.pick_device(a["mask"], a["flags"], a["bind"], req_mem_bytes=a["mem"], samples=a["smp"], stream=STREAM))
    for call in entry_points:
        with pytest.raises(ValueError, match=name):
            call()
    with pytest.raises(ValueError, match="out_fit"):  # the second mask at another pitch
        ev.eval_device(*[good[k] for k in ("cpu", "mem", "sel", "tol", "smp")], a["flags"], out_feasible=pitched(p, W, 16), out_fit=pitched(p, W, 3), stream=STREAM)
    with pytest.raises(ValueError, match="out"):
        ev.summarize_device(*[good[k] for k in ("cpu", "mem", "sel", "tol")], PREDS, out=dev((p, L.SUMMARY_WORDS - 1), torch.int32), stream=STREAM)
    assert calls_of(ev) == [], "a refused call reaches no library function"


def test_all_gather_forms():
    ev = make_evaluator()
    comm = make_comm(ev, world=2)
    local, gathered = dev((4,), torch.int32), dev((8,), torch.int32)
    want = ("ksched_allgather_bindings", (HC, local.data_ptr(), gathered.data_ptr(), 4, STREAM.cuda_stream))
    comm.all_gather(gathered, local, stream=STREAM)
    comm.bind_all_gather(gathered, local, STREAM)()
    assert calls_of(ev) == [want, want]
    clique = LocalClique.__new__(LocalClique)
    clique._evs, clique._lib, clique.n = [ev, SimpleNamespace(device=1)], ev._lib, 2
    clique._comms, clique._ctxs = (C.c_void_p * 2)(), (C.c_void_p * 2)()
    l2, g2 = [local, dev((4,), torch.int32, index=1)], [gathered, dev((8,), torch.int32, index=1)]
    clique.allgather_bindings(g2, l2, streams=[STREAM, STREAM])
    name, args = calls_of(ev)[2]
    assert name == "ksched_allgather_bindings_local" and args[1] == 2 and args[4] == 4
    assert ev._lib.arrays == [[t.data_ptr() for t in l2], [t.data_ptr() for t in g2]]
    del ev._lib.calls[:]
    bad = {"local": [(gathered, dev((4,), torch.int64)), (gathered, dev((4,), torch.int32, is_cuda=False)), (gathered, dev((4,), torch.int32, index=1)),
                     (gathered, strided((4,), torch.int32)), (gathered, dev((4, 1), torch.int32))],
           "gathered": [(dev((7,), torch.int32), local), (dev((9,), torch.int32), local), (dev((8,), torch.int32, is_cuda=False), local),
                        (dev((8,), torch.int32, index=1), local), (dev((8,), torch.int64), local)]}
    for name, cases in bad.items():
        for g, l in cases:
            for call in (lambda: comm.all_gather(g, l, stream=STREAM), lambda: comm.bind_all_gather(g, l, STREAM),
                         lambda: clique.allgather_bindings([g, g2[1]], [l, l2[1]], streams=[STREAM, STREAM])):
                with pytest.raises(ValueError, match=name):
                    call()
    with pytest.raises(ValueError, match=r"gathered\[1\]"):  # rank 1's buffer on rank 0's device
        clique.allgather_bindings([gathered, gathered], l2, streams=[STREAM, STREAM])
    assert calls_of(ev) == []


# ---- 3. the host (numpy) form --------------------------------------------------------------------------------------------------------
def host_args(p):
    rng = np.random.default_rng(p)
    return dict(cpu=rng.integers(0, 9, p).astype(np.int64), mem=rng.integers(0, 9, p).astype(np.int64), sel=rng.integers(0, 3, (N_KEYS, p)).astype(np.uint32),
                tol=rng.integers(0, 9, p).astype(np.uint64), smp=rng.integers(0, N_NODES, (p, A)).astype(np.uint32), feas=np.zeros((p, W), np.uint64))


def host_entry_points(ev, a, flags=PREDS | L.PICK_SAMPLED):
    return {"eval": lambda: ev.eval(a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"], flags),
            "explain": lambda: ev.explain(a["cpu"], a["mem"], a["sel"], a["tol"], [0], [1], PREDS),
            "summarize": lambda: ev.summarize(a["cpu"], a["mem"], a["sel"], a["tol"], PREDS),
            "pick": lambda: ev.pick(a["feas"], L.FIT | L.PICK_SAMPLED, req_mem_bytes=a["mem"], samples=a["smp"])}


@pytest.mark.parametrize("p", [0, 1, 9])
def test_host_entry_points_pass_the_callers_arrays(p):
    ev = make_evaluator()
    a = host_args(p)
    at = lambda *names: tuple(a[n].ctypes.data for n in names)  # noqa: E731
    flags = PREDS | L.PICK_SAMPLED
    calls = host_entry_points(ev, a)
    r = calls["eval"]()
    assert r.feasible.shape == (p, W) and r.binding.shape == (p,) and r.fit is None
    assert calls["explain"]().shape == (1,) and calls["summarize"]().shape == (p, L.SUMMARY_WORDS) and calls["pick"]().shape == (p,)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = calls_of(ev)
    assert (n0, a0[:9]) == ("ksched_eval", (H, p, *at("cpu", "mem", "sel", "tol", "smp"), A, flags)) and a0[9] == r.feasible.ctypes.data and a0[10] is None
    assert (n1, a1[:7], a1[9]) == ("ksched_explain", (H, p, *at("cpu", "mem", "sel", "tol"), 1), PREDS)
    assert (n2, a2[:7]) == ("ksched_summarize", (H, p, *at("cpu", "mem", "sel", "tol"), PREDS))
    assert (n3, a3[:7]) == ("ksched_pick", (H, p, *at("feas", "mem", "smp"), A, L.FIT | L.PICK_SAMPLED))


@pytest.mark.parametrize("entry", ["eval", "explain", "summarize", "pick"])
def test_host_entry_points_refuse_columns_of_the_wrong_length_or_rank(entry):
    p = 9
    ev = make_evaluator()
    good = host_args(p)
    bad = {"req_mem_bytes": dict(mem=good["mem"][:p - 1]), "req_cpu_milli": dict(cpu=np.zeros((p, 2), np.int64)),
           "tolerations": dict(tol=np.zeros(p + 1, np.uint64)), "sel_val_ids": dict(sel=good["sel"][:, :p - 1]), "samples": dict(smp=good["smp"][:p - 1])}
    reads = {"eval": bad.keys(), "explain": ("req_mem_bytes", "req_cpu_milli", "tolerations", "sel_val_ids"),
             "summarize": ("req_mem_bytes", "req_cpu_milli", "tolerations", "sel_val_ids"), "pick": ("req_mem_bytes", "samples")}[entry]
    for name in reads:
        with pytest.raises(ValueError, match=name):
            host_entry_points(ev, dict(good, **bad[name]))[entry]()
    assert calls_of(ev) == []


def test_host_form_still_converts_lists_and_strided_arrays():
    p = 4
    ev = make_evaluator()
    a = host_args(p)
    wide = np.zeros((p, 2 * A), np.uint32)
    converted = dict(cpu=a["cpu"].tolist(), mem=np.repeat(a["mem"], 2)[::2], sel=a["sel"].astype(np.int64), tol=a["tol"].tolist(), smp=wide[:, ::2],
                     feas=np.zeros((p, 2 * W), np.uint64)[:, ::2])
    for call in host_entry_points(ev, converted).values():
        call()
    assert [c[0] for c in calls_of(ev)] == ["ksched_eval", "ksched_explain", "ksched_summarize", "ksched_pick"]
    assert all(c[1][1] == p and c[1][2] not in (None, 0) for c in calls_of(ev))
    b = M.host_batch(N_KEYS, converted["cpu"], converted["mem"], converted["sel"], converted["tol"], converted["smp"], L.PICK_UNIFORM)
    assert b.attempts == A and [k.dtype for k in b.keep] == [np.int64, np.int64, np.uint32, np.uint64, np.uint32]
    assert all(k.flags.c_contiguous for k in b.keep) and np.array_equal(b.keep[0], a["cpu"]) and np.array_equal(b.keep[2], a["sel"])


def test_snapshot_columns_use_the_host_check():
    ev = make_evaluator()
    n = 5
    cpu, mem = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    ev.set_nodes(cpu.tolist(), mem, np.zeros((3, n), np.uint32), np.zeros(n, np.uint64))
    assert (ev.n, ev.n_keys) == (n, 3) and calls_of(ev)[0][1][1] == n and calls_of(ev)[0][1][5] == 3
    ev.update_nodes([1, 2], [5, 6], [7, 8])
    ev.update_node_labels([1], np.zeros((3, 1), np.uint32), [0])
    assert [c[0] for c in calls_of(ev)] == ["ksched_set_nodes", "ksched_update_nodes", "ksched_update_node_labels"]
    for name, call in (("avail_mem_bytes", lambda: ev.set_nodes(cpu, mem[:-1])), ("label_val_ids", lambda: ev.set_nodes(cpu, mem, np.zeros((3, n + 1), np.uint32))),
                       ("taints", lambda: ev.set_nodes(cpu, mem, None, np.zeros(n - 1, np.uint64))), ("avail_cpu_milli", lambda: ev.update_nodes([1, 2], [5], [7, 8])),
                       ("label_val_ids", lambda: ev.update_node_labels([1], np.zeros((2, 1), np.uint32))), ("node_index", lambda: ev.update_nodes([[1]], [[5]], [[7]]))):
        with pytest.raises(ValueError, match=name):
            call()
    assert len(calls_of(ev)) == 3
