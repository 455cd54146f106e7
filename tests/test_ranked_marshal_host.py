"""PICK_SPREAD and PICK_PACK through the binding's argument checks (kube_scheduler_rs_reference_amd/_marshal.py), without a GPU: over the
stand-in tensors and the recording stub of tests/test_marshal_host.py.  `samples` is required and its shape is checked with the flag, a
valid call passes all d columns as `attempts`, and a refused call -- a wrong shape is a ValueError -- reaches no library function."""
import numpy as np
import pytest
import torch

from kube_scheduler_rs_reference_amd import _lib as L
from kube_scheduler_rs_reference_amd import _marshal as M
from tests.test_marshal_host import (A, H, HP, PREDS, STREAM, W, calls_of, dev, device_args, make_evaluator, make_pipe, ptrs)

# the members that read every column of the table (neither reads a request column: ksched_pick_device gets no req_mem_bytes)
PICKS = pytest.mark.parametrize("PICK", [L.PICK_SPREAD, L.PICK_PACK], ids=["spread", "pack"])


@PICKS
def test_draws_are_required_and_their_shape_checked(PICK):
    p = 2
    assert M.DRAWS & PICK and M.DRAWS == L.PICK_DRAWS and L.PICK_RANKED & PICK and L.PICK_ANY & PICK
    good = dev((p, A), torch.int32)
    for device, smp in ((0, good), (None, np.zeros((p, A), np.uint32))):
        ptr, attempts, _ = M.draws(smp, "samples", PREDS | PICK, p, device)
        assert attempts == A and ptr.value == (smp.data_ptr() if device == 0 else smp.ctypes.data)
        with pytest.raises(ValueError, match="samples"):
            M.draws(None, "samples", PREDS | PICK, p, device)
    for d in (1, 2, 64):  # every column counts: d is the table's width
        assert M.draws(np.zeros((p, d), np.uint32), "samples", PICK, p)[1] == d
        assert M.draws(dev((p, d), torch.uint32), "samples", PICK, p, 0)[1] == d
    for bad in (np.zeros((p, 0), np.uint32), np.zeros((p - 1, A), np.uint32), np.zeros((p + 1, A), np.uint32), np.zeros((p * A,), np.uint32)):
        with pytest.raises(ValueError, match="samples"):
            M.draws(bad, "samples", PICK, p)
    with pytest.raises(ValueError, match="samples"):
        M.draws(dev((p, A), torch.int64), "samples", PICK, p, 0)  # not 32-bit


@PICKS
@pytest.mark.parametrize("p", [0, 1, 9])
def test_device_entry_points_pass_exactly_the_checked_arguments(p, PICK):
    ev = make_evaluator()
    a = device_args(p, PICK)
    assert a["attempts"] == A
    batch = (a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"])
    head = (p, *ptrs(a, "cpu", "mem", "sel", "tol", "smp"), A, a["flags"])
    ev.eval_device(*batch, a["flags"], out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM)
    assert calls_of(ev) == [("ksched_eval_device_pitched", (H, *head, *ptrs(a, "mask"), None, *ptrs(a, "bind"), a["pitch"], STREAM.cuda_stream))]
    pipe = make_pipe(ev)
    pipe.submit(1, *batch, a["flags"], a["mask"], a["bind"])
    assert calls_of(ev)[1:] == [("ksched_pipe_submit", (HP, 1, *head, *ptrs(a, "mask"), a["pitch"], *ptrs(a, "bind")))]
    ev.pick_device(a["mask"], PICK, a["bind"], samples=a["smp"], stream=STREAM)
    assert calls_of(ev)[2:] == [("ksched_pick_device", (H, p, *ptrs(a, "mask"), a["pitch"], None, *ptrs(a, "smp"), A, PICK, *ptrs(a, "bind"),
                                                        STREAM.cuda_stream))]


@PICKS
def test_host_entry_points_pass_the_table_and_its_width(PICK):
    p = 4
    ev = make_evaluator()
    z = np.zeros(p, np.int64)
    smp = np.zeros((p, 3), np.uint32)
    r = ev.eval(z, z, samples=smp, flags=L.FIT | PICK)
    (name, args), = calls_of(ev)
    assert name == "ksched_eval" and args[1] == p and args[6] == smp.ctypes.data and args[7] == 3 and args[8] == L.FIT | PICK
    assert r.binding is not None and r.binding.shape == (p,) and args[11] == r.binding.ctypes.data
    mask = np.zeros((p, W), np.uint64)
    ev.pick(mask, PICK, samples=smp)
    name, args = calls_of(ev)[1]
    assert name == "ksched_pick" and args[1] == p and args[4] == smp.ctypes.data and args[5] == 3 and args[6] == PICK


@PICKS
@pytest.mark.parametrize("smp", [None, (8, A), (9, 0), (9 * A,)], ids=["none", "a row short", "no column", "flat"])
def test_a_refusal_reaches_no_library_function(smp, PICK):
    p = 9
    ev = make_evaluator()
    pipe = make_pipe(ev)
    a = device_args(p, PICK)
    bad = None if smp is None else dev(smp, torch.int32)
    batch = (a["cpu"], a["mem"], a["sel"], a["tol"], bad)
    for call in (lambda: ev.eval_device(*batch, a["flags"], out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
                 lambda: ev.bind_eval_device(*batch, a["flags"], out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM),
                 lambda: pipe.submit(0, *batch, a["flags"], a["mask"], a["bind"]),
                 lambda: ev.pick_device(a["mask"], PICK, a["bind"], samples=bad, stream=STREAM)):
        with pytest.raises(ValueError, match="samples"):
            call()
    host_bad = None if smp is None else np.zeros(smp, np.uint32)
    z = np.zeros(p, np.int64)
    with pytest.raises(ValueError, match="samples"):
        ev.eval(z, z, samples=host_bad, flags=L.FIT | PICK)
    with pytest.raises(ValueError, match="samples"):
        ev.pick(np.zeros((p, W), np.uint64), PICK, samples=host_bad)
    assert calls_of(ev) == [], "a refused call reaches no library function"
