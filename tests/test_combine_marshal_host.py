"""COMBINE_AND / COMBINE_OR / COMBINE_ANDNOT through the binding's argument checks (kube_scheduler_rs_reference_amd/_marshal.py), without a
GPU: over the stand-in tensors and the recording stub of tests/test_marshal_host.py.  The one rule (_marshal.combine): only eval_device /
bind_eval_device accept the flags, at most one per call, `out_feasible` is required, WANT_FIT_MASK / `out_fit` are excluded; the host form
Evaluator.eval and Pipe.submit / bind refuse them.  Every refusal is a ValueError naming the argument and reaches no library function; an
accepted call passes the flags through unchanged."""
import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import _lib as L
from kube_scheduler_rs_reference_amd import _marshal as M
from tests.test_marshal_host import (A, H, PREDS, STREAM, calls_of, device_args, make_evaluator, make_pipe, ptrs)

OPS = pytest.mark.parametrize("OP", [L.COMBINE_AND, L.COMBINE_OR, L.COMBINE_ANDNOT], ids=["and", "or", "andnot"])


@OPS
def test_the_rule_itself(OP):
    mask, fit = object(), object()
    assert M.COMBINE == L.COMBINE_ANY and M.COMBINE & OP
    assert M.combine(PREDS | OP, "here", accepted=True, out_feasible=mask) is None
    assert M.combine(PREDS | OP | L.PICK_BESTFIT, "here", accepted=True, out_feasible=mask) is None
    # without a combine flag the rule says nothing, whatever the rest is
    assert M.combine(PREDS | L.WANT_FIT_MASK, "here", accepted=False, out_feasible=None, out_fit=fit) is None
    assert M.combine(0x1000, "here", accepted=False) is None  # (not a combine flag: the library's own KSCHED_E_INVAL)
    with pytest.raises(ValueError, match="flags.*here"):
        M.combine(PREDS | OP, "here", accepted=False, out_feasible=mask)
    with pytest.raises(ValueError, match="out_feasible"):
        M.combine(PREDS | OP, "here", accepted=True, out_feasible=None)
    with pytest.raises(ValueError, match="out_fit"):
        M.combine(PREDS | OP, "here", accepted=True, out_feasible=mask, out_fit=fit)
    with pytest.raises(ValueError, match="out_fit"):
        M.combine(PREDS | OP | L.WANT_FIT_MASK, "here", accepted=True, out_feasible=mask)
    for other in (L.COMBINE_AND, L.COMBINE_OR, L.COMBINE_ANDNOT):
        if other != OP:
            with pytest.raises(ValueError, match="flags"):
                M.combine(PREDS | OP | other, "here", accepted=True, out_feasible=mask)


@OPS
@pytest.mark.parametrize("pick", [0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_SPREAD], ids=["none", "sampled", "bestfit", "spread"])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_eval_device_passes_the_flags_through(p, pick, OP):
    ev = make_evaluator()
    a = device_args(p, pick)
    flags = a["flags"] | OP
    batch = (a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"])
    bind = a["bind"] if pick else None
    want = ("ksched_eval_device_pitched", (H, p, *ptrs(a, "cpu", "mem", "sel", "tol", "smp"), a["attempts"], flags, *ptrs(a, "mask"), None,
                                           bind.data_ptr() or None if pick else None, a["pitch"], STREAM.cuda_stream))
    ev.eval_device(*batch, flags, out_feasible=a["mask"], out_binding=bind, stream=STREAM)
    assert calls_of(ev) == [want]
    ev.bind_eval_device(*batch, flags, out_feasible=[a["mask"]], out_bindings=[bind] if pick else (), stream=STREAM)(0, 0)
    assert calls_of(ev) == [want, want], "the bound and the unbound form pass the same argument tuple"


@OPS
def test_every_refusal_is_a_value_error_naming_the_argument_before_any_library_call(OP):
    p = 9
    ev = make_evaluator()
    pipe = make_pipe(ev)
    a = device_args(p, L.PICK_UNIFORM)
    batch = (a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"])
    flags = a["flags"] | OP
    two = flags | (L.COMBINE_OR if OP != L.COMBINE_OR else L.COMBINE_AND)
    refused = {
        "out_feasible": [lambda: ev.eval_device(*batch, flags, out_binding=a["bind"], stream=STREAM),
                         lambda: ev.bind_eval_device(*batch, flags, out_bindings=[a["bind"]], stream=STREAM),
                         lambda: ev.bind_eval_device(*batch, flags, out_feasible=[a["mask"], None], out_bindings=[a["bind"]], stream=STREAM)],
        "out_fit": [lambda: ev.eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.eval_device(*batch, flags | L.WANT_FIT_MASK, out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.eval_device(*batch, flags | L.WANT_FIT_MASK, out_feasible=a["mask"], out_fit=a["fit"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.bind_eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_bindings=[a["bind"]], stream=STREAM)],
        "flags": [lambda: ev.eval_device(*batch, two, out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
                  lambda: ev.bind_eval_device(*batch, two, out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM),
                  lambda: pipe.submit(0, *batch, flags, a["mask"], a["bind"]),
                  lambda: pipe.bind(*batch, flags, [a["mask"], a["mask"]], [a["bind"], a["bind"]])],
    }
    for name, calls in refused.items():
        for i, call in enumerate(calls):
            with pytest.raises(ValueError, match=name):
                call()
                pytest.fail(f"{name}: refusal {i} was accepted")
    # the host form: masks are combined on the device
    z = np.zeros(p, np.int64)
    for host_flags in (L.FIT | OP, L.FIT | OP | L.PICK_BESTFIT):
        with pytest.raises(ValueError, match="flags.*Evaluator.eval"):
            ev.eval(z, z, flags=host_flags)
    with pytest.raises(ValueError, match="flags"):
        ev.eval(z, z, samples=np.zeros((p, A), np.uint32), flags=L.FIT | OP | L.PICK_UNIFORM, want_mask=False)
    assert calls_of(ev) == [], "a refused call reaches no library function"
