"""COMBINE_SOFT through the binding's argument checks (kube_scheduler_rs_reference_amd/_marshal.py), without a GPU: over the stand-in tensors
and the recording stub of tests/test_marshal_host.py.  The rules (_marshal.soft, beside _marshal.combine): only eval_device /
bind_eval_device accept the modifier, and only with COMBINE_AND or COMBINE_ANDNOT; everything a combining call needs it needs too
(`out_feasible`, no WANT_FIT_MASK / `out_fit`, one op); the host form Evaluator.eval and Pipe.submit / bind refuse it.  Every refusal is a
ValueError naming the argument and reaches no library function; an accepted call passes the flags through unchanged."""
import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import _lib as L
from kube_scheduler_rs_reference_amd import _marshal as M
from tests.test_marshal_host import (A, H, PREDS, STREAM, calls_of, device_args, make_evaluator, make_pipe, ptrs)

SOFT = L.COMBINE_SOFT
OPS = pytest.mark.parametrize("OP", [L.COMBINE_AND, L.COMBINE_ANDNOT], ids=["and", "andnot"])


@OPS
def test_the_rule_itself(OP):
    assert SOFT == 0x2000 and not (M.COMBINE & SOFT)
    assert M.soft(PREDS | OP | SOFT, "here", accepted=True) is None
    assert M.soft(PREDS | OP | SOFT | L.PICK_BESTFIT, "here", accepted=True) is None
    # without the modifier the rule says nothing, whatever the rest is
    for flags in (PREDS, PREDS | OP, PREDS | L.COMBINE_OR, PREDS | 0xE00, 0x1000, PREDS | L.WANT_FIT_MASK):
        assert M.soft(flags, "here", accepted=False) is None and M.soft(flags, "here", accepted=True) is None
    with pytest.raises(ValueError, match="flags.*here"):
        M.soft(PREDS | OP | SOFT, "here", accepted=False)
    with pytest.raises(ValueError, match="flags.*here"):
        M.soft(PREDS | SOFT, "here", accepted=False)
    with pytest.raises(ValueError, match="flags.*COMBINE_SOFT"):
        M.soft(PREDS | SOFT, "here", accepted=True)  # no op
    with pytest.raises(ValueError, match="flags.*COMBINE_SOFT"):
        M.soft(PREDS | L.COMBINE_OR | SOFT, "here", accepted=True)  # OR cannot empty a row
    for other in (L.COMBINE_AND, L.COMBINE_OR, L.COMBINE_ANDNOT):
        if other != OP:
            with pytest.raises(ValueError, match="flags"):
                M.soft(PREDS | OP | other | SOFT, "here", accepted=True)
    # the combining call's own rule is unchanged by the bit
    mask, fit = object(), object()
    assert M.combine(PREDS | OP | SOFT, "here", accepted=True, out_feasible=mask) is None
    assert M.combine(PREDS | SOFT, "here", accepted=False) is None
    with pytest.raises(ValueError, match="out_feasible"):
        M.combine(PREDS | OP | SOFT, "here", accepted=True, out_feasible=None)
    with pytest.raises(ValueError, match="out_fit"):
        M.combine(PREDS | OP | SOFT, "here", accepted=True, out_feasible=mask, out_fit=fit)


@OPS
@pytest.mark.parametrize("pick", [0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_SPREAD], ids=["none", "sampled", "bestfit", "spread"])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_eval_device_passes_the_flags_through(p, pick, OP):
    ev = make_evaluator()
    a = device_args(p, pick)
    flags = a["flags"] | OP | SOFT
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
    flags = a["flags"] | OP | SOFT
    no_op, with_or = a["flags"] | SOFT, a["flags"] | L.COMBINE_OR | SOFT
    two = flags | (L.COMBINE_OR if OP != L.COMBINE_AND else L.COMBINE_ANDNOT)
    refused = {
        "out_feasible": [lambda: ev.eval_device(*batch, flags, out_binding=a["bind"], stream=STREAM),
                         lambda: ev.bind_eval_device(*batch, flags, out_bindings=[a["bind"]], stream=STREAM),
                         lambda: ev.bind_eval_device(*batch, flags, out_feasible=[a["mask"], None], out_bindings=[a["bind"]], stream=STREAM)],
        "out_fit": [lambda: ev.eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.eval_device(*batch, flags | L.WANT_FIT_MASK, out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.bind_eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_bindings=[a["bind"]], stream=STREAM)],
        "flags": [lambda: ev.eval_device(*batch, no_op, out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
                  lambda: ev.eval_device(*batch, with_or, out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
                  lambda: ev.eval_device(*batch, two, out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM),
                  lambda: ev.bind_eval_device(*batch, no_op, out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM),
                  lambda: ev.bind_eval_device(*batch, with_or, out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM),
                  lambda: pipe.submit(0, *batch, flags, a["mask"], a["bind"]),
                  lambda: pipe.submit(0, *batch, no_op, a["mask"], a["bind"]),
                  lambda: pipe.bind(*batch, flags, [a["mask"], a["mask"]], [a["bind"], a["bind"]]),
                  lambda: pipe.bind(*batch, no_op, [a["mask"], a["mask"]], [a["bind"], a["bind"]])],
    }
    for name, calls in refused.items():
        for i, call in enumerate(calls):
            with pytest.raises(ValueError, match=name):
                call()
                pytest.fail(f"{name}: refusal {i} was accepted")
    # the host form: masks are combined on the device
    z = np.zeros(p, np.int64)
    for host_flags in (L.FIT | OP | SOFT, L.FIT | SOFT, L.FIT | OP | SOFT | L.PICK_BESTFIT):
        with pytest.raises(ValueError, match="flags.*Evaluator.eval"):
            ev.eval(z, z, flags=host_flags)
    with pytest.raises(ValueError, match="flags"):
        ev.eval(z, z, samples=np.zeros((p, A), np.uint32), flags=L.FIT | SOFT | L.PICK_UNIFORM, want_mask=False)
    assert calls_of(ev) == [], "a refused call reaches no library function"
