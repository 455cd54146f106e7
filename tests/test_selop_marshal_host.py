"""SELOP_EXISTS / SELOP_GT / SELOP_LT through the binding's argument checks (kube_scheduler_rs_reference_amd/_marshal.py), without a GPU: over
the stand-in tensors and the recording stub of tests/test_marshal_host.py.  The rule (_marshal.selop, beside _marshal.combine and
_marshal.soft): the evaluations -- Evaluator.eval, eval_device, bind_eval_device -- accept one operator flag beside SEL, with a combine op,
the modifier and a pick under their own rules, and without FIT, TAINT, WANT_FIT_MASK / `out_fit`; Pipe.submit / bind, the picks, the
summaries and explain refuse the flags.  Every refusal is a ValueError naming the argument and reaches no library function; an accepted
call passes the flag word through unchanged."""
import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import _lib as L
from kube_scheduler_rs_reference_amd import _marshal as M
from tests.test_marshal_host import (A, H, STREAM, calls_of, device_args, host_args, make_evaluator, make_pipe, ptrs)

OPS = pytest.mark.parametrize("OP", [L.SELOP_EXISTS, L.SELOP_GT, L.SELOP_LT], ids=["exists", "gt", "lt"])
COMBINES = [0, L.COMBINE_AND, L.COMBINE_OR, L.COMBINE_ANDNOT, L.COMBINE_AND | L.COMBINE_SOFT, L.COMBINE_ANDNOT | L.COMBINE_SOFT]


def others(OP):
    return [o for o in (L.SELOP_EXISTS, L.SELOP_GT, L.SELOP_LT) if o != OP]


@OPS
def test_the_rule_itself(OP):
    assert (L.SELOP_EXISTS, L.SELOP_GT, L.SELOP_LT, L.SELOP_ANY) == (0x4000, 0x8000, 0x10000, 0x1C000)
    assert not (M.COMBINE & L.SELOP_ANY) and not (L.COMBINE_SOFT & L.SELOP_ANY) and not (L.PICK_ANY & L.SELOP_ANY)
    for comb in COMBINES:
        for pick in (0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_SPREAD):
            assert M.selop(L.SEL | OP | comb | pick, "here", accepted=True) is None
    # without an operator flag the rule says nothing, whatever the rest is
    fit = object()
    for flags in (0, L.SEL, L.FIT | L.SEL | L.TAINT, L.FIT | L.WANT_FIT_MASK, 0x1000, 0xE00, L.COMBINE_SOFT):
        assert M.selop(flags, "here", accepted=False) is None and M.selop(flags, "here", accepted=True, out_fit=fit) is None
    with pytest.raises(ValueError, match="flags.*here"):
        M.selop(L.SEL | OP, "here", accepted=False)
    with pytest.raises(ValueError, match="flags.*here"):
        M.selop(OP, "here", accepted=False)
    for other in others(OP):
        with pytest.raises(ValueError, match="flags.*at most one"):
            M.selop(L.SEL | OP | other, "here", accepted=True)
    with pytest.raises(ValueError, match="flags.*at most one"):
        M.selop(L.SEL | L.SELOP_ANY, "here", accepted=True)
    with pytest.raises(ValueError, match="flags.*SEL"):
        M.selop(OP, "here", accepted=True)
    with pytest.raises(ValueError, match="flags.*SEL"):
        M.selop(OP | L.PICK_UNIFORM, "here", accepted=True)
    for pred in (L.FIT, L.TAINT, L.FIT | L.TAINT):
        with pytest.raises(ValueError, match="flags.*FIT"):
            M.selop(L.SEL | OP | pred, "here", accepted=True)
    with pytest.raises(ValueError, match="out_fit"):
        M.selop(L.SEL | OP | L.WANT_FIT_MASK, "here", accepted=True)
    with pytest.raises(ValueError, match="out_fit"):
        M.selop(L.SEL | OP, "here", accepted=True, out_fit=fit)
    # the combining call's own rules are unchanged by the flag
    mask = object()
    assert M.combine(L.SEL | OP | L.COMBINE_AND, "here", accepted=True, out_feasible=mask) is None
    assert M.soft(L.SEL | OP | L.COMBINE_ANDNOT | L.COMBINE_SOFT, "here", accepted=True) is None
    with pytest.raises(ValueError, match="out_feasible"):
        M.combine(L.SEL | OP | L.COMBINE_AND, "here", accepted=True, out_feasible=None)
    with pytest.raises(ValueError, match="flags.*COMBINE_SOFT"):
        M.soft(L.SEL | OP | L.COMBINE_OR | L.COMBINE_SOFT, "here", accepted=True)


@OPS
@pytest.mark.parametrize("comb", COMBINES, ids=["plain", "and", "or", "andnot", "soft-and", "soft-andnot"])
@pytest.mark.parametrize("pick", [0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_SPREAD], ids=["none", "sampled", "bestfit", "spread"])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_eval_device_passes_the_flags_through(p, pick, comb, OP):
    ev = make_evaluator()
    a = device_args(p, pick)
    flags = L.SEL | OP | comb | pick
    batch = (a["cpu"], a["mem"], a["sel"], None, a["smp"])
    bind = a["bind"] if pick else None
    want = ("ksched_eval_device_pitched", (H, p, *ptrs(a, "cpu", "mem", "sel"), None, *ptrs(a, "smp"), a["attempts"], flags, *ptrs(a, "mask"), None,
                                           bind.data_ptr() or None if pick else None, a["pitch"], STREAM.cuda_stream))
    ev.eval_device(*batch, flags, out_feasible=a["mask"], out_binding=bind, stream=STREAM)
    assert calls_of(ev) == [want]
    ev.bind_eval_device(*batch, flags, out_feasible=[a["mask"]], out_bindings=[bind] if pick else (), stream=STREAM)(0, 0)
    assert calls_of(ev) == [want, want], "the bound and the unbound form pass the same argument tuple"


@OPS
@pytest.mark.parametrize("pick", [0, L.PICK_UNIFORM], ids=["none", "uniform"])
def test_the_host_form_passes_the_flags_through(pick, OP):
    p = 9
    ev = make_evaluator()
    a = host_args(p)
    flags = L.SEL | OP | pick
    r = ev.eval(a["cpu"], a["mem"], a["sel"], None, a["smp"] if pick else None, flags)
    (name, args), = calls_of(ev)
    assert name == "ksched_eval" and args[:2] == (H, p) and args[8] == flags and args[7] == (A if pick else 0)
    assert args[2:5] == (a["cpu"].ctypes.data, a["mem"].ctypes.data, a["sel"].ctypes.data) and args[5] is None
    assert args[9] == r.feasible.ctypes.data and args[10] is None and (args[11] == r.binding.ctypes.data if pick else args[11] is None)


@OPS
def test_every_refusal_is_a_value_error_naming_the_argument_before_any_library_call(OP):
    p = 9
    ev = make_evaluator()
    pipe = make_pipe(ev)
    a = device_args(p, L.PICK_UNIFORM)
    h = host_args(p)
    batch = (a["cpu"], a["mem"], a["sel"], None, a["smp"])
    flags = L.SEL | OP | L.PICK_UNIFORM
    two = flags | others(OP)[0]
    no_sel = OP | L.PICK_UNIFORM
    dev_kw = dict(out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM)
    bound_kw = dict(out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM)
    refused = {
        "flags": [lambda: ev.eval_device(*batch, two, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.SELOP_ANY, **dev_kw),
                  lambda: ev.eval_device(*batch, no_sel, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.FIT, **dev_kw),
                  lambda: ev.eval_device(a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"], flags | L.TAINT, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.COMBINE_AND | L.FIT, **dev_kw),
                  lambda: ev.bind_eval_device(*batch, two, **bound_kw),
                  lambda: ev.bind_eval_device(*batch, no_sel, **bound_kw),
                  lambda: ev.bind_eval_device(*batch, flags | L.FIT, **bound_kw),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], two),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], no_sel),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], flags | L.FIT),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], h["tol"], h["smp"], flags | L.TAINT),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], flags | L.COMBINE_AND),  # (the host form combines nothing)
                  lambda: pipe.submit(0, *batch, flags, a["mask"], a["bind"]),
                  lambda: pipe.submit(0, *batch, L.FIT | flags, a["mask"], a["bind"]),
                  lambda: pipe.bind(*batch, flags, [a["mask"], a["mask"]], [a["bind"], a["bind"]]),
                  lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | OP, a["bind"], samples=a["smp"], stream=STREAM),
                  lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | L.SEL | OP, a["bind"], samples=a["smp"], stream=STREAM),
                  lambda: ev.pick(h["feas"], L.PICK_UNIFORM | L.SEL | OP, samples=h["smp"]),
                  lambda: ev.summarize(h["cpu"], h["mem"], h["sel"], None, L.SEL | OP),
                  lambda: ev.summarize_device(a["cpu"], a["mem"], a["sel"], None, L.SEL | OP, out=a["table"], stream=STREAM),
                  lambda: ev.explain(h["cpu"], h["mem"], h["sel"], None, [0], [1], L.SEL | OP)],
        "out_fit": [lambda: ev.eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.eval_device(*batch, flags | L.WANT_FIT_MASK, **dev_kw),
                    lambda: ev.bind_eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_bindings=[a["bind"]], stream=STREAM),
                    lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], flags | L.WANT_FIT_MASK)],
        # the combining call's own refusals, with an operator flag beside the op
        "out_feasible": [lambda: ev.eval_device(*batch, flags | L.COMBINE_AND, out_binding=a["bind"], stream=STREAM),
                         lambda: ev.bind_eval_device(*batch, flags | L.COMBINE_ANDNOT | L.COMBINE_SOFT, out_bindings=[a["bind"]], stream=STREAM)],
    }
    for name, calls in refused.items():
        for i, call in enumerate(calls):
            with pytest.raises(ValueError, match=name):
                call()
                pytest.fail(f"{name}: refusal {i} was accepted")
    for where, call in (("Pipe.submit", lambda: pipe.submit(0, *batch, flags, a["mask"], a["bind"])),
                        ("Evaluator.pick_device", lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | OP, a["bind"], samples=a["smp"], stream=STREAM)),
                        ("Evaluator.pick", lambda: ev.pick(h["feas"], L.PICK_UNIFORM | OP, samples=h["smp"])),
                        ("Evaluator.summarize", lambda: ev.summarize(h["cpu"], h["mem"], h["sel"], None, L.SEL | OP)),
                        ("Evaluator.summarize_device", lambda: ev.summarize_device(a["cpu"], a["mem"], a["sel"], None, L.SEL | OP, out=a["table"], stream=STREAM)),
                        ("Evaluator.explain", lambda: ev.explain(h["cpu"], h["mem"], h["sel"], None, [0], [1], L.SEL | OP))):
        with pytest.raises(ValueError, match="flags: " + where.replace(".", r"\.") + " takes no SELOP"):
            call()
    assert calls_of(ev) == [], "a refused call reaches no library function"
    assert np.array_equal(h["feas"], np.zeros_like(h["feas"]))
