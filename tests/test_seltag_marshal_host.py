"""SELOP_TAGGED through the binding's argument checks (kube_scheduler_rs_reference_amd/_marshal.py), without a GPU: over the stand-in tensors
and the recording stub of tests/test_marshal_host.py.  The rule (_marshal.seltag, beside _marshal.selop): the evaluations -- Evaluator.eval,
eval_device, bind_eval_device -- accept the flag beside SEL, with a combine op, the modifier and a pick under their own rules, and without
a SELOP_EXISTS / _GT / _LT flag, FIT, TAINT, WANT_FIT_MASK / `out_fit`; Pipe.submit / bind, the picks, the summaries and explain refuse it.
Every refusal is a ValueError naming the argument and reaches no library function; an accepted call passes the flag word through
unchanged.  And the entry helper `seltag(tag, ids)`: what it builds, and what it refuses."""
import numpy as np
import pytest

import kube_scheduler_rs_reference_amd as pkg
from kube_scheduler_rs_reference_amd import _lib as L
from kube_scheduler_rs_reference_amd import _marshal as M
from tests.test_marshal_host import (A, H, STREAM, calls_of, device_args, host_args, make_evaluator, make_pipe, ptrs)

T = L.SELOP_TAGGED
OPS = [L.SELOP_EXISTS, L.SELOP_GT, L.SELOP_LT]
COMBINES = [0, L.COMBINE_AND, L.COMBINE_OR, L.COMBINE_ANDNOT, L.COMBINE_AND | L.COMBINE_SOFT, L.COMBINE_ANDNOT | L.COMBINE_SOFT]


def test_the_rule_itself():
    assert T == 0x40000 and not T & (L.SELOP_ANY | M.COMBINE | L.COMBINE_SOFT | L.PICK_ANY | 0x1FF)
    for comb in COMBINES:
        for pick in (0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_UNIFORM, L.PICK_SPREAD, L.PICK_PACK):
            assert M.seltag(L.SEL | T | comb | pick, "here", accepted=True) is None
    # without the flag the rule says nothing, whatever the rest is
    fit = object()
    for flags in (0, L.SEL, L.FIT | L.SEL | L.TAINT, L.FIT | L.WANT_FIT_MASK, 0x1000, 0x20000, 0xE00, L.COMBINE_SOFT, L.SEL | L.SELOP_GT, L.SELOP_ANY):
        assert M.seltag(flags, "here", accepted=False) is None and M.seltag(flags, "here", accepted=True, out_fit=fit) is None
    with pytest.raises(ValueError, match="flags.*here"):
        M.seltag(L.SEL | T, "here", accepted=False)
    with pytest.raises(ValueError, match="flags.*here"):
        M.seltag(T, "here", accepted=False)
    for op in OPS + [L.SELOP_ANY, L.SELOP_GT | L.SELOP_LT]:
        with pytest.raises(ValueError, match="flags.*SELOP_TAGGED excludes SELOP_EXISTS"):
            M.seltag(L.SEL | T | op, "here", accepted=True)
    with pytest.raises(ValueError, match="flags.*needs SEL"):
        M.seltag(T, "here", accepted=True)
    with pytest.raises(ValueError, match="flags.*needs SEL"):
        M.seltag(T | L.PICK_UNIFORM, "here", accepted=True)
    for pred in (L.FIT, L.TAINT, L.FIT | L.TAINT):
        with pytest.raises(ValueError, match="flags.*FIT"):
            M.seltag(L.SEL | T | pred, "here", accepted=True)
    with pytest.raises(ValueError, match="out_fit"):
        M.seltag(L.SEL | T | L.WANT_FIT_MASK, "here", accepted=True)
    with pytest.raises(ValueError, match="out_fit"):
        M.seltag(L.SEL | T, "here", accepted=True, out_fit=fit)
    # the operator rule says nothing about the flag, and the combining call's own rules are unchanged by it
    assert M.selop(L.SEL | T, "here", accepted=False) is None
    mask = object()
    assert M.combine(L.SEL | T | L.COMBINE_AND, "here", accepted=True, out_feasible=mask) is None
    assert M.soft(L.SEL | T | L.COMBINE_ANDNOT | L.COMBINE_SOFT, "here", accepted=True) is None
    with pytest.raises(ValueError, match="out_feasible"):
        M.combine(L.SEL | T | L.COMBINE_AND, "here", accepted=True, out_feasible=None)
    with pytest.raises(ValueError, match="flags.*COMBINE_SOFT"):
        M.soft(L.SEL | T | L.COMBINE_OR | L.COMBINE_SOFT, "here", accepted=True)


@pytest.mark.parametrize("comb", COMBINES, ids=["plain", "and", "or", "andnot", "soft-and", "soft-andnot"])
@pytest.mark.parametrize("pick", [0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_SPREAD], ids=["none", "sampled", "bestfit", "spread"])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_eval_device_passes_the_flag_through(p, pick, comb):
    ev = make_evaluator()
    a = device_args(p, pick)
    flags = L.SEL | T | comb | pick
    batch = (a["cpu"], a["mem"], a["sel"], None, a["smp"])
    bind = a["bind"] if pick else None
    want = ("ksched_eval_device_pitched", (H, p, *ptrs(a, "cpu", "mem", "sel"), None, *ptrs(a, "smp"), a["attempts"], flags, *ptrs(a, "mask"), None,
                                           bind.data_ptr() or None if pick else None, a["pitch"], STREAM.cuda_stream))
    ev.eval_device(*batch, flags, out_feasible=a["mask"], out_binding=bind, stream=STREAM)
    assert calls_of(ev) == [want]
    ev.bind_eval_device(*batch, flags, out_feasible=[a["mask"]], out_bindings=[bind] if pick else (), stream=STREAM)(0, 0)
    assert calls_of(ev) == [want, want], "the bound and the unbound form pass the same argument tuple"


@pytest.mark.parametrize("pick", [0, L.PICK_UNIFORM], ids=["none", "uniform"])
def test_the_host_form_passes_the_flag_through(pick):
    p = 9
    ev = make_evaluator()
    a = host_args(p)
    flags = L.SEL | T | pick
    r = ev.eval(a["cpu"], a["mem"], a["sel"], None, a["smp"] if pick else None, flags)
    (name, args), = calls_of(ev)
    assert name == "ksched_eval" and args[:2] == (H, p) and args[8] == flags and args[7] == (A if pick else 0)
    assert args[2:5] == (a["cpu"].ctypes.data, a["mem"].ctypes.data, a["sel"].ctypes.data) and args[5] is None
    assert args[9] == r.feasible.ctypes.data and args[10] is None and (args[11] == r.binding.ctypes.data if pick else args[11] is None)


def test_every_refusal_is_a_value_error_naming_the_argument_before_any_library_call():
    p = 9
    ev = make_evaluator()
    pipe = make_pipe(ev)
    a = device_args(p, L.PICK_UNIFORM)
    h = host_args(p)
    batch = (a["cpu"], a["mem"], a["sel"], None, a["smp"])
    flags = L.SEL | T | L.PICK_UNIFORM
    no_sel = T | L.PICK_UNIFORM
    dev_kw = dict(out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM)
    bound_kw = dict(out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM)
    refused = {
        "flags": [lambda: ev.eval_device(*batch, flags | L.SELOP_EXISTS, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.SELOP_GT, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.SELOP_LT, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.SELOP_ANY, **dev_kw),
                  lambda: ev.eval_device(*batch, no_sel, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.FIT, **dev_kw),
                  lambda: ev.eval_device(a["cpu"], a["mem"], a["sel"], a["tol"], a["smp"], flags | L.TAINT, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.COMBINE_AND | L.FIT, **dev_kw),
                  lambda: ev.bind_eval_device(*batch, flags | L.SELOP_GT, **bound_kw),
                  lambda: ev.bind_eval_device(*batch, no_sel, **bound_kw),
                  lambda: ev.bind_eval_device(*batch, flags | L.FIT, **bound_kw),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], flags | L.SELOP_LT),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], no_sel),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], flags | L.FIT),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], h["tol"], h["smp"], flags | L.TAINT),
                  lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], flags | L.COMBINE_AND),  # (the host form combines nothing)
                  lambda: pipe.submit(0, *batch, flags, a["mask"], a["bind"]),
                  lambda: pipe.submit(0, *batch, L.FIT | flags, a["mask"], a["bind"]),
                  lambda: pipe.bind(*batch, flags, [a["mask"], a["mask"]], [a["bind"], a["bind"]]),
                  lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | T, a["bind"], samples=a["smp"], stream=STREAM),
                  lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | L.SEL | T, a["bind"], samples=a["smp"], stream=STREAM),
                  lambda: ev.pick(h["feas"], L.PICK_UNIFORM | L.SEL | T, samples=h["smp"]),
                  lambda: ev.summarize(h["cpu"], h["mem"], h["sel"], None, L.SEL | T),
                  lambda: ev.summarize_device(a["cpu"], a["mem"], a["sel"], None, L.SEL | T, out=a["table"], stream=STREAM),
                  lambda: ev.explain(h["cpu"], h["mem"], h["sel"], None, [0], [1], L.SEL | T)],
        "out_fit": [lambda: ev.eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.eval_device(*batch, flags | L.WANT_FIT_MASK, **dev_kw),
                    lambda: ev.bind_eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_bindings=[a["bind"]], stream=STREAM),
                    lambda: ev.eval(h["cpu"], h["mem"], h["sel"], None, h["smp"], flags | L.WANT_FIT_MASK)],
        # the combining call's own refusals, with the flag beside the op
        "out_feasible": [lambda: ev.eval_device(*batch, flags | L.COMBINE_AND, out_binding=a["bind"], stream=STREAM),
                         lambda: ev.bind_eval_device(*batch, flags | L.COMBINE_ANDNOT | L.COMBINE_SOFT, out_bindings=[a["bind"]], stream=STREAM)],
    }
    for name, calls in refused.items():
        for i, call in enumerate(calls):
            with pytest.raises(ValueError, match=name):
                call()
                pytest.fail(f"{name}: refusal {i} was accepted")
    for where, call in (("Pipe.submit", lambda: pipe.submit(0, *batch, flags, a["mask"], a["bind"])),
                        ("Evaluator.pick_device", lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | T, a["bind"], samples=a["smp"], stream=STREAM)),
                        ("Evaluator.pick", lambda: ev.pick(h["feas"], L.PICK_UNIFORM | T, samples=h["smp"])),
                        ("Evaluator.summarize", lambda: ev.summarize(h["cpu"], h["mem"], h["sel"], None, L.SEL | T)),
                        ("Evaluator.summarize_device", lambda: ev.summarize_device(a["cpu"], a["mem"], a["sel"], None, L.SEL | T, out=a["table"], stream=STREAM)),
                        ("Evaluator.explain", lambda: ev.explain(h["cpu"], h["mem"], h["sel"], None, [0], [1], L.SEL | T))):
        with pytest.raises(ValueError, match="flags: " + where.replace(".", r"\.") + " takes no SELOP_TAGGED"):
            call()
    assert calls_of(ev) == [], "a refused call reaches no library function"
    assert np.array_equal(h["feas"], np.zeros_like(h["feas"]))


def test_the_entry_helper_round_trips():
    assert (L.SELTAG_SHIFT, L.SELTAG_ID_MASK) == (29, 0x1FFFFFFF)
    assert (L.SELTAG_EQ, L.SELTAG_NE, L.SELTAG_EXISTS, L.SELTAG_ABSENT, L.SELTAG_GT, L.SELTAG_LT) == (0, 1, 2, 3, 4, 5)
    ids = np.array([0, 1, 2, 1000, 0x1FFFFFFE, 0x1FFFFFFF], dtype=np.uint32)
    for tag in range(6):
        e = pkg.seltag(tag, ids)
        assert e.dtype == np.uint32 and e.shape == ids.shape
        assert np.array_equal(e >> L.SELTAG_SHIFT, np.full(ids.shape, tag)) and np.array_equal(e & L.SELTAG_ID_MASK, ids)
    # a tag per element, broadcasting, scalars, lists and int64 input
    tags = np.arange(6)[:, None]
    e = pkg.seltag(tags, ids[None, :])
    assert e.shape == (6, 6) and np.array_equal(e >> 29, np.broadcast_to(tags, (6, 6))) and np.array_equal(e & 0x1FFFFFFF, np.broadcast_to(ids, (6, 6)))
    assert int(pkg.seltag(L.SELTAG_GT, 16)) == 0x80000010 and pkg.seltag(L.SELTAG_GT, 16).shape == ()
    assert pkg.seltag([L.SELTAG_NE, L.SELTAG_LT], [3, 4]).tolist() == [0x20000003, 0xA0000004]
    assert pkg.seltag(np.int64(L.SELTAG_ABSENT), np.array([0], np.int64)).tolist() == [0x60000000]
    # EQ with id 0 is the unconstrained entry; every entry the helper builds lies below tag 6, so none is SEL_NEVER
    assert int(pkg.seltag(L.SELTAG_EQ, 0)) == 0
    assert int(pkg.seltag(L.SELTAG_LT, L.SELTAG_ID_MASK)) == 0xBFFFFFFF < 0xC0000000 <= L.SEL_NEVER
    assert pkg.seltag(np.zeros((0,), np.int64), np.zeros((0,), np.int64)).shape == (0,)


def test_the_entry_helper_refuses_what_an_entry_cannot_hold():
    for tag in (6, 7, 8, -1, 1 << 31):
        with pytest.raises(ValueError, match="tag"):
            pkg.seltag(tag, 1)
    with pytest.raises(ValueError, match="tag"):
        pkg.seltag([0, 5, 6], [1, 1, 1])
    for ident in (0x20000000, 0x20000001, 0xFFFFFFFF, -1, 1 << 40):
        with pytest.raises(ValueError, match="ids"):
            pkg.seltag(L.SELTAG_EQ, ident)
    with pytest.raises(ValueError, match="ids"):
        pkg.seltag(L.SELTAG_GT, np.array([1, 0x20000000], dtype=np.uint32))
    with pytest.raises(ValueError, match="integers"):
        pkg.seltag(1.0, 1)
    with pytest.raises(ValueError, match="integers"):
        pkg.seltag(1, np.array([1.5]))
