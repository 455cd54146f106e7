"""A term count (`sel_terms(t)`, extension E10) through the binding's argument checks (kube_scheduler_rs_reference_amd/_marshal.py), without
a GPU: over the stand-in tensors and the recording stub of tests/test_marshal_host.py.  The rule (_marshal.selterms, beside
_marshal.seltag): the evaluations -- Evaluator.eval, eval_device, bind_eval_device -- accept the field beside SEL | SELOP_TAGGED and
nowhere else; Pipe.submit / bind, the picks, the summaries and explain refuse it.  The shape: with the field saying T, sel_val_ids is a
contiguous [T, n_keys, p] or [T * n_keys, p] array or tensor and nothing else -- the library reads T * n_keys * p entries, any other shape
would be an out-of-bounds read.  Every refusal is a ValueError naming the argument and reaches no library function; an accepted call
passes the flag word and the selectors' address through unchanged."""
import numpy as np
import pytest
import torch

import kube_scheduler_rs_reference_amd as pkg
from kube_scheduler_rs_reference_amd import _lib as L
from kube_scheduler_rs_reference_amd import _marshal as M
from tests.test_marshal_host import (A, H, N_KEYS, STREAM, calls_of, dev, device_args, host_args, make_evaluator, make_pipe, ptrs, strided)

TG = L.SEL | L.SELOP_TAGGED
COMBINES = [0, L.COMBINE_AND, L.COMBINE_OR, L.COMBINE_ANDNOT, L.COMBINE_AND | L.COMBINE_SOFT, L.COMBINE_ANDNOT | L.COMBINE_SOFT]


def test_the_constants_and_the_field_helper():
    assert (L.SEL_TERMS_SHIFT, L.SEL_TERMS_MASK, L.MAX_TERMS) == (20, 0x00F00000, 15)
    assert [L.sel_terms(t) for t in (1, 2, 15)] == [0x100000, 0x200000, 0xF00000] and pkg.sel_terms is L.sel_terms
    for bad in (0, -1, 16, 255):
        with pytest.raises(ValueError, match="sel_terms"):
            L.sel_terms(bad)
    assert M.terms_of(0) == 0 and M.terms_of(TG) == 0 and M.terms_of(TG | L.sel_terms(7) | L.PICK_PACK) == 7 and M.terms_of(0xFFFFFFFF) == 15


def test_the_rule_itself():
    for t in (1, 2, 15):
        f = TG | L.sel_terms(t)
        for comb in COMBINES:
            for pick in (0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_UNIFORM, L.PICK_SPREAD, L.PICK_PACK):
                assert M.selterms(f | comb | pick, "here", accepted=True) is None
        with pytest.raises(ValueError, match="flags: here takes no term count"):
            M.selterms(f, "here", accepted=False)
        # the field without SELOP_TAGGED: a plain call, an operator call, nothing at all
        for rest in (0, L.SEL, L.FIT | L.SEL, L.SEL | L.SELOP_GT, L.PICK_UNIFORM):
            with pytest.raises(ValueError, match="flags.*needs SEL \\| SELOP_TAGGED"):
                M.selterms(rest | L.sel_terms(t), "here", accepted=True)
        # ... and a tagged call's own refusals, with the field beside the flag
        with pytest.raises(ValueError, match="flags.*needs SEL"):
            M.selterms(L.SELOP_TAGGED | L.sel_terms(t), "here", accepted=True)
        for op in (L.SELOP_EXISTS, L.SELOP_GT, L.SELOP_LT):
            with pytest.raises(ValueError, match="flags.*excludes SELOP_EXISTS"):
                M.selterms(f | op, "here", accepted=True)
        for pred in (L.FIT, L.TAINT):
            with pytest.raises(ValueError, match="flags.*FIT"):
                M.selterms(f | pred, "here", accepted=True)
        with pytest.raises(ValueError, match="out_fit"):
            M.selterms(f | L.WANT_FIT_MASK, "here", accepted=True)
        with pytest.raises(ValueError, match="out_fit"):
            M.selterms(f, "here", accepted=True, out_fit=object())
    # without the field the rule says nothing, whatever the rest is
    for flags in (0, TG, TG | L.FIT, L.SELOP_TAGGED, L.SEL | L.SELOP_ANY, 0x1000, 0x20000, 0x80000):
        assert M.selterms(flags, "here", accepted=False) is None and M.selterms(flags, "here", accepted=True, out_fit=object()) is None
    # the other rules say nothing about the field
    f = TG | L.sel_terms(3)
    assert M.seltag(f, "here", accepted=True) is None and M.selop(f, "here", accepted=False) is None
    assert M.combine(f | L.COMBINE_OR, "here", accepted=True, out_feasible=object()) is None


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("t", [1, 3, 15])
@pytest.mark.parametrize("p", [0, 1, 9])
def test_eval_device_passes_the_field_and_the_rows_through(p, t, layout):
    ev = make_evaluator()
    a = device_args(p, L.PICK_SPREAD)
    sel = dev((t, N_KEYS, p) if layout == "3d" else (t * N_KEYS, p), torch.int32)
    flags = TG | L.sel_terms(t) | L.COMBINE_OR | L.PICK_SPREAD
    want = ("ksched_eval_device_pitched", (H, p, *ptrs(a, "cpu", "mem"), sel.data_ptr() or None, None, *ptrs(a, "smp"), A, flags, *ptrs(a, "mask"), None,
                                           a["bind"].data_ptr() or None, a["pitch"], STREAM.cuda_stream))
    ev.eval_device(a["cpu"], a["mem"], sel, None, a["smp"], flags, out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM)
    ev.bind_eval_device(a["cpu"], a["mem"], sel, None, a["smp"], flags, out_feasible=[a["mask"]], out_bindings=[a["bind"]], stream=STREAM)(0, 0)
    assert calls_of(ev) == [want, want]
    # no selectors at all: every node passes, nothing to read
    ev.eval_device(a["cpu"], a["mem"], None, None, None, TG | L.sel_terms(t), out_feasible=a["mask"], stream=STREAM)
    assert calls_of(ev)[-1][1][4] is None


@pytest.mark.parametrize("t", [1, 4])
def test_the_host_form_passes_the_field_and_the_rows_through(t):
    p = 9
    ev = make_evaluator()
    h = host_args(p)
    for sel in (np.zeros((t, N_KEYS, p), np.uint32), np.zeros((t * N_KEYS, p), np.uint32)):
        flags = TG | L.sel_terms(t)
        ev.eval(h["cpu"], h["mem"], sel, None, None, flags)
        name, args = calls_of(ev)[-1]
        assert name == "ksched_eval" and args[:2] == (H, p) and args[8] == flags and args[4] == sel.ctypes.data
    # whatever numpy converts: nested lists, and a strided array is made contiguous with all T * n_keys * p entries
    big = np.arange(t * N_KEYS * p * 2, dtype=np.uint32).reshape(t, N_KEYS, 2 * p)[:, :, ::2]
    ev.eval(h["cpu"], h["mem"], big, None, None, TG | L.sel_terms(t))
    ev.eval(h["cpu"], h["mem"], big.tolist(), None, None, TG | L.sel_terms(t))
    assert len(calls_of(ev)) == 4


def test_a_wrong_shape_is_refused_before_any_library_call():
    p, t = 9, 3
    ev = make_evaluator()
    a = device_args(p, L.PICK_SPREAD)
    h = host_args(p)
    f = TG | L.sel_terms(t)
    kw = dict(out_feasible=a["mask"], stream=STREAM)
    bad_shapes = [(N_KEYS, p), (t - 1, N_KEYS, p), (t + 1, N_KEYS, p), (t, N_KEYS, p - 1), (t, N_KEYS + 1, p), (t * N_KEYS + 1, p), (t * N_KEYS, p + 1),
                  (t * N_KEYS * p,), (1, t, N_KEYS, p), (N_KEYS, t, p)[::-1]]
    for shape in bad_shapes:
        with pytest.raises(ValueError, match="sel_val_ids"):
            ev.eval_device(a["cpu"], a["mem"], dev(shape, torch.int32), None, None, f, **kw)
        with pytest.raises(ValueError, match="sel_val_ids"):
            ev.bind_eval_device(a["cpu"], a["mem"], dev(shape, torch.int32), None, None, f, out_feasible=[a["mask"]], stream=STREAM)
        with pytest.raises(ValueError, match="sel_val_ids"):
            ev.eval(h["cpu"], h["mem"], np.zeros(shape, np.uint32), None, None, f)
    # a term-shaped array without the field, and a [n_keys, p] one with it
    with pytest.raises(ValueError, match="sel_val_ids"):
        ev.eval_device(a["cpu"], a["mem"], dev((t, N_KEYS, p), torch.int32), None, None, TG, **kw)
    with pytest.raises(ValueError, match="sel_val_ids"):
        ev.eval(h["cpu"], h["mem"], np.zeros((t, N_KEYS, p), np.uint32), None, None, TG)
    # the right shape in the wrong dtype, on the wrong device, or not contiguous
    with pytest.raises(ValueError, match="sel_val_ids"):
        ev.eval_device(a["cpu"], a["mem"], dev((t, N_KEYS, p), torch.int64), None, None, f, **kw)
    with pytest.raises(ValueError, match="sel_val_ids"):
        ev.eval_device(a["cpu"], a["mem"], dev((t, N_KEYS, p), torch.int32, index=1), None, None, f, **kw)
    with pytest.raises(ValueError, match="sel_val_ids.*contiguous"):
        ev.eval_device(a["cpu"], a["mem"], strided((t, N_KEYS, p), torch.int32), None, None, f, **kw)
    assert calls_of(ev) == [], "a refused call reaches no library function"


def test_every_refusal_of_the_field_is_a_value_error_naming_the_argument_before_any_library_call():
    p, t = 9, 2
    ev = make_evaluator()
    pipe = make_pipe(ev)
    a = device_args(p, L.PICK_UNIFORM)
    h = host_args(p)
    sel, hsel = dev((t, N_KEYS, p), torch.int32), np.zeros((t, N_KEYS, p), np.uint32)
    F = L.sel_terms(t)
    flags = TG | F | L.PICK_UNIFORM
    batch = (a["cpu"], a["mem"], sel, None, a["smp"])
    dev_kw = dict(out_feasible=a["mask"], out_binding=a["bind"], stream=STREAM)
    refused = {
        "flags": [lambda: ev.eval_device(*batch, L.SEL | F | L.PICK_UNIFORM, **dev_kw),                       # no SELOP_TAGGED
                  lambda: ev.eval_device(*batch, L.SELOP_TAGGED | F | L.PICK_UNIFORM, **dev_kw),              # no SEL
                  lambda: ev.eval_device(*batch, L.FIT | F | L.PICK_UNIFORM, **dev_kw),
                  lambda: ev.eval_device(*batch, L.SEL | L.SELOP_GT | F | L.PICK_UNIFORM, **dev_kw),          # an operator call
                  lambda: ev.eval_device(*batch, flags | L.SELOP_EXISTS, **dev_kw),
                  lambda: ev.eval_device(*batch, flags | L.FIT, **dev_kw),
                  lambda: ev.eval_device(a["cpu"], a["mem"], sel, a["tol"], a["smp"], flags | L.TAINT, **dev_kw),
                  lambda: ev.bind_eval_device(*batch, L.SEL | F | L.PICK_UNIFORM, out_feasible=a["mask"], out_bindings=[a["bind"]], stream=STREAM),
                  lambda: ev.eval(h["cpu"], h["mem"], hsel, None, h["smp"], L.SEL | F | L.PICK_UNIFORM),
                  lambda: ev.eval(h["cpu"], h["mem"], hsel, None, h["smp"], flags | L.FIT),
                  lambda: ev.eval(h["cpu"], h["mem"], hsel, None, h["smp"], flags | L.COMBINE_OR),  # (the host form combines nothing)
                  lambda: pipe.submit(0, *batch, flags, a["mask"], a["bind"]),
                  lambda: pipe.bind(*batch, flags, [a["mask"], a["mask"]], [a["bind"], a["bind"]]),
                  lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | F, a["bind"], samples=a["smp"], stream=STREAM),
                  lambda: ev.pick(h["feas"], L.PICK_UNIFORM | F, samples=h["smp"]),
                  lambda: ev.summarize(h["cpu"], h["mem"], hsel, None, L.SEL | F),
                  lambda: ev.summarize_device(a["cpu"], a["mem"], sel, None, L.SEL | F, out=a["table"], stream=STREAM),
                  lambda: ev.explain(h["cpu"], h["mem"], hsel, None, [0], [1], L.SEL | F)],
        "out_fit": [lambda: ev.eval_device(*batch, flags, out_feasible=a["mask"], out_fit=a["fit"], out_binding=a["bind"], stream=STREAM),
                    lambda: ev.eval_device(*batch, flags | L.WANT_FIT_MASK, **dev_kw),
                    lambda: ev.eval(h["cpu"], h["mem"], hsel, None, h["smp"], flags | L.WANT_FIT_MASK)],
        "out_feasible": [lambda: ev.eval_device(*batch, flags | L.COMBINE_OR, out_binding=a["bind"], stream=STREAM)],
    }
    for name, calls in refused.items():
        for i, call in enumerate(calls):
            with pytest.raises(ValueError, match=name):
                call()
                pytest.fail(f"{name}: refusal {i} was accepted")
    # where a tagged call is refused, the field without the flag is refused for itself
    for where, call in (("Pipe.submit", lambda: pipe.submit(0, *batch, L.FIT | F | L.PICK_UNIFORM, a["mask"], a["bind"])),
                        ("Evaluator.pick_device", lambda: ev.pick_device(a["mask"], L.PICK_UNIFORM | F, a["bind"], samples=a["smp"], stream=STREAM)),
                        ("Evaluator.pick", lambda: ev.pick(h["feas"], L.PICK_UNIFORM | F, samples=h["smp"])),
                        ("Evaluator.summarize", lambda: ev.summarize(h["cpu"], h["mem"], hsel, None, L.SEL | F)),
                        ("Evaluator.summarize_device", lambda: ev.summarize_device(a["cpu"], a["mem"], sel, None, L.SEL | F, out=a["table"], stream=STREAM)),
                        ("Evaluator.explain", lambda: ev.explain(h["cpu"], h["mem"], hsel, None, [0], [1], L.SEL | F))):
        with pytest.raises(ValueError, match="flags: " + where.replace(".", r"\.") + " takes no term count"):
            call()
    assert calls_of(ev) == [], "a refused call reaches no library function"
