"""Caller's arrays -> checked pointers: the one place where the binding turns a tensor or a numpy array into an address.

The C ABI receives bare pointers and a pod count and cannot know how large a buffer is, so this is the boundary at which a wrong shape,
dtype, device or row pitch can still be refused (ValueError naming the argument) before it becomes an out-of-bounds access.  Every
rule is stated once here; evaluator.py and dist.py call nothing else to obtain an address.  torch is imported on first use only.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from . import _lib as L

DRAWS = L.PICK_DRAWS  # the picks that read `samples`
COMBINE = L.COMBINE_ANY  # the flags that fold a call's evaluation into the caller's mask (extension E6)

# element kinds of the C ABI: the torch dtypes that may stand for them (int64 stands in for uint64, int32 for uint32, bool for uint8)
KINDS = {"i64": ("int64",), "u64": ("int64", "uint64"), "i32": ("int32",), "u32": ("int32", "uint32"), "u8": ("uint8", "bool")}
_NP = {"i64": np.int64, "u64": np.uint64, "i32": np.int32, "u32": np.uint32}
_torch_kinds = {}


def _dtypes(kind: str):
    if not _torch_kinds:
        import torch
        _torch_kinds.update({k: tuple(getattr(torch, n) for n in names) for k, names in KINDS.items()})
    return _torch_kinds[kind]


def _on_device(t, name: str, kind: str, device: int):
    if not t.is_cuda or t.device.index != device or t.dtype not in _dtypes(kind):
        raise ValueError(f"{name}: expected a {'/'.join(KINDS[kind])} CUDA tensor on cuda:{device}, got {t.dtype} on {t.device}")


def device_ptr(t, name: str, kind: str, shape, device: int) -> Optional[int]:
    """Address of a contiguous CUDA tensor of `kind` on cuda:`device` with exactly `shape` (None: any shape); None for an absent
    tensor (and for an empty one, whose address nobody reads)."""
    if t is None:
        return None
    _on_device(t, name, kind, device)
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor, got strides {tuple(t.stride())}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr() or None


def mask_rows(p: int, W: int, device: int, *named_masks):
    """([address or None per (name, mask)], row pitch in words) of the [p, W] mask views of one call: int64/uint64 CUDA tensors with unit
    column stride, rows `pitch` >= W words apart, one pitch for all of them.  A single row (or none) has no pitch of its own: W."""
    ptrs, pitch = [], None
    for name, t in named_masks:
        if t is not None:
            _on_device(t, name, "u64", device)
            if tuple(t.shape) != (p, W) or (W and t.stride(1) != 1) or (p > 1 and t.stride(0) < W):
                raise ValueError(f"{name}: expected a [{p}, {W}] view with unit column stride and rows at least {W} words apart, "
                                 f"got {tuple(t.shape)} with strides {tuple(t.stride())}")
            tp = int(t.stride(0)) if p > 1 else W
            if pitch is not None and tp != pitch:
                raise ValueError(f"{name}: every mask of one call must have the same row pitch ({tp} != {pitch})")
            pitch = tp
        ptrs.append(None if t is None else t.data_ptr() or None)
    return ptrs, W if pitch is None else pitch


def host_array(a, name: str, kind: str, shape=None):
    """C-contiguous numpy array of `kind` from whatever the caller passed (lists and strided arrays are converted), None for None;
    `shape`: the exact shape, an entry None = any length."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=_NP[kind])
    if shape is not None and (a.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, a.shape))):
        raise ValueError(f"{name}: expected shape [{', '.join('*' if s is None else str(s) for s in shape)}], got {list(a.shape)}")
    return a


def host_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _vp(address: Optional[int]):
    return None if address is None else C.c_void_p(address)


def draws(samples, name: str, flags: int, p: int, device: Optional[int] = None):
    """(address, attempts, what the address points into): `samples` is read exactly when flags carry PICK_SAMPLED (node indices),
    PICK_UNIFORM (32-bit draws, column 0) or PICK_SPREAD / PICK_PACK (32-bit draws, every column) and must then be a contiguous [p, attempts >= 1] uint32 array (device None: whatever numpy
    converts) or CUDA tensor on cuda:`device`; a wrong shape would be an out-of-bounds read.  Without such a flag attempts is 0 and
    nothing reads it, whatever its shape."""
    if device is None:
        samples = host_array(samples, name, "u32")
    attempts = 0
    if flags & DRAWS:
        if samples is None or len(samples.shape) != 2 or int(samples.shape[0]) != p or int(samples.shape[1]) < 1:
            raise ValueError(f"{name}: expected a contiguous [{p}, attempts >= 1] array with KSCHED_PICK_SAMPLED / KSCHED_PICK_UNIFORM / KSCHED_PICK_SPREAD / KSCHED_PICK_PACK, "
                             f"got {None if samples is None else tuple(samples.shape)}")
        attempts = int(samples.shape[1])
    return host_ptr(samples) if device is None else _vp(device_ptr(samples, name, "u32", None, device)), attempts, samples


def combine(flags: int, where: str, accepted: bool, out_feasible=None, out_fit=None) -> None:
    """The one rule of COMBINE_AND / COMBINE_OR / COMBINE_ANDNOT (include/ksched.h, extension E6), before any library call: only
    `eval_device` / `bind_eval_device` accept them (accepted=True) -- a host mask would first have to travel to the device, a pipe slot's
    mask belongs to the slot --, at most one per call, `out_feasible` is required (it is read and written: the caller's mask from earlier
    calls) and WANT_FIT_MASK / `out_fit` are excluded (a combining call writes one mask).  ValueError naming the argument."""
    c = int(flags) & COMBINE
    if not c:
        return
    if not accepted:
        raise ValueError(f"flags: {where} takes no COMBINE_AND / COMBINE_OR / COMBINE_ANDNOT (the mask is combined on the device: Evaluator.eval_device)")
    if c & (c - 1):
        raise ValueError(f"flags: at most one of COMBINE_AND / COMBINE_OR / COMBINE_ANDNOT per call, got {c:#x}")
    if out_feasible is None:
        raise ValueError("out_feasible: a COMBINE_* flag needs the mask it combines into")
    if out_fit is not None or int(flags) & L.WANT_FIT_MASK:
        raise ValueError("out_fit: a COMBINE_* flag excludes WANT_FIT_MASK / out_fit")


def soft(flags: int, where: str, accepted: bool) -> None:
    """The rules of COMBINE_SOFT (include/ksched.h, extension E7) that `combine` does not already state, before any library call: only
    `eval_device` / `bind_eval_device` accept the modifier (accepted=True), and only together with COMBINE_AND or COMBINE_ANDNOT -- it
    modifies an op, and COMBINE_OR cannot empty a row.  Everything a combining call needs (`combine`) it needs too.  ValueError naming the
    argument; a word without the modifier passes."""
    if not int(flags) & L.COMBINE_SOFT:
        return
    if not accepted:
        raise ValueError(f"flags: {where} takes no COMBINE_SOFT (the mask is combined on the device: Evaluator.eval_device)")
    if int(flags) & COMBINE not in (L.COMBINE_AND, L.COMBINE_ANDNOT):
        raise ValueError(f"flags: COMBINE_SOFT modifies COMBINE_AND or COMBINE_ANDNOT, got {int(flags) & COMBINE:#x} beside it")


def selop(flags: int, where: str, accepted: bool, out_fit=None) -> None:
    """The one rule of SELOP_EXISTS / SELOP_GT / SELOP_LT (include/ksched.h, extension E8), before any library call: the evaluations accept
    them (accepted=True: `eval`, `eval_device`, `bind_eval_device`), the pipe, the picks, the summaries and `explain` do not; at most one
    per call; SEL is required -- the operator is a reading of the selector entries --; FIT, TAINT and WANT_FIT_MASK / `out_fit` are
    excluded: the call answers the selector term alone, fit and taints are combined in from another call.  ValueError naming the
    argument; a word without an operator flag passes."""
    o = int(flags) & L.SELOP_ANY
    if not o:
        return
    if not accepted:
        raise ValueError(f"flags: {where} takes no SELOP_EXISTS / SELOP_GT / SELOP_LT (an operator call is an evaluation: Evaluator.eval, Evaluator.eval_device)")
    if o & (o - 1):
        raise ValueError(f"flags: at most one of SELOP_EXISTS / SELOP_GT / SELOP_LT per call, got {o:#x}")
    if not int(flags) & L.SEL:
        raise ValueError("flags: a SELOP_* flag needs SEL (it says how the selector entries are read)")
    if int(flags) & (L.FIT | L.TAINT):
        raise ValueError("flags: a SELOP_* flag excludes FIT and TAINT (combine them in from another call: COMBINE_AND)")
    if out_fit is not None or int(flags) & L.WANT_FIT_MASK:
        raise ValueError("out_fit: a SELOP_* flag excludes WANT_FIT_MASK / out_fit")


def seltag(flags: int, where: str, accepted: bool, out_fit=None) -> None:
    """The one rule of SELOP_TAGGED (include/ksched.h, extension E9), before any library call: the evaluations accept it (accepted=True:
    `eval`, `eval_device`, `bind_eval_device`), the pipe, the picks, the summaries and `explain` do not; no SELOP_EXISTS / SELOP_GT /
    SELOP_LT beside it -- the operator is the entry's or the call's, not both --; SEL is required; FIT, TAINT and WANT_FIT_MASK /
    `out_fit` are excluded: the call answers the selector term alone, fit and taints are combined in from another call.  ValueError
    naming the argument; a word without the flag passes."""
    if not int(flags) & L.SELOP_TAGGED:
        return
    if not accepted:
        raise ValueError(f"flags: {where} takes no SELOP_TAGGED (a tagged call is an evaluation: Evaluator.eval, Evaluator.eval_device)")
    if int(flags) & L.SELOP_ANY:
        raise ValueError(f"flags: SELOP_TAGGED excludes SELOP_EXISTS / SELOP_GT / SELOP_LT, got {int(flags) & L.SELOP_ANY:#x} beside it")
    if not int(flags) & L.SEL:
        raise ValueError("flags: SELOP_TAGGED needs SEL (it says how the selector entries are read)")
    if int(flags) & (L.FIT | L.TAINT):
        raise ValueError("flags: SELOP_TAGGED excludes FIT and TAINT (combine them in from another call: COMBINE_AND)")
    if out_fit is not None or int(flags) & L.WANT_FIT_MASK:
        raise ValueError("out_fit: SELOP_TAGGED excludes WANT_FIT_MASK / out_fit")


def terms_of(flags: int) -> int:
    """the term count of a flag word (extension E10): 0 = no term field"""
    return (int(flags) & L.SEL_TERMS_MASK) >> L.SEL_TERMS_SHIFT


def selterms(flags: int, where: str, accepted: bool, out_fit=None) -> None:
    """The one rule of a term count, `sel_terms(t)` in the flag word (include/ksched.h, extension E10), before any library call: it modifies
    a TAGGED call, so where SELOP_TAGGED is accepted (accepted=True: `eval`, `eval_device`, `bind_eval_device`) it needs SELOP_TAGGED --
    hence SEL, and no SELOP_EXISTS / SELOP_GT / SELOP_LT -- and excludes FIT, TAINT and WANT_FIT_MASK / `out_fit` as a tagged call does;
    the pipe, the picks, the summaries and `explain` do not take it.  ValueError naming the argument; a word without the field passes."""
    t = terms_of(flags)
    if not t:
        return
    if not accepted:
        raise ValueError(f"flags: {where} takes no term count (sel_terms({t}) modifies a tagged call, an evaluation: Evaluator.eval, Evaluator.eval_device)")
    if not int(flags) & L.SELOP_TAGGED:
        raise ValueError(f"flags: a term count (sel_terms({t})) needs SEL | SELOP_TAGGED (it says how many tagged rows a pod has)")
    seltag(flags, where, accepted, out_fit)


def _sel_shapes(n_keys: int, p: int, flags: int):
    """the shapes sel_val_ids may have: [n_keys, p]; with a term count T (extension E10) [T, n_keys, p] or [T * n_keys, p] -- the library
    reads T * n_keys * p entries, so any other shape would be an out-of-bounds read"""
    t = terms_of(flags)
    return ((n_keys, p),) if not t else ((t, n_keys, p), (t * n_keys, p))


def _sel_shape_error(name: str, got, shapes, flags: int) -> ValueError:
    what = " or ".join(str(list(s)) for s in shapes)
    return ValueError(f"{name}: expected shape {what}" + (f" with sel_terms({terms_of(flags)})" if terms_of(flags) else "") + f", got {list(got)}")


class Batch(NamedTuple):
    """One pod batch as the C ABI takes it; [:8] is the argument run every evaluation entry point shares."""
    p: int
    cpu: Optional[C.c_void_p]
    mem: Optional[C.c_void_p]
    sel: Optional[C.c_void_p]
    tol: Optional[C.c_void_p]
    smp: Optional[C.c_void_p]
    attempts: int
    flags: int
    keep: tuple  # what the addresses point into


def _rows(req_cpu, name: str, p: Optional[int]) -> int:
    if p is not None:
        return int(p)
    if req_cpu is None or len(req_cpu.shape) != 1:
        raise ValueError(f"{name}: expected a 1-D array of the pods' requests, got {None if req_cpu is None else tuple(req_cpu.shape)}")
    return int(req_cpu.shape[0])


def device_batch(device: int, n_keys: int, req_cpu, req_mem, sel_val_ids, tolerations, samples, flags: int, p: Optional[int] = None) -> Batch:
    """torch CUDA tensors on cuda:`device`: requests int64 [p], sel_val_ids int32/uint32 [n_keys, p] ([T, n_keys, p] or [T * n_keys, p]
    where flags carry a term count T, extension E10), tolerations int64/uint64 [p], samples int32/uint32 [p, attempts] (see draws); any of
    them may be None.  p = len(req_cpu) unless given (the pick alone)."""
    p = _rows(req_cpu, "req_cpu_milli", p)
    smp, attempts, _ = draws(samples, "samples", flags, p, device)
    sel_shape = (n_keys, p)
    if sel_val_ids is not None and terms_of(flags):
        shapes = _sel_shapes(n_keys, p, flags)
        if tuple(sel_val_ids.shape) not in shapes:
            raise _sel_shape_error("sel_val_ids", sel_val_ids.shape, shapes, flags)
        sel_shape = tuple(sel_val_ids.shape)
    cols = ((req_cpu, "req_cpu_milli", "i64", (p,)), (req_mem, "req_mem_bytes", "i64", (p,)), (sel_val_ids, "sel_val_ids", "u32", sel_shape),
            (tolerations, "tolerations", "u64", (p,)))
    return Batch(p, *[_vp(device_ptr(*col, device)) for col in cols], smp, attempts, int(flags), (req_cpu, req_mem, sel_val_ids, tolerations, samples))


def host_batch(n_keys: int, req_cpu, req_mem, sel_val_ids, tolerations, samples, flags: int, p: Optional[int] = None) -> Batch:
    """The same batch from host memory: whatever numpy converts, every column 1-D of length p, sel_val_ids [n_keys][p] ([T][n_keys][p] or
    [T * n_keys][p] where flags carry a term count T, extension E10)."""
    cpu = host_array(req_cpu, "req_cpu_milli", "i64")
    p = _rows(cpu, "req_cpu_milli", p)
    smp, attempts, samples = draws(samples, "samples", flags, p)
    sel = host_array(sel_val_ids, "sel_val_ids", "u32", None if terms_of(flags) else (n_keys, p))
    if sel is not None and terms_of(flags) and tuple(sel.shape) not in _sel_shapes(n_keys, p, flags):
        raise _sel_shape_error("sel_val_ids", sel.shape, _sel_shapes(n_keys, p, flags), flags)
    keep = (cpu, host_array(req_mem, "req_mem_bytes", "i64", (p,)), sel,
            host_array(tolerations, "tolerations", "u64", (p,)))
    return Batch(p, *map(host_ptr, keep), smp, attempts, int(flags), keep + (samples,))
