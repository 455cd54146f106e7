"""Python face of the C ABI: `Evaluator` owns one `ksched_ctx` (one GPU).

Two call styles, both straight through the C ABI (include/ksched.h):
  * `eval(...)`        numpy arrays in host memory -> ksched_eval        (copies in/out, synchronous)
  * `eval_device(...)` torch CUDA tensors          -> ksched_eval_device (enqueue on torch's stream)
torch is used only as the owner of device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L


def mask_words(n_nodes: int) -> int:
    return (int(n_nodes) + 63) // 64


def _np(a, dtype, name):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_DRAWS = L.PICK_SAMPLED | L.PICK_UNIFORM                 # the picks that read `samples`
_PICKS = L.PICK_SAMPLED | L.PICK_BESTFIT | L.PICK_UNIFORM  # at most one per call


def _attempts(samples, flags: int, p: int) -> int:
    """Draws per pod of a device `samples` tensor (PICK_SAMPLED: node indices; PICK_UNIFORM: 32-bit draws, column 0 is read); a wrong
    shape would be an out-of-bounds device read, so it is refused here."""
    if not (flags & _DRAWS):
        return 0
    if samples is None or samples.dim() != 2 or int(samples.shape[0]) != p or int(samples.shape[1]) == 0 or not samples.is_contiguous():
        raise ValueError(f"samples must be a contiguous [{p}, attempts] tensor with KSCHED_PICK_SAMPLED / KSCHED_PICK_UNIFORM")
    return int(samples.shape[1])


def _apply_args(ev, bindings, req_cpu, req_mem, ok, status_out):
    """(count, bindings, req_cpu, req_mem, ok, status_out) of one apply on `ev`'s device (one rank's rows of a sharded one), checked: all
    [count] contiguous CUDA tensors, bindings int32, requests int64, ok uint8/bool, status_out int32.  Pointers as ints, None for an absent
    tensor (and may be None when count is 0)."""
    import torch
    if bindings.dim() != 1:
        raise ValueError("bindings must be a 1-D int32 tensor")
    p = int(bindings.shape[0])

    def dp(t, dtypes, name):
        if t is None:
            return None
        if not t.is_cuda or t.device.index != ev.device or not t.is_contiguous() or t.dtype not in dtypes:
            raise ValueError(f"{name}: expected a contiguous {dtypes} CUDA tensor on cuda:{ev.device}")
        if tuple(t.shape) != (p,):
            raise ValueError(f"{name}: expected shape ({p},), got {tuple(t.shape)}")
        return t.data_ptr() or None
    return (p, dp(bindings, (torch.int32,), "bindings"), dp(req_cpu, (torch.int64,), "req_cpu"), dp(req_mem, (torch.int64,), "req_mem"),
            dp(ok, (torch.uint8, torch.bool), "ok"), dp(status_out, (torch.int32,), "status_out"))


@dataclass
class EvalResult:
    feasible: Optional[np.ndarray] = None  # [P, W] uint64
    fit: Optional[np.ndarray] = None       # [P, W] uint64
    binding: Optional[np.ndarray] = None   # [P] int32


class Evaluator:
    def __init__(self, device: int = 0):
        self._lib = L.load()
        h = C.c_void_p()
        rc = self._lib.ksched_create(C.byref(h), int(device))
        if rc != L.OK:
            raise L.KschedError(rc, "ksched_create")
        self._h = h
        self.device = int(device)
        self.n = 0
        self.n_keys = 0
        if os.environ.get("KSCHED_DEBUG"):  # A/B switches of tools/ (KSCHED_OPT_DEBUG), so that a whole test file can run under one
            import sys
            print(f"kube_scheduler_rs_reference_amd: KSCHED_DEBUG={os.environ['KSCHED_DEBUG']} -> KSCHED_OPT_DEBUG (ablation switches: timings "
                  "and possibly results are not the shipped path's)", file=sys.stderr)
            self.set_option(L.OPT_DEBUG, int(os.environ["KSCHED_DEBUG"], 0))

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.ksched_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, where: str):
        if rc != L.OK:
            raise L.KschedError(rc, where, self._lib.ksched_last_error(self._h).decode())

    # -- options / introspection ---------------------------------------------------------------
    def set_option(self, option: int, value: int):
        self._check(self._lib.ksched_set_option(self._h, option, value), "ksched_set_option")

    def forget_stream(self, stream):
        """Call BEFORE destroying a stream evaluations were enqueued on while this evaluator lives (ksched_forget_stream)."""
        self._check(self._lib.ksched_forget_stream(self._h, C.c_void_p(stream.cuda_stream)), "ksched_forget_stream")

    def set_kernel(self, name: str):
        self.set_option(L.OPT_KERNEL, {"auto": L.KERNEL_AUTO, "direct": L.KERNEL_DIRECT, "fused": L.KERNEL_FUSED}[name])

    def set_timing(self, on, every: int = 1):
        """Events on every `every`-th mask kernel launch (0 / False = off)."""
        self.set_option(L.OPT_TIMING, int(every) if on else 0)

    def kernel_time_ms(self):
        ms = C.c_double(0)
        cnt = C.c_uint64(0)
        self._check(self._lib.ksched_kernel_time_ms(self._h, C.byref(ms), C.byref(cnt)), "ksched_kernel_time_ms")
        return ms.value, cnt.value

    def kernel_time_samples(self, cap: int = 4096) -> np.ndarray:
        """Per-launch durations (ms) of the timed mask kernel launches since the last reset, in launch order."""
        out = np.zeros((cap,), dtype=np.float64)
        n = self._lib.ksched_kernel_time_samples(self._h, out.ctypes.data_as(C.c_void_p), cap)
        if n < 0:
            self._check(n, "ksched_kernel_time_samples")
        return out[:n]

    def trace_read(self, max_blocks: int = 8192) -> np.ndarray:
        """Diagnostics: per-block phase timestamps of the last fused launch (set_option(OPT_TRACE, 1) first)."""
        out = np.zeros((max_blocks, L.TRACE_WORDS), dtype=np.uint64)
        n = self._lib.ksched_trace_read(self._h, out.ctypes.data_as(C.c_void_p), max_blocks)
        if n < 0:
            self._check(n, "ksched_trace_read")
        return out[:n]

    def index_checksum(self):
        """(rows, aux) checksums of the per-tile bitmap index on the device; (0, 0) when the snapshot has none."""
        out = np.zeros((2,), dtype=np.uint64)
        self._check(self._lib.ksched_index_checksum(self._h, out.ctypes.data_as(C.c_void_p)), "ksched_index_checksum")
        return int(out[0]), int(out[1])

    @property
    def last_kernel(self) -> str:
        return self._lib.ksched_last_kernel(self._h).decode()

    @property
    def last_pick(self) -> str:
        """How the latest evaluation's pick ran: "fused-tile" / "fused" (inside the mask launch), "select", "bestfit-rows", "from-mask", "uniform", "none"."""
        return self._lib.ksched_last_pick(self._h).decode()

    @property
    def W(self) -> int:
        return mask_words(self.n)

    # -- snapshot --------------------------------------------------------------------------------
    def set_nodes(self, avail_cpu_milli, avail_mem_bytes, label_val_ids=None, taints=None):
        cpu = _np(avail_cpu_milli, np.int64, "avail_cpu_milli")
        mem = _np(avail_mem_bytes, np.int64, "avail_mem_bytes")
        n = cpu.shape[0]
        if mem.shape != (n,):
            raise ValueError("avail_mem_bytes shape")
        lab = _np(label_val_ids, np.uint32, "label_val_ids")
        n_keys = 0
        if lab is not None:
            if lab.ndim != 2 or lab.shape[1] != n:
                raise ValueError("label_val_ids must be [n_keys][n]")
            n_keys = lab.shape[0]
        tnt = _np(taints, np.uint64, "taints")
        if tnt is not None and tnt.shape != (n,):
            raise ValueError("taints shape")
        rc = self._lib.ksched_set_nodes(self._h, n, _ptr(cpu), _ptr(mem), _ptr(lab) if n_keys else None, n_keys, _ptr(tnt))
        self._check(rc, "ksched_set_nodes")
        self.n = n
        self.n_keys = n_keys

    def update_nodes(self, node_index, avail_cpu_milli, avail_mem_bytes):
        """New `available` values for the listed canonical node indices (ksched_update_nodes)."""
        idx = _np(node_index, np.uint32, "node_index")
        cpu = _np(avail_cpu_milli, np.int64, "avail_cpu_milli")
        mem = _np(avail_mem_bytes, np.int64, "avail_mem_bytes")
        if idx.ndim != 1 or cpu.shape != idx.shape or mem.shape != idx.shape:
            raise ValueError("node_index, avail_cpu_milli, avail_mem_bytes must be 1-D of one length")
        self._check(self._lib.ksched_update_nodes(self._h, idx.shape[0], _ptr(idx), _ptr(cpu), _ptr(mem)), "ksched_update_nodes")

    def update_node_labels(self, node_index, label_val_ids=None, taints=None):
        """New label ids of every key ([n_keys][count]) and, with `taints` ([count]), new taint bits for the listed canonical node
        indices (ksched_update_node_labels); `available` is not touched."""
        idx = _np(node_index, np.uint32, "node_index")
        if idx.ndim != 1:
            raise ValueError("node_index must be 1-D")
        count = idx.shape[0]
        lab = _np(label_val_ids, np.uint32, "label_val_ids")
        if lab is not None and (lab.ndim != 2 or lab.shape != (self.n_keys, count)):
            raise ValueError(f"label_val_ids must be [{self.n_keys}][{count}]")
        tnt = _np(taints, np.uint64, "taints")
        if tnt is not None and tnt.shape != (count,):
            raise ValueError("taints shape")
        rc = self._lib.ksched_update_node_labels(self._h, count, _ptr(idx), _ptr(lab) if lab is not None and lab.size else None, _ptr(tnt))
        self._check(rc, "ksched_update_node_labels")

    def apply_bindings_device(self, bindings, req_cpu_milli, req_mem_bytes, ok=None, flags: int = 0, status_out=None, stream=None):
        """Apply a batch's bindings to the snapshot on the device (ksched_apply_bindings_device): `available` of every node shrinks by the
        requests of the eligible pods bound to it (grows with APPLY_RELEASE).  torch CUDA tensors on this evaluator's device, all [p]:
        bindings int32, requests int64, ok uint8/bool or None (= every POST landed), status_out int32 or None.  Enqueued on `stream`
        (default: torch's current stream) behind whatever wrote `bindings` there; the host does not wait."""
        import torch
        p, *ptrs = _apply_args(self, bindings, req_cpu_milli, req_mem_bytes, ok, status_out)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = self._lib.ksched_apply_bindings_device(self._h, p, *ptrs[:4], int(flags), ptrs[4], C.c_void_p(stream.cuda_stream))
        self._check(rc, "ksched_apply_bindings_device")

    def read_nodes(self, first: int = 0, count: Optional[int] = None):
        """(cpu, mem) int64 numpy arrays: the device's current `available` columns for nodes [first, first + count), after every
        snapshot change enqueued so far (ksched_read_nodes; waits for them)."""
        if count is None:
            count = max(self.n - int(first), 0)
        cpu = np.empty((int(count),), dtype=np.int64)
        mem = np.empty((int(count),), dtype=np.int64)
        self._check(self._lib.ksched_read_nodes(self._h, int(first), int(count), _ptr(cpu), _ptr(mem)), "ksched_read_nodes")
        return cpu, mem

    # -- evaluation, host buffers ------------------------------------------------------------------
    def eval(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, samples=None, flags: int = L.FIT,
             want_mask: bool = True, out: "EvalResult | None" = None) -> EvalResult:
        """flags: predicates, at most one of PICK_SAMPLED (samples [p][attempts] node indices), PICK_BESTFIT and PICK_UNIFORM (samples [p][attempts]
        32-bit draws of which column 0 is read: uniformly among the pod's feasible nodes), WANT_FIT_MASK.
        `out`: an EvalResult of an earlier call with the same shapes whose arrays are written again instead of fresh ones -- a caller that evaluates batch
        after batch keeps its result buffers (a fresh 63 MB numpy array is first touched BY the copy: 6 ms per C3 mask instead of 1.4)."""
        cpu = _np(req_cpu_milli, np.int64, "req_cpu_milli")
        mem = _np(req_mem_bytes, np.int64, "req_mem_bytes")
        p = cpu.shape[0]
        sel = _np(sel_val_ids, np.uint32, "sel_val_ids")
        if sel is not None and sel.shape != (self.n_keys, p):
            raise ValueError(f"sel_val_ids must be [{self.n_keys}][{p}]")
        tol = _np(tolerations, np.uint64, "tolerations")
        smp = _np(samples, np.uint32, "samples")
        attempts = 0
        if flags & _DRAWS:
            if smp is None or smp.ndim != 2 or smp.shape[0] != p:
                raise ValueError("samples must be [p][attempts]")
            attempts = smp.shape[1]
        W = self.W
        res = EvalResult()

        def buf(prev, shape, dtype):
            if prev is not None and prev.shape == shape and prev.dtype == dtype and prev.flags.c_contiguous and prev.flags.writeable:
                return prev
            return np.empty(shape, dtype=dtype)
        if want_mask:
            res.feasible = buf(out.feasible if out is not None else None, (p, W), np.uint64)
        if flags & L.WANT_FIT_MASK:
            res.fit = buf(out.fit if out is not None else None, (p, W), np.uint64)
        if flags & _PICKS:
            res.binding = buf(out.binding if out is not None else None, (p,), np.int32)
        rc = self._lib.ksched_eval(self._h, p, _ptr(cpu), _ptr(mem), _ptr(sel), _ptr(tol), _ptr(smp), attempts, flags,
                                   _ptr(res.feasible), _ptr(res.fit), _ptr(res.binding))
        self._check(rc, "ksched_eval")
        return res

    # -- evaluation, device buffers (torch tensors) ----------------------------------------------
    def eval_device(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, samples=None,
                    flags: int = L.FIT, out_feasible=None, out_fit=None, out_binding=None, stream=None):
        """All arguments are torch CUDA tensors on this evaluator's device (int64 stands in for
        uint64, int32 for uint32).  Work is enqueued on `stream` (default: torch's current stream).  `samples` [p, attempts] is read with
        PICK_SAMPLED (node indices) and with PICK_UNIFORM (32-bit draws, column 0)."""
        import torch

        def dp(t, dtypes, shape=None):
            if t is None:
                return None
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or t.dtype not in dtypes:
                raise ValueError(f"expected contiguous {dtypes} CUDA tensor on cuda:{self.device}")
            if shape is not None and tuple(t.shape) != tuple(shape):
                raise ValueError(f"expected shape {shape}, got {tuple(t.shape)}")
            return C.c_void_p(t.data_ptr())

        def mask_ptr(t, pitch):
            """[p, W] view of a (possibly pitched) mask buffer: rows `pitch` words apart."""
            if t is None:
                return None, pitch
            if not t.is_cuda or t.device.index != self.device or t.dtype not in u64 or t.dim() != 2:
                raise ValueError(f"mask must be a 2-D int64/uint64 CUDA tensor on cuda:{self.device}")
            if tuple(t.shape) != (p, W) or (W and t.stride(1) != 1) or (p > 1 and t.stride(0) < W):
                raise ValueError(f"mask must be [{p}, {W}] with unit column stride, got {tuple(t.shape)} strides {t.stride()}")
            tp = int(t.stride(0)) if p > 1 else max(W, pitch or W)
            if pitch is not None and tp != pitch and p > 1:
                raise ValueError("out_feasible and out_fit must share one row pitch")
            return C.c_void_p(t.data_ptr()), tp

        p = int(req_cpu_milli.shape[0])
        W = self.W
        i64 = (torch.int64,)
        u64 = (torch.int64, torch.uint64)
        u32 = (torch.int32, torch.uint32)
        attempts = int(samples.shape[1]) if (flags & _DRAWS and samples is not None and samples.dim() == 2) else 0
        if flags & _DRAWS and (samples is None or samples.dim() != 2 or samples.shape[0] != p or attempts == 0):
            raise ValueError(f"samples must be a [{p}, attempts] tensor with KSCHED_PICK_SAMPLED / KSCHED_PICK_UNIFORM")  # a wrong shape would be an out-of-bounds device read
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        pf, pitch = mask_ptr(out_feasible, None)
        pr, pitch = mask_ptr(out_fit, pitch)
        rc = self._lib.ksched_eval_device_pitched(
            self._h, p, dp(req_cpu_milli, i64, (p,)), dp(req_mem_bytes, i64, (p,)),
            dp(sel_val_ids, u32, (self.n_keys, p)) if sel_val_ids is not None else None,
            dp(tolerations, u64, (p,)), dp(samples, u32), attempts, flags,
            pf, pr, dp(out_binding, (torch.int32,), (p,)), pitch if pitch is not None else W,
            C.c_void_p(stream.cuda_stream))
        self._check(rc, "ksched_eval_device_pitched")

    def bind_eval_device(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, samples=None, flags: int = L.FIT,
                         out_feasible=None, out_fit=None, out_bindings=(), stream=None):
        """Pre-marshal eval_device for a steady-state loop whose inputs stay in place: validates once and returns run(i, m=0)
        that enqueues the evaluation writing out_bindings[i] (and, when `out_feasible` is a LIST of equally shaped masks, the
        mask out_feasible[m]: a loop can rotate its output over several buffers).  Saves the per-call tensor checks and pointer
        conversions (tens of microseconds of Python per step)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        p, W = int(req_cpu_milli.shape[0]), self.W
        outs = list(out_bindings) or [None]
        masks = list(out_feasible) if isinstance(out_feasible, (list, tuple)) else [out_feasible]
        for t, dt in ((req_cpu_milli, (torch.int64,)), (req_mem_bytes, (torch.int64,))):
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or t.dtype not in dt or tuple(t.shape) != (p,):
                raise ValueError("bind_eval_device: request columns must be contiguous int64 [p] CUDA tensors on this device")
        if sel_val_ids is not None and (tuple(sel_val_ids.shape) != (self.n_keys, p) or not sel_val_ids.is_contiguous()):
            raise ValueError(f"sel_val_ids must be contiguous [{self.n_keys}][{p}]")
        for b in outs:
            if b is not None and (b.dtype != torch.int32 or tuple(b.shape) != (p,) or not b.is_contiguous()):
                raise ValueError("out_bindings must be contiguous int32 [p] CUDA tensors")
        pitch = None
        for m in masks + [out_fit]:
            if m is not None:
                if tuple(m.shape) != (p, W) or (W and m.stride(1) != 1):
                    raise ValueError(f"mask must be a [{p}, {W}] view with unit column stride")
                mp = int(m.stride(0)) if p > 1 else W
                if pitch is not None and mp != pitch:
                    raise ValueError("every mask of one bound evaluation must have the same row pitch")
                pitch = mp
        if pitch is None:
            pitch = W
        attempts = _attempts(samples, flags, p)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        head = (self._h, p, ptr(req_cpu_milli), ptr(req_mem_bytes), ptr(sel_val_ids), ptr(tolerations), ptr(samples), attempts, flags)
        mids = [(ptr(m), ptr(out_fit)) for m in masks]
        tails = [(ptr(b), pitch, C.c_void_p(stream.cuda_stream)) for b in outs]
        keep = (req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples, masks, out_fit, outs)
        fn, check = self._lib.ksched_eval_device_pitched, self._check
        calls = [[head + mid + tail for mid in mids] for tail in tails]  # the whole argument tuple per (binding buffer, mask buffer), built once

        def run(i: int = 0, m: int = 0, _keep=keep):
            rc = fn(*calls[i][m])
            if rc:
                check(rc, "ksched_eval_device_pitched")
        return run

    def pick_device(self, feasible, flags: int, out_binding, req_mem_bytes=None, samples=None, stream=None):
        """The pick alone (ksched_pick_device) from a [p, W] device mask written by eval_device: torch CUDA tensors,
        enqueued on `stream` (default: torch's current stream).  flags: PICK_SAMPLED (+ samples [p, attempts]),
        PICK_UNIFORM (+ samples [p, attempts]: 32-bit draws, column 0 is read) or PICK_BESTFIT (+ FIT and req_mem_bytes when the mask
        includes the resource fit)."""
        import torch
        p, W = int(feasible.shape[0]), self.W
        if not feasible.is_cuda or feasible.dim() != 2 or feasible.shape[1] != W or (W and feasible.stride(1) != 1):
            raise ValueError(f"feasible must be a [p, {W}] CUDA mask with unit column stride")
        pitch = int(feasible.stride(0)) if p > 1 else W  # a single row: any pitch >= W
        if out_binding.dtype != torch.int32 or tuple(out_binding.shape) != (p,) or not out_binding.is_contiguous():
            raise ValueError("out_binding must be a contiguous int32 [p] CUDA tensor")
        attempts = _attempts(samples, flags, p)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        rc = self._lib.ksched_pick_device(self._h, p, ptr(feasible), pitch, ptr(req_mem_bytes), ptr(samples), attempts, flags,
                                          ptr(out_binding), C.c_void_p(stream.cuda_stream))
        self._check(rc, "ksched_pick_device")

    def pick(self, feasible: np.ndarray, flags: int, req_mem_bytes=None, samples=None) -> np.ndarray:
        """The pick alone from HOST masks (ksched_pick): `feasible` = [p, W] uint64 rows as `eval` returns them (or as a caller has combined
        them: ANDed masks of a selector evaluated in key groups).  flags: PICK_SAMPLED (+ samples [p, attempts]), PICK_UNIFORM (+ samples
        [p, attempts]: 32-bit draws, column 0 is read) or PICK_BESTFIT (+ FIT and req_mem_bytes when the mask includes the resource fit)."""
        f = np.ascontiguousarray(feasible, dtype=np.uint64)
        if f.ndim != 2 or f.shape[1] != self.W:
            raise ValueError(f"feasible must be [p, {self.W}] uint64")
        p = f.shape[0]
        mem = _np(req_mem_bytes, np.int64, "req_mem_bytes")
        smp = _np(samples, np.uint32, "samples")
        attempts = 0
        if flags & _DRAWS:
            if smp is None or smp.ndim != 2 or smp.shape[0] != p:
                raise ValueError("samples must be [p][attempts]")
            attempts = smp.shape[1]
        out = np.empty((p,), dtype=np.int32)
        rc = self._lib.ksched_pick(self._h, p, _ptr(f), _ptr(mem), _ptr(smp), attempts, flags, _ptr(out))
        self._check(rc, "ksched_pick")
        return out

    def pipe(self, depth: int = 2) -> "Pipe":
        """A `depth`-slot two-stream pipeline over this evaluator (ksched_pipe_*)."""
        return Pipe(self, depth)

    def alloc_mask(self, p: int, pitched: bool = True, how=None):
        """A [p, W] int64 mask tensor on this device.  pitched=True: rows at the pitch ksched_mask_pitch(n) gives (cache-line aligned rows: the
        fast layout), the memory ALLOCATED BY THE LIBRARY (ksched_mask_alloc: the placement the measurements found fastest, profiles/r06_mask_alloc.md)
        and handed back to it when the tensor dies; `how` = one of _lib.MASK_ALLOC_* (default AUTO).  pitched=False: a packed torch tensor."""
        import torch
        W = self.W
        if not pitched:
            return torch.empty((p, max(W, 1)), dtype=torch.int64, device=f"cuda:{self.device}")[:, :W]
        ptr, pitch = C.c_void_p(), C.c_uint32(0)
        self._check(self._lib.ksched_mask_alloc(self._h, int(p), int(L.MASK_ALLOC_AUTO if how is None else how), C.byref(ptr), C.byref(pitch)), "ksched_mask_alloc")
        pitch = max(int(pitch.value), 1)
        owner = _LibraryMask(self, ptr.value, (max(int(p), 1), pitch))
        buf = torch.as_tensor(owner, device=f"cuda:{self.device}")  # zero-copy (__cuda_array_interface__); the tensor keeps `owner` alive
        return buf[:int(p), :W]

    def mask_probe_report(self) -> np.ndarray:
        """Microseconds per mask kernel launch into each candidate of this evaluator's latest probe-and-keep allocation (empty: it did not probe)."""
        out = np.zeros((16,), dtype=np.float64)
        n = self._lib.ksched_mask_probe_report(self._h, out.ctypes.data_as(C.c_void_p), 16)
        if n < 0:
            self._check(n, "ksched_mask_probe_report")
        return out[:n]

    # -- reasons -------------------------------------------------------------------------------------
    def explain(self, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, pair_pod, pair_node, flags: int) -> np.ndarray:
        """ksched_explain: REASON_* of check_node_validity for the listed (pod, node) pairs, decided on the device."""
        cpu = _np(req_cpu_milli, np.int64, "req_cpu_milli")
        mem = _np(req_mem_bytes, np.int64, "req_mem_bytes")
        p = cpu.shape[0]
        sel = _np(sel_val_ids, np.uint32, "sel_val_ids")
        if sel is not None and sel.shape != (self.n_keys, p):
            raise ValueError(f"sel_val_ids must be [{self.n_keys}][{p}]")
        tol = _np(tolerations, np.uint64, "tolerations")
        pp, pn = _np(pair_pod, np.uint32, "pair_pod"), _np(pair_node, np.uint32, "pair_node")
        if pp.ndim != 1 or pp.shape != pn.shape:
            raise ValueError("pair_pod, pair_node must be 1-D of one length")
        out = np.empty((pp.shape[0],), dtype=np.int32)
        rc = self._lib.ksched_explain(self._h, p, _ptr(cpu), _ptr(mem), _ptr(sel), _ptr(tol), pp.shape[0], _ptr(pp), _ptr(pn), flags, _ptr(out))
        self._check(rc, "ksched_explain")
        return out

    def summarize(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, flags: int = L.FIT) -> np.ndarray:
        """ksched_summarize: per pod the number of nodes check_node_validity accepts / rejects by reason, [p, SUMMARY_WORDS] uint32
        (column r = REASON_*; column 0 = feasible nodes; every row adds up to the node count)."""
        cpu = _np(req_cpu_milli, np.int64, "req_cpu_milli")
        mem = _np(req_mem_bytes, np.int64, "req_mem_bytes")
        p = cpu.shape[0]
        if cpu.ndim != 1 or mem.shape != (p,):
            raise ValueError("req_cpu_milli, req_mem_bytes must be 1-D of one length")
        sel = _np(sel_val_ids, np.uint32, "sel_val_ids")
        if sel is not None and sel.shape != (self.n_keys, p):
            raise ValueError(f"sel_val_ids must be [{self.n_keys}][{p}]")
        tol = _np(tolerations, np.uint64, "tolerations")
        if tol is not None and tol.shape != (p,):
            raise ValueError(f"tolerations must be [{p}]")
        out = np.empty((p, L.SUMMARY_WORDS), dtype=np.uint32)
        rc = self._lib.ksched_summarize(self._h, p, _ptr(cpu), _ptr(mem), _ptr(sel), _ptr(tol), int(flags), _ptr(out))
        self._check(rc, "ksched_summarize")
        return out

    def summarize_device(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, flags: int = L.FIT, out=None, stream=None):
        """ksched_summarize_device on torch CUDA tensors (int64 stands in for uint64, int32 for uint32); enqueued on `stream`
        (default: torch's current stream), the host does not wait.  `out`: a contiguous [p, SUMMARY_WORDS] int32/uint32 tensor
        (allocated when None; it need not be zeroed).  Returns it."""
        import torch

        def dp(t, dtypes, shape):
            if t is None:
                return None
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or t.dtype not in dtypes:
                raise ValueError(f"expected contiguous {dtypes} CUDA tensor on cuda:{self.device}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"expected shape {shape}, got {tuple(t.shape)}")
            return C.c_void_p(t.data_ptr())

        p = int(req_cpu_milli.shape[0])
        u64 = (torch.int64, torch.uint64)
        u32 = (torch.int32, torch.uint32)
        if out is None:
            out = torch.empty((p, L.SUMMARY_WORDS), dtype=torch.int32, device=torch.device("cuda", self.device))
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = self._lib.ksched_summarize_device(
            self._h, p, dp(req_cpu_milli, (torch.int64,), (p,)), dp(req_mem_bytes, (torch.int64,), (p,)),
            dp(sel_val_ids, u32, (self.n_keys, p)), dp(tolerations, u64, (p,)), int(flags), dp(out, u32, (p, L.SUMMARY_WORDS)),
            C.c_void_p(stream.cuda_stream))
        self._check(rc, "ksched_summarize_device")
        return out

    def reason(self, feasible_row: np.ndarray, fit_row: Optional[np.ndarray], node: int, flags: int) -> int:
        f = np.ascontiguousarray(feasible_row, dtype=np.uint64)
        r = None if fit_row is None else np.ascontiguousarray(fit_row, dtype=np.uint64)
        return self._lib.ksched_reason(_ptr(f), _ptr(r), int(node), int(flags))


class _LibraryMask:
    """Owner of one ksched_mask_alloc buffer, seen by torch through __cuda_array_interface__; ksched_mask_free when the last tensor over it dies."""

    def __init__(self, ev: "Evaluator", ptr: int, shape):
        self._ev, self._ptr = ev, ptr
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<i8", "data": (int(ptr), False), "version": 3, "strides": None}

    def __del__(self):
        ev, ptr = self._ev, self._ptr
        self._ptr = None
        if ptr and getattr(ev, "_h", None):  # (a closed evaluator has freed it already: ksched_destroy)
            try:
                ev._lib.ksched_mask_free(ev._h, C.c_void_p(ptr))
            except Exception:  # pragma: no cover
                pass


class Pipe:
    """ksched_pipe: consecutive batches software-pipelined over two internal HIP streams (mask kernel of batch i + 1
    overlaps the pick of batch i).  The caller owns the per-slot mask / binding tensors."""

    def __init__(self, ev: "Evaluator", depth: int):
        self.ev, self.depth = ev, depth
        self._lib = ev._lib
        h = C.c_void_p()
        ev._check(self._lib.ksched_pipe_create(ev._h, depth, C.byref(h)), "ksched_pipe_create")
        self._h = h

    def close(self):
        if self._h:
            self._lib.ksched_pipe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def stream(self, which: int):
        """torch view of an internal stream: 0 = mask stream, 1 = pick stream, 2 .. = further streams of the alternate mode."""
        import torch
        return torch.cuda.ExternalStream(int(self._lib.ksched_pipe_stream(self._h, which)), device=self.ev.device)

    def slot_stream(self, slot: int):
        """The stream that carried the slot's latest pick (alternate mode: its whole evaluation), or None before its first submit:
        work enqueued there is ordered behind the slot's bindings by the stream itself (ksched_pipe_slot_stream)."""
        import torch
        h = self._lib.ksched_pipe_slot_stream(self._h, slot)
        return torch.cuda.ExternalStream(int(h), device=self.ev.device) if h else None

    def slot_stream_handle(self, slot: int) -> int:
        """ksched_pipe_slot_stream as the raw hipStream_t (0 before the slot's first submit): the cheap form for a per-step check."""
        return int(self._lib.ksched_pipe_slot_stream(self._h, slot) or 0)

    def submit(self, slot: int, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples, flags: int, mask, binding):
        """torch CUDA tensors (see Evaluator.eval_device); `mask` is a [p, W] (possibly pitched) view, `binding` int32 [p].  flags carry one
        of PICK_SAMPLED, PICK_BESTFIT, PICK_UNIFORM (the uniform pick reads the mask: its slot runs in the split mode, ordered by events)."""
        p, W = int(req_cpu_milli.shape[0]), self.ev.W
        pitch = int(mask.stride(0)) if p > 1 else W
        attempts = _attempts(samples, flags, p)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        rc = self._lib.ksched_pipe_submit(self._h, slot, p, ptr(req_cpu_milli), ptr(req_mem_bytes), ptr(sel_val_ids), ptr(tolerations),
                                          ptr(samples), attempts, flags, ptr(mask), pitch, ptr(binding))
        self.ev._check(rc, "ksched_pipe_submit")

    def bind(self, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples, flags: int, masks, bindings):
        """Pre-marshal a batch whose inputs stay in place (steady-state loops): returns submit(slot) for slot-indexed `masks` /
        `bindings` lists.  Saves the per-call tensor -> pointer conversions (the host would otherwise bound the step rate)."""
        p, W = int(req_cpu_milli.shape[0]), self.ev.W
        attempts = _attempts(samples, flags, p)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        fixed = (ptr(req_cpu_milli), ptr(req_mem_bytes), ptr(sel_val_ids), ptr(tolerations), ptr(samples), attempts, flags)
        per_slot = [(ptr(m), int(m.stride(0)) if p > 1 else W, ptr(b)) for m, b in zip(masks, bindings)]
        keep = (req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples, list(masks), list(bindings))  # keep the tensors alive
        fn, h, check = self._lib.ksched_pipe_submit, self._h, self.ev._check

        def submit(slot: int, _keep=keep):
            m, pitch, b = per_slot[slot]
            rc = fn(h, slot, p, *fixed, m, pitch, b)
            if rc:
                check(rc, "ksched_pipe_submit")
        return submit

    def _wait(self, name: str, slot: int, stream, host: bool):
        import torch
        if host:
            sp = None
        else:
            sp = C.c_void_p((stream or torch.cuda.current_stream(self.ev.device)).cuda_stream or 0)
            if not sp.value:  # the legacy default stream has handle 0 = "block the host" in the C ABI: use a host wait instead
                sp = None
        self.ev._check(getattr(self._lib, name)(self._h, slot, sp), name)

    def wait(self, slot: int, stream=None, host: bool = False):
        """Order `stream` (default: torch's current stream) after the slot's pick; host=True blocks the host instead."""
        self._wait("ksched_pipe_wait", slot, stream, host)

    def wait_mask(self, slot: int, stream=None, host: bool = False):
        """The same for the slot's mask kernel (the pick does not read the mask: a finished pick says nothing about it)."""
        self._wait("ksched_pipe_wait_mask", slot, stream, host)


# ---- pure helpers on masks (numpy; no predicate logic here) -----------------------------------------
def unpack_mask(mask: np.ndarray, n_nodes: int) -> np.ndarray:
    """[P, W] uint64 -> [P, n_nodes] bool (bit node%64 of word node/64)."""
    p = mask.shape[0]
    if n_nodes == 0:
        return np.zeros((p, 0), dtype=bool)
    b = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), axis=1, bitorder="little")
    return b[:, :n_nodes].astype(bool)


def pack_mask(bits: np.ndarray) -> np.ndarray:
    """[P, N] bool -> [P, W] uint64, padding bits zero."""
    p, n = bits.shape
    W = mask_words(n)
    if W == 0:
        return np.zeros((p, 0), dtype=np.uint64)
    padded = np.zeros((p, W * 64), dtype=np.uint8)
    padded[:, :n] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(p, W)
