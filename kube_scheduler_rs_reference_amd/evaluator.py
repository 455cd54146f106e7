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
from . import _marshal as M


def mask_words(n_nodes: int) -> int:
    return (int(n_nodes) + 63) // 64


_PICKS = L.PICK_ANY  # at most one per call
_ptr = M.host_ptr


def _apply_args(ev, bindings, req_cpu, req_mem, ok, status_out):
    """(count, bindings, req_cpu, req_mem, ok, status_out) of one apply on `ev`'s device (one rank's rows of a sharded one), checked: all
    [count] contiguous CUDA tensors, bindings int32, requests int64, ok uint8/bool, status_out int32.  Pointers as ints, None for an absent
    tensor (and may be None when count is 0)."""
    if bindings is None or len(bindings.shape) != 1:
        raise ValueError("bindings must be a 1-D int32 tensor")
    p = int(bindings.shape[0])
    cols = ((bindings, "bindings", "i32"), (req_cpu, "req_cpu", "i64"), (req_mem, "req_mem", "i64"), (ok, "ok", "u8"), (status_out, "status_out", "i32"))
    return (p, *[M.device_ptr(*col, (p,), ev.device) for col in cols])


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
        """How the latest evaluation's pick ran: "fused-tile" / "fused" (inside the mask launch), "select", "bestfit-rows", "from-mask", "uniform", "spread", "pack", "none"."""
        return self._lib.ksched_last_pick(self._h).decode()

    @property
    def W(self) -> int:
        return mask_words(self.n)

    # -- snapshot --------------------------------------------------------------------------------
    def set_nodes(self, avail_cpu_milli, avail_mem_bytes, label_val_ids=None, taints=None):
        cpu = M.host_array(avail_cpu_milli, "avail_cpu_milli", "i64", (None,))
        n = cpu.shape[0]
        mem = M.host_array(avail_mem_bytes, "avail_mem_bytes", "i64", (n,))
        lab = M.host_array(label_val_ids, "label_val_ids", "u32", (None, n))
        n_keys = 0 if lab is None else lab.shape[0]
        tnt = M.host_array(taints, "taints", "u64", (n,))
        rc = self._lib.ksched_set_nodes(self._h, n, _ptr(cpu), _ptr(mem), _ptr(lab) if n_keys else None, n_keys, _ptr(tnt))
        self._check(rc, "ksched_set_nodes")
        self.n = n
        self.n_keys = n_keys

    def update_nodes(self, node_index, avail_cpu_milli, avail_mem_bytes):
        """New `available` values for the listed canonical node indices (ksched_update_nodes)."""
        idx = M.host_array(node_index, "node_index", "u32", (None,))
        cpu = M.host_array(avail_cpu_milli, "avail_cpu_milli", "i64", idx.shape)
        mem = M.host_array(avail_mem_bytes, "avail_mem_bytes", "i64", idx.shape)
        self._check(self._lib.ksched_update_nodes(self._h, idx.shape[0], _ptr(idx), _ptr(cpu), _ptr(mem)), "ksched_update_nodes")

    def update_node_labels(self, node_index, label_val_ids=None, taints=None):
        """New label ids of every key ([n_keys][count]) and, with `taints` ([count]), new taint bits for the listed canonical node
        indices (ksched_update_node_labels); `available` is not touched."""
        idx = M.host_array(node_index, "node_index", "u32", (None,))
        count = idx.shape[0]
        lab = M.host_array(label_val_ids, "label_val_ids", "u32", (self.n_keys, count))
        tnt = M.host_array(taints, "taints", "u64", (count,))
        rc = self._lib.ksched_update_node_labels(self._h, count, _ptr(idx), _ptr(lab) if lab is not None and lab.size else None, _ptr(tnt))
        self._check(rc, "ksched_update_node_labels")

    def apply_bindings_device(self, bindings, req_cpu_milli, req_mem_bytes, ok=None, flags: int = 0, status_out=None, stream=None):
        """Apply a batch's bindings to the snapshot on the device (ksched_apply_bindings_device): `available` of every node shrinks by the
        requests of the eligible pods bound to it (grows with APPLY_RELEASE).  flags: 0 accepts every eligible pod, APPLY_FIRST_PER_NODE one
        pod per node (the others DEFERRED), APPLY_WHILE_FIT per node the pods in ascending index while they still fit what is left (a pod
        that does not fit is DEFERRED and the walk goes on: no node is over-committed; not with the other two flags).  torch CUDA tensors on
        this evaluator's device, all [p]:
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
        32-bit draws of which column 0 is read: uniformly among the pod's feasible nodes) and PICK_SPREAD (samples [p][d] 32-bit draws, all read:
        the least loaded -- available memory, then cpu, then the lowest index -- of d uniformly drawn feasible nodes) and PICK_PACK
        (the same draws: the tightest -- the smallest available memory, then cpu, then the lowest index -- of them), WANT_FIT_MASK.
        `out`: an EvalResult of an earlier call with the same shapes whose arrays are written again instead of fresh ones -- a caller that evaluates batch
        after batch keeps its result buffers (a fresh 63 MB numpy array is first touched BY the copy: 6 ms per C3 mask instead of 1.4).
        The COMBINE_* flags are refused here (ValueError): masks are combined on the device, by eval_device.
        SEL with one of SELOP_EXISTS / SELOP_GT / SELOP_LT (extension E8) is an operator call, as in eval_device; SEL | SELOP_TAGGED
        (extension E9) a tagged call, as there, and with `sel_terms(T)` in the flags (extension E10) sel_val_ids is [T][n_keys][p]."""
        M.combine(flags, "Evaluator.eval", accepted=False)
        M.soft(flags, "Evaluator.eval", accepted=False)
        M.selop(flags, "Evaluator.eval", accepted=True)
        M.seltag(flags, "Evaluator.eval", accepted=True)
        M.selterms(flags, "Evaluator.eval", accepted=True)
        b = M.host_batch(self.n_keys, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples, flags)
        p, W = b.p, self.W
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
        rc = self._lib.ksched_eval(self._h, *b[:8], _ptr(res.feasible), _ptr(res.fit), _ptr(res.binding))
        self._check(rc, "ksched_eval")
        return res

    # -- evaluation, device buffers (torch tensors) ----------------------------------------------
    def eval_device(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, samples=None,
                    flags: int = L.FIT, out_feasible=None, out_fit=None, out_binding=None, stream=None):
        """All arguments are torch CUDA tensors on this evaluator's device (int64 stands in for
        uint64, int32 for uint32).  Work is enqueued on `stream` (default: torch's current stream).  `samples` [p, attempts] is read with
        PICK_SAMPLED (node indices), with PICK_UNIFORM (32-bit draws, column 0) and with PICK_SPREAD / PICK_PACK (32-bit draws, every column).
        With one of COMBINE_AND / COMBINE_OR / COMBINE_ANDNOT (extension E6) `out_feasible` is read AND written: it holds the caller's mask
        from earlier calls and becomes out_feasible & / | / & ~ feasible(this call), on the device -- words [0, W) of every row, bits at or
        beyond n of the last word zero afterwards.  A pick flag in the same call picks from the COMBINED mask (as pick_device on it with the
        pick flag alone).  Needs `out_feasible`; excludes WANT_FIT_MASK / `out_fit`.  So `zone In {a, b} and disk NotIn {hdd} and fit` is
        four calls on one mask: SEL (zone = a), SEL | COMBINE_OR (zone = b), SEL | COMBINE_ANDNOT (disk = hdd), FIT | COMBINE_AND | a pick.
        COMBINE_SOFT (extension E7) beside COMBINE_AND or COMBINE_ANDNOT makes the call a soft constraint: per pod row the mask narrows to
        out_feasible & feasible(this call) (or & ~) only where that leaves the pod a node; a row it would empty keeps what it held (bits at
        or beyond n zero either way).  A preferred affinity term is SEL | COMBINE_AND | COMBINE_SOFT on the hard mask; tiers applied most
        important first are lexicographic.
        SEL with one of SELOP_EXISTS / SELOP_GT / SELOP_LT (extension E8) is an OPERATOR call: a constrained key (entry neither 0 nor
        SEL_NEVER) passes where the node carries the key at all / carries it with an id above / below the entry, ids compared as unsigned
        32-bit numbers (ordering a numeric key's ids is the caller's interning); a node without the key fails.  No FIT, TAINT or
        WANT_FIT_MASK beside it; a COMBINE_* op (with or without COMBINE_SOFT) and a pick may be: `gpu Exists and cores Gt 16 and fit` is
        SEL | SELOP_EXISTS, then SEL | SELOP_GT | COMBINE_AND, then FIT | COMBINE_AND | a pick; DoesNotExist is SELOP_EXISTS with COMBINE_ANDNOT.
        SEL | SELOP_TAGGED (extension E9) is a TAGGED call: every entry of sel_val_ids carries its own operator, `seltag(tag, id)` =
        tag << SELTAG_SHIFT | id with tag SELTAG_EQ / _NE / _EXISTS / _ABSENT / _GT / _LT, compared against the node's whole 32-bit id (entry
        0: unconstrained; SEL_NEVER: nothing; NE and ABSENT pass a node without the key), so one call answers a whole conjunctive
        matchExpressions term per pod: `gpu Exists and cores Gt 16 and zone NotIn {z3}` is one row.  No SELOP_EXISTS / _GT / _LT, FIT, TAINT
        or WANT_FIT_MASK beside it; a COMBINE_* op (with or without COMBINE_SOFT) and a pick may be.  Interned ids must stay below 2^29.
        SEL | SELOP_TAGGED | sel_terms(T) (extension E10, 1 <= T <= MAX_TERMS) takes T tagged rows per pod, sel_val_ids [T, n_keys, p] (or
        [T * n_keys, p]), and writes the OR of the T conjunctions: a required nodeAffinity -- ORed nodeSelectorTerms, `In {a, b}` as two
        terms -- in one call and one mask.  An all-zero term passes everywhere; a term with SEL_NEVER in one key passes nowhere (the padding
        of a pod with fewer terms).  `node_affinity_rows` builds such rows from matchExpressions.  Everything else is the tagged call's."""
        calls, _ = self._marshal_eval_device((req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples), flags,
                                             [out_feasible], out_fit, [out_binding], stream)
        self._check(self._lib.ksched_eval_device_pitched(*calls[0][0]), "ksched_eval_device_pitched")

    def _marshal_eval_device(self, cols, flags, masks, out_fit, outs, stream):
        """calls[i][m] = the checked argument tuple of ksched_eval_device_pitched that writes bindings outs[i] and mask masks[m], and
        what those addresses point into."""
        import torch
        for m in masks:
            M.combine(flags, "Evaluator.eval_device", accepted=True, out_feasible=m, out_fit=out_fit)
        M.soft(flags, "Evaluator.eval_device", accepted=True)
        M.selop(flags, "Evaluator.eval_device", accepted=True, out_fit=out_fit)
        M.seltag(flags, "Evaluator.eval_device", accepted=True, out_fit=out_fit)
        M.selterms(flags, "Evaluator.eval_device", accepted=True, out_fit=out_fit)
        b = M.device_batch(self.device, self.n_keys, *cols, flags)
        (*pm, pr), pitch = M.mask_rows(b.p, self.W, self.device, *[("out_feasible", m) for m in masks], ("out_fit", out_fit))
        po = [M.device_ptr(o, "out_binding", "i32", (b.p,), self.device) for o in outs]
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        vp, st = C.c_void_p, C.c_void_p(stream.cuda_stream)
        return [[(self._h, *b[:8], vp(m), vp(pr), vp(o), pitch, st) for m in pm] for o in po], (b.keep, masks, out_fit, outs)

    def bind_eval_device(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, samples=None, flags: int = L.FIT,
                         out_feasible=None, out_fit=None, out_bindings=(), stream=None):
        """Pre-marshal eval_device for a steady-state loop whose inputs stay in place: validates once and returns run(i, m=0)
        that enqueues the evaluation writing out_bindings[i] (and, when `out_feasible` is a LIST of equally shaped masks, the
        mask out_feasible[m]: a loop can rotate its output over several buffers).  Saves the per-call tensor checks and pointer
        conversions (tens of microseconds of Python per step).  The COMBINE_* flags as in eval_device: every mask of the list is then
        one that run(i, m) reads and writes."""
        masks = list(out_feasible) if isinstance(out_feasible, (list, tuple)) else [out_feasible]
        calls, keep = self._marshal_eval_device((req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples), flags,
                                                masks, out_fit, list(out_bindings) or [None], stream)
        fn, check = self._lib.ksched_eval_device_pitched, self._check

        def run(i: int = 0, m: int = 0, _keep=keep):
            rc = fn(*calls[i][m])
            if rc:
                check(rc, "ksched_eval_device_pitched")
        return run

    def pick_device(self, feasible, flags: int, out_binding, req_mem_bytes=None, samples=None, stream=None):
        """The pick alone (ksched_pick_device) from a [p, W] device mask written by eval_device: torch CUDA tensors,
        enqueued on `stream` (default: torch's current stream).  flags: PICK_SAMPLED (+ samples [p, attempts]),
        PICK_UNIFORM (+ samples [p, attempts]: 32-bit draws, column 0 is read), PICK_SPREAD / PICK_PACK (+ samples [p, d]: 32-bit draws, all read; the nodes'
        available columns as this stream sees them at this point) or PICK_BESTFIT (+ FIT and req_mem_bytes when the mask
        includes the resource fit)."""
        import torch
        M.selop(flags, "Evaluator.pick_device", accepted=False)
        M.seltag(flags, "Evaluator.pick_device", accepted=False)
        M.selterms(flags, "Evaluator.pick_device", accepted=False)
        if feasible is None or len(feasible.shape) != 2:
            raise ValueError(f"feasible must be a [p, {self.W}] CUDA mask with unit column stride")
        b = M.device_batch(self.device, self.n_keys, None, req_mem_bytes, None, None, samples, flags, p=feasible.shape[0])
        (pf,), pitch = M.mask_rows(b.p, self.W, self.device, ("feasible", feasible))
        po = M.device_ptr(out_binding, "out_binding", "i32", (b.p,), self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = self._lib.ksched_pick_device(self._h, b.p, pf, pitch, b.mem, b.smp, b.attempts, b.flags, po, C.c_void_p(stream.cuda_stream))
        self._check(rc, "ksched_pick_device")

    def pick(self, feasible: np.ndarray, flags: int, req_mem_bytes=None, samples=None) -> np.ndarray:
        """The pick alone from HOST masks (ksched_pick): `feasible` = [p, W] uint64 rows as `eval` returns them (or as a caller has combined
        them: ANDed masks of a selector evaluated in key groups).  flags: PICK_SAMPLED (+ samples [p, attempts]), PICK_UNIFORM (+ samples
        [p, attempts]: 32-bit draws, column 0 is read), PICK_SPREAD / PICK_PACK (+ samples [p, d]: 32-bit draws, all read; no req_mem_bytes needed) or PICK_BESTFIT (+ FIT and req_mem_bytes when the mask includes the resource fit)."""
        M.selop(flags, "Evaluator.pick", accepted=False)
        M.seltag(flags, "Evaluator.pick", accepted=False)
        M.selterms(flags, "Evaluator.pick", accepted=False)
        f = M.host_array(feasible, "feasible", "u64", (None, self.W))
        b = M.host_batch(self.n_keys, None, req_mem_bytes, None, None, samples, flags, p=f.shape[0])
        out = np.empty((b.p,), dtype=np.int32)
        rc = self._lib.ksched_pick(self._h, b.p, _ptr(f), b.mem, b.smp, b.attempts, b.flags, _ptr(out))
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
        M.selop(flags, "Evaluator.explain", accepted=False)
        M.seltag(flags, "Evaluator.explain", accepted=False)
        M.selterms(flags, "Evaluator.explain", accepted=False)
        b = M.host_batch(self.n_keys, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, None, 0)
        pp = M.host_array(pair_pod, "pair_pod", "u32", (None,))
        pn = M.host_array(pair_node, "pair_node", "u32", pp.shape)
        out = np.empty(pp.shape, dtype=np.int32)
        rc = self._lib.ksched_explain(self._h, *b[:5], pp.shape[0], _ptr(pp), _ptr(pn), flags, _ptr(out))
        self._check(rc, "ksched_explain")
        return out

    def summarize(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, flags: int = L.FIT) -> np.ndarray:
        """ksched_summarize: per pod the number of nodes check_node_validity accepts / rejects by reason, [p, SUMMARY_WORDS] uint32
        (column r = REASON_*; column 0 = feasible nodes; every row adds up to the node count)."""
        M.selop(flags, "Evaluator.summarize", accepted=False)
        M.seltag(flags, "Evaluator.summarize", accepted=False)
        M.selterms(flags, "Evaluator.summarize", accepted=False)
        b = M.host_batch(self.n_keys, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, None, 0)
        out = np.empty((b.p, L.SUMMARY_WORDS), dtype=np.uint32)
        rc = self._lib.ksched_summarize(self._h, *b[:5], int(flags), _ptr(out))
        self._check(rc, "ksched_summarize")
        return out

    def summarize_device(self, req_cpu_milli, req_mem_bytes, sel_val_ids=None, tolerations=None, flags: int = L.FIT, out=None, stream=None):
        """ksched_summarize_device on torch CUDA tensors (int64 stands in for uint64, int32 for uint32); enqueued on `stream`
        (default: torch's current stream), the host does not wait.  `out`: a contiguous [p, SUMMARY_WORDS] int32/uint32 tensor
        (allocated when None; it need not be zeroed).  Returns it."""
        import torch
        M.selop(flags, "Evaluator.summarize_device", accepted=False)
        M.seltag(flags, "Evaluator.summarize_device", accepted=False)
        M.selterms(flags, "Evaluator.summarize_device", accepted=False)
        b = M.device_batch(self.device, self.n_keys, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, None, 0)
        if out is None:
            out = torch.empty((b.p, L.SUMMARY_WORDS), dtype=torch.int32, device=torch.device("cuda", self.device))
        po = M.device_ptr(out, "out", "u32", (b.p, L.SUMMARY_WORDS), self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = self._lib.ksched_summarize_device(self._h, *b[:5], int(flags), po, C.c_void_p(stream.cuda_stream))
        self._check(rc, "ksched_summarize_device")
        return out

    def reason(self, feasible_row: np.ndarray, fit_row: Optional[np.ndarray], node: int, flags: int) -> int:
        f, r = M.host_array(feasible_row, "feasible_row", "u64"), M.host_array(fit_row, "fit_row", "u64")
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

    def _marshal(self, cols, flags, masks, bindings):
        """(the batch, [(mask, pitch, binding) per slot]) as ksched_pipe_submit takes them, checked"""
        ev = self.ev
        M.combine(flags, "Pipe.submit", accepted=False)
        M.soft(flags, "Pipe.submit", accepted=False)
        M.selop(flags, "Pipe.submit", accepted=False)
        M.seltag(flags, "Pipe.submit", accepted=False)
        M.selterms(flags, "Pipe.submit", accepted=False)
        b = M.device_batch(ev.device, ev.n_keys, *cols, flags)
        per_slot = []
        for m, o in zip(masks, bindings):
            (pm,), pitch = M.mask_rows(b.p, ev.W, ev.device, ("mask", m))
            per_slot.append((C.c_void_p(pm), pitch, C.c_void_p(M.device_ptr(o, "binding", "i32", (b.p,), ev.device))))
        return b, per_slot

    def submit(self, slot: int, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples, flags: int, mask, binding):
        """torch CUDA tensors (see Evaluator.eval_device); `mask` is a [p, W] (possibly pitched) view, `binding` int32 [p].  flags carry one
        of PICK_SAMPLED, PICK_BESTFIT, PICK_UNIFORM, PICK_SPREAD, PICK_PACK (the uniform, the spread and the pack pick read the mask: their slot runs in the split mode, ordered by events).
        The COMBINE_* flags, COMBINE_SOFT included, are refused (ValueError): a slot's mask belongs to the slot; combine with Evaluator.eval_device."""
        b, per_slot = self._marshal((req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples), flags, [mask], [binding])
        self.ev._check(self._lib.ksched_pipe_submit(self._h, slot, *b[:8], *per_slot[0]), "ksched_pipe_submit")

    def bind(self, req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples, flags: int, masks, bindings):
        """Pre-marshal a batch whose inputs stay in place (steady-state loops): returns submit(slot) for slot-indexed `masks` /
        `bindings` lists.  Saves the per-call tensor -> pointer conversions (the host would otherwise bound the step rate)."""
        masks, bindings = list(masks), list(bindings)
        b, per_slot = self._marshal((req_cpu_milli, req_mem_bytes, sel_val_ids, tolerations, samples), flags, masks, bindings)
        fixed, keep = b[:8], (b.keep, masks, bindings)  # keep the tensors alive
        fn, h, check = self._lib.ksched_pipe_submit, self._h, self.ev._check

        def submit(slot: int, _keep=keep):
            rc = fn(h, slot, *fixed, *per_slot[slot])
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


# ---- tagged selector entries (extension E9; numpy, no predicate logic here) ----------------------------
def seltag(tag, ids) -> np.ndarray:
    """Tagged selector entries for a SEL | SELOP_TAGGED call: `tag << SELTAG_SHIFT | id`, elementwise over `tag` and `ids` (scalars or
    arrays, broadcast against each other), as a uint32 array of the broadcast shape.  tag: SELTAG_EQ (In {one value}), SELTAG_NE
    (NotIn {one value}: a node without the key passes), SELTAG_EXISTS, SELTAG_ABSENT (the id is not looked at), SELTAG_GT, SELTAG_LT.
    ValueError for a tag above SELTAG_LT or an id above SELTAG_ID_MASK (interned ids must stay below 2^29 in a tagged call) or below 0.
    SELTAG_EQ with id 0 IS the unconstrained entry 0: the pod does not constrain that key.  "Matches nothing" is SEL_NEVER, as ever."""
    t = np.asarray(tag)
    i = np.asarray(ids)
    if t.dtype.kind not in "iu" or i.dtype.kind not in "iu":
        raise ValueError(f"seltag: tag and ids must be integers, got {t.dtype} and {i.dtype}")
    t = t.astype(np.int64) if t.dtype != np.uint64 else t
    i = i.astype(np.int64) if i.dtype != np.uint64 else i
    if t.size and (t.min() < 0 or t.max() > L.SELTAG_LT):
        raise ValueError(f"tag: expected SELTAG_EQ ({L.SELTAG_EQ}) ... SELTAG_LT ({L.SELTAG_LT}), got {int(t.min())} ... {int(t.max())}")
    if i.size and (i.min() < 0 or i.max() > L.SELTAG_ID_MASK):
        raise ValueError(f"ids: a tagged entry holds ids 0 ... {L.SELTAG_ID_MASK:#x}, got {int(i.min())} ... {int(i.max())}")
    return ((t.astype(np.uint64) << np.uint64(L.SELTAG_SHIFT)) | i.astype(np.uint64)).astype(np.uint32)
