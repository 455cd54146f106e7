#!/usr/bin/env python
"""Diagnostic: what the soft combine (KSCHED_COMBINE_SOFT, k_mask_combine_soft) costs beside the plain one (not a bench line).

At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000, FIT | SEL | TAINT): device events around every
call, warmed up, the candidates ALTERNATING in one process, medians over --calls calls (default 200).  All masks are torch buffers of
[P] rows at the pitch ksched_mask_pitch(n) gives; every kernel candidate reads the same right operand, feasible(this call).
  (y)  k_mask_combine alone, COMBINE_AND (tools/libmask_combine_bench.so enqueues the library's own launch path): the yardstick -- it moves
       the same two reads and at most the same write;
  (s)  k_mask_combine_soft alone, COMBINE_AND, every row narrowing that can (the old mask is all ones);
  (h)  the same with HALF the rows dropped (every odd row's old mask holds only nodes the evaluation removes);
  (t)  as (s) and (u) as (h), in the form that reads a row twice, which the library takes only for rows beyond 64 x kSoftKeepUnits units:
       the comparison of the two forms at rows that fit in registers;
  (b)  the whole plain combining call (COMBINE_AND) and (a) the whole soft one (COMBINE_AND | COMBINE_SOFT), on the all-ones old mask;
  (y') the yardstick again, at another place of the alternation: |y - y'| is the session's own run-to-run spread.
Aims (reported, not gated):  the kernel  (s), (h) <= max(y, y') + |y - y'|;  the call  (a) <= (b) + |y - y'|.
The results are checked on the device: after its last call every candidate's mask is the row rule restated in torch (r = old' & new; r where
it has a set bit, else old') -- the soft combine with AND changes nothing when applied again, so the mask after many calls is the mask after
one.  The shares of narrowed / dropped / empty rows are printed.
Writes <out-dir>/mask_combine_soft_cost.txt (the lines printed) and <out-dir>/mask_combine_soft_cost.json (one JSON object per configuration).
usage: python tools/mask_combine_soft_cost.py [--calls 200] [--warmup 20] [--configs C3,C5s] [--out-dir profiles]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.summary_cost import CONFIGS, stats, timed  # noqa: E402  (the same configurations, the same timing loop)

BENCH_LIB = os.path.join(ROOT, "tools", "libmask_combine_bench.so")
ORDER = ("y_and_kernel", "s_soft_kernel_all_narrow", "h_soft_kernel_half_dropped", "t_soft_read_twice_all_narrow", "u_soft_read_twice_half_dropped",
         "b_and_call", "a_soft_call", "y2_and_kernel_again")


def bench_lib():
    if not os.path.exists(BENCH_LIB):
        raise SystemExit(f"{BENCH_LIB} not found: run `make tools`")
    lib = C.CDLL(BENCH_LIB)
    lib.mcb_combine.restype = C.c_int
    lib.mcb_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.mcb_combine_soft.restype = C.c_int
    lib.mcb_combine_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    return lib


def run(name: str, calls: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import COMBINE_AND, COMBINE_SOFT, FIT, SEL, TAINT, Evaluator, _lib, synth
    bench = bench_lib()
    cfg, P = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    flags = FIT | SEL | (TAINT if c.n_taints else 0)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    sel_t = t(c.pod_sel, np.int32) if c.n_keys else None
    tol_t = t(c.pod_tol, np.int64) if c.n_taints else None
    W = (c.N + 63) // 64
    pitch = int(_lib.load().ksched_mask_pitch(c.N))
    out = {"config": name, "P": c.P, "N": c.N, "flags": flags, "W": W, "pitch_words": pitch, "mask_buffer_bytes": c.P * pitch * 8,
           "combine_bytes": 3 * c.P * W * 8}
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        s = torch.cuda.current_stream()
        st = C.c_void_p(s.cuda_stream)
        names = ("src", "and", "soft_all", "soft_half", "twice_all", "twice_half", "and_call", "soft_call")
        bufs = {k: torch.empty((c.P, pitch), dtype=torch.int64, device=dev) for k in names}
        view = lambda k: bufs[k][:, :W]  # noqa: E731
        assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
        ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags, out_feasible=view("src"), stream=s)
        torch.cuda.synchronize()
        feas = view("src")
        # the old masks: all ones (garbage at and beyond n included); and, on every odd row, only nodes the evaluation removes
        valid = torch.full((W,), -1, dtype=torch.int64, device=dev)
        if c.N % 64:
            valid[-1] = (1 << (c.N % 64)) - 1
        old_all = torch.full((c.P, W), -1, dtype=torch.int64, device=dev)
        old_half = old_all.clone()
        old_half[1::2] = ~feas[1::2]

        def restated(old):
            old_p = old & valid
            r = old_p & feas
            return torch.where((r != 0).any(dim=1, keepdim=True), r, old_p), (r != 0).any(dim=1), (old_p != 0).any(dim=1)
        want_all, narrows_all, _ = restated(old_all)
        want_half, narrows_half, nonempty_half = restated(old_half)
        out["rows"] = {"all_narrowed": float(narrows_all.float().mean()), "half_narrowed": float(narrows_half.float().mean()),
                       "half_dropped": float((~narrows_half & nonempty_half).float().mean()), "half_empty": float((~nonempty_half).float().mean())}
        for k in names[1:]:
            view(k).copy_(old_half if k.endswith("half") else old_all)
        torch.cuda.synchronize()

        def check(rc):
            if rc:
                raise RuntimeError(f"HIP error {rc}")

        def kernel(fn, k, *extra):
            return lambda: check(fn(bufs[k].data_ptr(), bufs["src"].data_ptr(), c.P, c.N, pitch, COMBINE_AND, *extra, st))
        yardstick = kernel(bench.mcb_combine, "and")
        bodies = {
            "y_and_kernel": yardstick,
            "s_soft_kernel_all_narrow": kernel(bench.mcb_combine_soft, "soft_all", 0),
            "h_soft_kernel_half_dropped": kernel(bench.mcb_combine_soft, "soft_half", 0),
            "t_soft_read_twice_all_narrow": kernel(bench.mcb_combine_soft, "twice_all", 1),
            "u_soft_read_twice_half_dropped": kernel(bench.mcb_combine_soft, "twice_half", 1),
            "b_and_call": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags | COMBINE_AND, out_feasible=view("and_call"), stream=s),
            "a_soft_call": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags | COMBINE_AND | COMBINE_SOFT, out_feasible=view("soft_call"), stream=s),
            "y2_and_kernel_again": yardstick,
        }
        assert tuple(bodies) == ORDER
        for k, v in timed(torch, s, calls, warmup, bodies).items():
            out[k] = stats(v)
        out["last_kernel"] = ev.last_kernel
        for k in ("soft_all", "twice_all", "soft_call"):
            assert torch.equal(view(k), want_all), k
        for k in ("soft_half", "twice_half"):
            assert torch.equal(view(k), want_half), k
        assert torch.equal(view("and"), feas & valid) and torch.equal(view("and_call"), feas & valid)
    y, y2, sk, hk, b, a = (out[x]["median_us"] for x in ("y_and_kernel", "y2_and_kernel_again", "s_soft_kernel_all_narrow", "h_soft_kernel_half_dropped",
                                                          "b_and_call", "a_soft_call"))
    spread = abs(y - y2)
    bound = max(y, y2) + spread
    out["aims"] = {"spread_us": spread, "kernel_bound_us": bound, "all_narrow_us": sk, "all_narrow_met": bool(sk <= bound), "half_dropped_us": hk,
                   "half_dropped_met": bool(hk <= bound), "call_bound_us": b + spread, "call_us": a, "call_met": bool(a <= b + spread)}
    out["rates_TBps"] = {"and_kernel": out["combine_bytes"] / max(y, y2) / 1e6, "soft_kernel_all_narrow": out["combine_bytes"] / sk / 1e6}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    lines, raw = [f"# tools/mask_combine_soft_cost.py --calls {a.calls} --warmup {a.warmup} --configs {a.configs}: median us (min, p90), device events, candidates alternating"], []

    def emit(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    for name in a.configs.split(","):
        r = run(name, a.calls, a.warmup)
        raw.append(r)
        q = r["rows"]
        emit(f"{name} ({r['P']} x {r['N']}, W {r['W']}, pitch {r['pitch_words']} words, mask buffer {r['mask_buffer_bytes'] / 1e6:.1f} MB, mask kernel \"{r['last_kernel']}\"):",
             f"  rows: all-ones old mask {q['all_narrowed']:.3f} narrowed; half-dropped old mask {q['half_narrowed']:.3f} narrowed, {q['half_dropped']:.3f} dropped, {q['half_empty']:.3f} empty")
        for k in ORDER:
            tag, what = k.split("_", 1)
            emit(f"  ({tag.replace('2', chr(39))}) {what:<32} {r[k]['median_us']:9.1f} us  (min {r[k]['min_us']:.1f}, p90 {r[k]['p90_us']:.1f})")
        v, rate = r["aims"], r["rates_TBps"]
        emit(f"  the kernel: (s) {v['all_narrow_us']:.1f} us, (h) {v['half_dropped_us']:.1f} us against max(y, y') + |y - y'| = {v['kernel_bound_us']:.1f} us: "
             f"{'met' if v['all_narrow_met'] else 'MISSED'}, {'met' if v['half_dropped_met'] else 'MISSED'}"
             f"  ({rate['soft_kernel_all_narrow']:.2f} TB/s against {rate['and_kernel']:.2f} TB/s over 3 x P x W x 8 B)")
        emit(f"  the call:   (a) {v['call_us']:.1f} us against (b) + |y - y'| = {v['call_bound_us']:.1f} us: {'met' if v['call_met'] else 'MISSED'}")
    with open(os.path.join(a.out_dir, "mask_combine_soft_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "mask_combine_soft_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
