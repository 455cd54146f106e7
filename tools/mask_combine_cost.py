#!/usr/bin/env python
"""Diagnostic: what the combine step of a combining evaluation (KSCHED_COMBINE_*, k_mask_combine) costs (not a bench line).

At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000, FIT | SEL | TAINT): device events around every
call, warmed up, the candidates ALTERNATING in one process, medians over --calls calls (default 200).  All masks are torch buffers of
[P] rows at the pitch ksched_mask_pitch(n) gives; every candidate works on the same ones.
  (m)  a device-to-device hipMemcpyAsync of the whole mask buffer: the yardstick -- one stream read, one written;
  (c)  k_mask_combine alone (COMBINE_AND; tools/libmask_combine_bench.so enqueues the library's own launch path): two streams read, one
       written;
  (e)  a plain mask-only evaluation into the mask: existing code, whose device code the flags do not alter;
  (a)  the whole combining call (COMBINE_AND): the same evaluation into the ctx's scratch mask, then the combine into the mask;
  (m') the copy again, at another place of the alternation: |m - m'| is the session's own run-to-run spread.
Aims (reported, not gated):  the kernel  (c) <= 1.5 * max(m, m') + |m - m'|  (three streams against two);
                             the call    (a) <= (e) + (c) + |m - m'|        (nothing hides, nothing is added beyond the two launches).
Also printed: the kernel's bytes (3 x P x W x 8) over its time, and (c) for the one-word path (the same buffers one word in: rows 8-byte
aligned only).  The results are checked: after its last call every candidate's mask is what tests/combine_ref.py says.
Writes <out-dir>/mask_combine_cost.txt (the lines printed) and <out-dir>/mask_combine_cost.json (one JSON object per configuration).
usage: python tools/mask_combine_cost.py [--calls 200] [--warmup 20] [--configs C3,C5s] [--out-dir profiles]
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


def bench_lib():
    if not os.path.exists(BENCH_LIB):
        raise SystemExit(f"{BENCH_LIB} not found: run `make tools`")
    lib = C.CDLL(BENCH_LIB)
    lib.mcb_combine.restype = C.c_int
    lib.mcb_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.mcb_copy.restype = C.c_int
    lib.mcb_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def run(name: str, calls: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import COMBINE_AND, FIT, SEL, TAINT, Evaluator, _lib, synth
    from tests.combine_ref import combine
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
    nbytes = c.P * pitch * 8
    out = {"config": name, "P": c.P, "N": c.N, "flags": flags, "W": W, "pitch_words": pitch, "mask_buffer_bytes": nbytes,
           "combine_bytes": 3 * c.P * W * 8, "copy_bytes": 2 * nbytes}
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        s = torch.cuda.current_stream()
        st = C.c_void_p(s.cuda_stream)
        # one more word than the buffer: the one-word path runs on the same sizes one word in
        bufs = {k: torch.empty((c.P * pitch + 2,), dtype=torch.int64, device=dev) for k in ("src", "kernel", "narrow_src", "narrow", "plain", "call", "copy")}
        body = lambda k, off=0: bufs[k][off:off + c.P * pitch].view(c.P, pitch)  # noqa: E731
        view = lambda k, off=0: body(k, off)[:, :W]  # noqa: E731
        assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
        # feasible(this call) once, as the combine's right operand; the old mask: every second node of every row
        ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags, out_feasible=view("src"), stream=s)
        ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags, out_feasible=view("narrow_src", 1), stream=s)
        old = 0x5555555555555555
        for k in ("kernel", "narrow", "call"):
            bufs[k].fill_(old)
        torch.cuda.synchronize()
        feas = view("src").cpu().numpy().view(np.uint64)
        assert np.array_equal(feas, view("narrow_src", 1).cpu().numpy().view(np.uint64))

        def check(rc):
            if rc:
                raise RuntimeError(f"HIP error {rc}")

        def copy():
            check(bench.mcb_copy(bufs["copy"].data_ptr(), bufs["src"].data_ptr(), nbytes, st))

        bodies = {
            "m_copy_d2d": copy,
            "c_combine_kernel": lambda: check(bench.mcb_combine(body("kernel").data_ptr(), body("src").data_ptr(), c.P, c.N, pitch, COMBINE_AND, st)),
            "e_plain_eval": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags, out_feasible=view("plain"), stream=s),
            "a_combining_call": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags | COMBINE_AND, out_feasible=view("call"), stream=s),
            "n_combine_kernel_one_word_path": lambda: check(bench.mcb_combine(body("narrow", 1).data_ptr(), body("narrow_src", 1).data_ptr(), c.P, c.N, pitch, COMBINE_AND, st)),
            "m2_copy_d2d_again": copy,
        }
        for k, v in timed(torch, s, calls, warmup, bodies).items():
            out[k] = stats(v)
        out["last_kernel"] = ev.last_kernel
        # every candidate computed what it should (AND is idempotent: the mask after many calls is the mask after one)
        want = combine(np.full((c.P, W), old, dtype=np.uint64), feas, COMBINE_AND, c.N)
        for k, off in (("kernel", 0), ("call", 0), ("narrow", 1)):
            assert np.array_equal(view(k, off).cpu().numpy().view(np.uint64), want), k
        assert np.array_equal(view("plain").cpu().numpy().view(np.uint64), feas)
        assert torch.equal(body("copy"), body("src"))
    m, m2, k, e, a = (out[x]["median_us"] for x in ("m_copy_d2d", "m2_copy_d2d_again", "c_combine_kernel", "e_plain_eval", "a_combining_call"))
    spread = abs(m - m2)
    out["aims"] = {"spread_us": spread, "kernel_bound_us": 1.5 * max(m, m2) + spread, "kernel_us": k, "kernel_met": bool(k <= 1.5 * max(m, m2) + spread),
                   "call_bound_us": e + k + spread, "call_us": a, "call_met": bool(a <= e + k + spread)}
    out["rates_TBps"] = {"combine_kernel": out["combine_bytes"] / k / 1e6, "copy_d2d": out["copy_bytes"] / max(m, m2) / 1e6,
                         "combine_kernel_one_word_path": out["combine_bytes"] / out["n_combine_kernel_one_word_path"]["median_us"] / 1e6}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    lines, raw = [f"# tools/mask_combine_cost.py --calls {a.calls} --warmup {a.warmup} --configs {a.configs}: median us (min, p90), device events, candidates alternating"], []

    def emit(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    for name in a.configs.split(","):
        r = run(name, a.calls, a.warmup)
        raw.append(r)
        emit(f"{name} ({r['P']} x {r['N']}, W {r['W']}, pitch {r['pitch_words']} words, mask buffer {r['mask_buffer_bytes'] / 1e6:.1f} MB, mask kernel \"{r['last_kernel']}\"):")
        for k in ("m_copy_d2d", "c_combine_kernel", "e_plain_eval", "a_combining_call", "n_combine_kernel_one_word_path", "m2_copy_d2d_again"):
            tag, what = k.split("_", 1)
            emit(f"  ({tag.replace('2', chr(39))}) {what:<30} {r[k]['median_us']:9.1f} us  (min {r[k]['min_us']:.1f}, p90 {r[k]['p90_us']:.1f})")
        v, q = r["aims"], r["rates_TBps"]
        emit(f"  the kernel: (c) {v['kernel_us']:.1f} us against 1.5 x max(m, m') + |m - m'| = {v['kernel_bound_us']:.1f} us: {'met' if v['kernel_met'] else 'MISSED'}"
             f"  ({q['combine_kernel']:.2f} TB/s over 3 x P x W x 8 B; the copy {q['copy_d2d']:.2f} TB/s over 2 x the buffer; the one-word path {q['combine_kernel_one_word_path']:.2f} TB/s)")
        emit(f"  the call:   (a) {v['call_us']:.1f} us against (e) + (c) + |m - m'| = {v['call_bound_us']:.1f} us: {'met' if v['call_met'] else 'MISSED'}")
    with open(os.path.join(a.out_dir, "mask_combine_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "mask_combine_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
