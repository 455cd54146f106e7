#!/usr/bin/env python
"""Diagnostic: what the uniform pick (KSCHED_PICK_UNIFORM, k_pick_uniform) costs per call, against a copy of the mask it reads (not a bench line).

At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000, FIT | SEL | TAINT), device events around every call,
warmed up, the candidates ALTERNATING in one process, medians over --calls calls (default 200), the mask in a library-allocated pitched buffer:
  (a) ksched_eval_device_pitched writing the mask + the uniform pick behind it;
  (b) the same call, the mask only;
  (c) ksched_pick_device, the uniform pick alone on that mask;
  (d) the yardstick: a device-to-device hipMemcpyAsync of the same mask buffer (every row at its pitch) into a second one;
  (e) for context only: the mask + the sampled pick as shipped (it rides in the mask launch where that pays).
Requirement: (c) <= (d) at both sizes -- the copy reads the bytes the pick reads and writes them as well, so the pick
gets no margin.  (c) is never compared with itself.
Writes <out-dir>/uniform_pick_cost.txt (the lines printed) and <out-dir>/uniform_pick_cost.json (one JSON object per configuration).
usage: python tools/uniform_pick_cost.py [--calls 200] [--warmup 20] [--configs C3,C5s] [--out-dir profiles]
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

HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def hip_runtime():
    """the HIP runtime this process has loaded already (torch's), by its path: hipMemcpyAsync is called on it directly"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if not paths:
        raise RuntimeError("no libamdhip64 is loaded in this process")
    hip = C.CDLL(sorted(paths)[0])
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


def run(name: str, calls: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import FIT, PICK_SAMPLED, PICK_UNIFORM, SEL, TAINT, Evaluator, synth
    cfg, P = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    flags = FIT | SEL | (TAINT if c.n_taints else 0)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    sel_t = t(c.pod_sel, np.int32) if c.n_keys else None
    tol_t = t(c.pod_tol, np.int64) if c.n_taints else None
    smp_t = t(c.samples, np.int32)  # node indices: the sampled pick's draws
    draws = np.random.default_rng(0xE3).integers(0, 1 << 32, size=(c.P, 1), dtype=np.uint64).astype(np.uint32)
    draws_t = t(draws, np.int32)
    W = (c.N + 63) // 64
    hip = hip_runtime()
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        s = torch.cuda.current_stream()
        sp = C.c_void_p(s.cuda_stream)
        mask, copy = ev.alloc_mask(c.P), ev.alloc_mask(c.P)
        pitch = int(mask.stride(0))
        nbytes = c.P * pitch * 8
        b_a = torch.full((c.P,), -7, dtype=torch.int32, device=dev)
        b_c = torch.full((c.P,), -7, dtype=torch.int32, device=dev)
        b_e = torch.full((c.P,), -7, dtype=torch.int32, device=dev)
        out = {"config": name, "P": c.P, "N": c.N, "flags": flags, "W": W, "pitch_words": pitch,
               "bytes": {"mask_rows_read_by_the_pick": c.P * W * 8, "mask_buffer_copied": nbytes, "draws_read": c.P * 4, "bindings_written": c.P * 4}}

        def copy_mask():
            rc = hip.hipMemcpyAsync(copy.data_ptr(), mask.data_ptr(), nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, sp)
            assert rc == 0, f"hipMemcpyAsync: {rc}"
        bodies = {
            "a_mask_and_uniform": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, draws_t, flags | PICK_UNIFORM, out_feasible=mask, out_binding=b_a, stream=s),
            "b_mask_only": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags, out_feasible=mask, stream=s),
            "c_uniform_alone": lambda: ev.pick_device(mask, PICK_UNIFORM, b_c, samples=draws_t, stream=s),
            "d_copy_of_the_mask": copy_mask,
            "e_mask_and_sampled": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, smp_t, flags | PICK_SAMPLED, out_feasible=mask, out_binding=b_e, stream=s),
        }
        spans = timed(torch, s, calls, warmup, bodies)
        for k, v in spans.items():
            out[k] = stats(v)
        # the candidates computed the same thing, and it is a uniform pick: a binding exactly where the row has a set bit, and that bit set
        assert torch.equal(b_a, b_c), "the pick behind the mask kernel and the pick alone disagree"
        assert torch.equal(mask, copy), "the copy is not the mask"
        got = b_c.cpu().numpy()
        m = mask.cpu().numpy().view(np.uint64)
        assert np.array_equal(got >= 0, m.any(axis=1)), "a binding must exist exactly where a node is feasible"
        rows = np.nonzero(got >= 0)[0]
        assert ((m[rows, got[rows] >> 6] >> (got[rows] & 63).astype(np.uint64)) & np.uint64(1)).all(), "a chosen node's bit must be set"
        out["bound_fraction_uniform"] = float((got >= 0).mean())
        out["bound_fraction_sampled"] = float((b_e.cpu().numpy() >= 0).mean())
        out["uniform_over_copy"] = out["c_uniform_alone"]["median_us"] / out["d_copy_of_the_mask"]["median_us"]
        out["requirement_met"] = out["c_uniform_alone"]["median_us"] <= out["d_copy_of_the_mask"]["median_us"]
        for k in ("c_uniform_alone", "d_copy_of_the_mask"):
            out[k]["GB_per_s_of_mask_read"] = (c.P * W * 8 if k[0] == "c" else nbytes) / out[k]["median_us"] * 1e-3
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    lines, raw = [f"# tools/uniform_pick_cost.py --calls {a.calls} --warmup {a.warmup} --configs {a.configs}: median us per call (min, p90), device events, candidates alternating"], []
    for name in a.configs.split(","):
        r = run(name, a.calls, a.warmup)
        raw.append(r)
        keys = ("a_mask_and_uniform", "b_mask_only", "c_uniform_alone", "d_copy_of_the_mask", "e_mask_and_sampled")
        lines.append(f"{name} ({r['P']} x {r['N']}, W {r['W']}, pitch {r['pitch_words']} words):")
        for k in keys:
            lines.append(f"  ({k[0]}) {k[2:]:<20} {r[k]['median_us']:9.1f} us  (min {r[k]['min_us']:.1f}, p90 {r[k]['p90_us']:.1f})")
        lines.append(f"  (c) reads {r['bytes']['mask_rows_read_by_the_pick'] / 1e6:.0f} MB at {r['c_uniform_alone']['GB_per_s_of_mask_read']:.0f} GB/s; "
                     f"(d) copies {r['bytes']['mask_buffer_copied'] / 1e6:.0f} MB at {r['d_copy_of_the_mask']['GB_per_s_of_mask_read']:.0f} GB/s read (+ as much written)")
        lines.append(f"  pods bound: uniform {100 * r['bound_fraction_uniform']:.1f} %, sampled {100 * r['bound_fraction_sampled']:.1f} %")
        lines.append(f"  (c) / (d) = {r['uniform_over_copy']:.3f}   requirement_met (c) <= (d): {r['requirement_met']}")
        print("\n".join(lines[-(len(keys) + 4):]), flush=True)
        print(json.dumps(r), flush=True)
    lines.append(f"requirement_met at every size: {all(r['requirement_met'] for r in raw)}")
    print(lines[-1], flush=True)
    with open(os.path.join(a.out_dir, "uniform_pick_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "uniform_pick_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
