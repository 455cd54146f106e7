#!/usr/bin/env python
"""Diagnostic: what the spread pick (KSCHED_PICK_SPREAD, k_pick_spread) costs per call, against the uniform pick on the same mask (not a bench line).

At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000, FIT | SEL | TAINT), device events around every call,
warmed up, the candidates ALTERNATING in one process, medians over --calls calls (default 200), the mask (written once, before the loop) in
a library-allocated pitched buffer; every candidate is ksched_pick_device on that one mask:
  (s1) (s2) (s3) (s5) the spread pick alone with d = 1, 2, 3, 5 draws per pod;
  (u) (v) the yardstick, twice: the uniform pick alone -- existing code, whose device code the spread pick's change does not alter.  The
          two are the same call at two places of the alternation: |median(u) - median(v)| is this session's own run-to-run spread;
  (m) for scale: a device-to-device hipMemcpyAsync of the same mask buffer (every row at its pitch) into a second one.
Aim: the spread pick reads the mask bytes the uniform pick reads, plus 20 d bytes per pod from cache-resident
arrays.  At the C5 shard, where the uniform pick is bandwidth-bound, (s1) .. (s5) <= max(u, v) + |u - v|.  At C3 both picks are
latency-shaped and every candidate adds a dependent select-and-gather chain: the figure is recorded.
Writes <out-dir>/spread_pick_cost.txt (the lines printed) and <out-dir>/spread_pick_cost.json (one JSON object per configuration).
usage: python tools/spread_pick_cost.py [--calls 200] [--warmup 20] [--configs C3,C5s] [--out-dir profiles]
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
from tools.uniform_pick_cost import HIP_MEMCPY_DEVICE_TO_DEVICE, hip_runtime  # noqa: E402

DS = (1, 2, 3, 5)


def run(name: str, calls: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import FIT, PICK_SPREAD, PICK_UNIFORM, SEL, TAINT, Evaluator, synth
    cfg, P = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    flags = FIT | SEL | (TAINT if c.n_taints else 0)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    sel_t = t(c.pod_sel, np.int32) if c.n_keys else None
    tol_t = t(c.pod_tol, np.int64) if c.n_taints else None
    draws = np.random.default_rng(0xE4).integers(0, 1 << 32, size=(c.P, max(DS)), dtype=np.uint64).astype(np.uint32)
    tables = {d: t(draws[:, :d], np.int32) for d in DS}
    W = (c.N + 63) // 64
    hip = hip_runtime()
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        s = torch.cuda.current_stream()
        sp = C.c_void_p(s.cuda_stream)
        mask, copy = ev.alloc_mask(c.P), ev.alloc_mask(c.P)
        pitch = int(mask.stride(0))
        nbytes = c.P * pitch * 8
        ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags, out_feasible=mask, stream=s)
        torch.cuda.synchronize()
        outs = {k: torch.full((c.P,), -7, dtype=torch.int32, device=dev) for k in [f"s{d}" for d in DS] + ["u", "v"]}
        out = {"config": name, "P": c.P, "N": c.N, "flags": flags, "W": W, "pitch_words": pitch,
               "bytes": {"mask_rows_read_by_a_pick": c.P * W * 8, "mask_buffer_copied": nbytes, "draws_and_gathered_columns_per_draw": c.P * 20,
                         "bindings_written": c.P * 4}}

        def copy_mask():
            rc = hip.hipMemcpyAsync(copy.data_ptr(), mask.data_ptr(), nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, sp)
            assert rc == 0, f"hipMemcpyAsync: {rc}"
        spread = lambda d: (lambda: ev.pick_device(mask, PICK_SPREAD, outs[f"s{d}"], samples=tables[d], stream=s))  # noqa: E731
        uniform = lambda k: (lambda: ev.pick_device(mask, PICK_UNIFORM, outs[k], samples=tables[1], stream=s))  # noqa: E731
        bodies = {"u_uniform_alone": uniform("u"), "s1_spread_d1": spread(1), "s2_spread_d2": spread(2), "s3_spread_d3": spread(3),
                  "s5_spread_d5": spread(5), "v_uniform_alone_again": uniform("v"), "m_copy_of_the_mask": copy_mask}
        spans = timed(torch, s, calls, warmup, bodies)
        for k, v in spans.items():
            out[k] = stats(v)
        # the candidates computed what they should: d = 1 is the uniform pick; every d binds exactly the pods with a feasible node, to a set bit
        assert torch.equal(outs["u"], outs["v"]) and torch.equal(outs["s1"], outs["u"]), "the spread pick with one draw is not the uniform pick"
        assert torch.equal(mask, copy), "the copy is not the mask"
        m = mask.cpu().numpy().view(np.uint64)
        some = m.any(axis=1)
        for d in DS:
            got = outs[f"s{d}"].cpu().numpy()
            assert np.array_equal(got >= 0, some), "a binding must exist exactly where a node is feasible"
            rows = np.nonzero(got >= 0)[0]
            assert ((m[rows, got[rows] >> 6] >> (got[rows] & 63).astype(np.uint64)) & np.uint64(1)).all(), "a chosen node's bit must be set"
        out["bound_fraction"] = float(some.mean())
        u, v = out["u_uniform_alone"]["median_us"], out["v_uniform_alone_again"]["median_us"]
        out["uniform_run_to_run_us"] = abs(u - v)
        out["bound_us"] = max(u, v) + abs(u - v)
        out["spread_over_uniform"] = {f"d{d}": out[f"s{d}_spread_d{d}"]["median_us"] / min(u, v) for d in DS}
        out["aim_met"] = all(out[f"s{d}_spread_d{d}"]["median_us"] <= out["bound_us"] for d in DS)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    lines, raw = [f"# tools/spread_pick_cost.py --calls {a.calls} --warmup {a.warmup} --configs {a.configs}: median us per call (min, p90), device events, candidates alternating"], []
    keys = ("u_uniform_alone", "s1_spread_d1", "s2_spread_d2", "s3_spread_d3", "s5_spread_d5", "v_uniform_alone_again", "m_copy_of_the_mask")
    for name in a.configs.split(","):
        r = run(name, a.calls, a.warmup)
        raw.append(r)
        lines.append(f"{name} ({r['P']} x {r['N']}, W {r['W']}, pitch {r['pitch_words']} words, {100 * r['bound_fraction']:.1f} % of the pods have a feasible node):")
        for k in keys:
            tag, what = k.split("_", 1)
            lines.append(f"  ({tag}) {what:<22} {r[k]['median_us']:9.1f} us  (min {r[k]['min_us']:.1f}, p90 {r[k]['p90_us']:.1f})")
        lines.append(f"  a pick reads {r['bytes']['mask_rows_read_by_a_pick'] / 1e6:.0f} MB of mask rows; every draw adds {r['bytes']['draws_and_gathered_columns_per_draw'] / 1e6:.1f} MB "
                     f"of draws and gathered columns; (m) copies {r['bytes']['mask_buffer_copied'] / 1e6:.0f} MB")
        lines.append(f"  uniform run to run |u - v| = {r['uniform_run_to_run_us']:.1f} us; bound max(u, v) + |u - v| = {r['bound_us']:.1f} us; spread / uniform: "
                     + ", ".join(f"d = {k[1:]} {v:.3f}" for k, v in r["spread_over_uniform"].items()))
        lines.append(f"  aim (every d <= the bound) met: {r['aim_met']}" + ("" if name == "C5s" else "   (recorded; the aim is set at the C5 shard)"))
        print("\n".join(lines[-(len(keys) + 4):]), flush=True)
        print(json.dumps(r), flush=True)
    with open(os.path.join(a.out_dir, "spread_pick_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "spread_pick_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
