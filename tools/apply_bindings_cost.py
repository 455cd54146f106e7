#!/usr/bin/env python
"""Diagnostic: what closing the evaluate -> bind -> apply loop costs per step, on the device and through the host (not a bench line).

At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000, FIT | SEL | TAINT), bindings only (sampled pick, or
best-fit with --bestfit), it prints microseconds per step of
  (a) eval_device + pick alone, on one stream;
  (b) (a) + apply_bindings_device of the step's bindings on the same stream (no host wait inside the loop);
  (c) (a) + the bindings copied back, applied on the host (numpy, a host copy of `available`) and ksched_update_nodes of the touched rows
      -- the route a caller had before ksched_apply_bindings_device;
and the device time of one apply alone (events around it on the stream, median).  So that every step applies a full batch of bindings
whatever the loop has done before, steps alternate between applying the step's bindings and releasing (KSCHED_APPLY_RELEASE) those of
the step before: the snapshot stays near its starting point in every loop.
usage: python tools/apply_bindings_cost.py [--steps 200] [--warmup 20] [--configs C3,C5s] [--bestfit] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, PICK_SAMPLED, SEL, TAINT, Evaluator, _lib, synth  # noqa: E402

CONFIGS = {"C3": ("C3", None, FIT | SEL), "C5s": ("C5", 125_000, FIT | SEL | TAINT)}


def run(name: str, steps: int, warmup: int, bestfit: bool) -> dict:
    import torch
    cfg, P, flags = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    flags |= PICK_BESTFIT if bestfit else PICK_SAMPLED
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    sel_t = t(c.pod_sel, np.int32) if c.n_keys else None
    tol_t = t(c.pod_tol, np.int64) if flags & TAINT else None
    smp_t = t(c.samples, np.int32) if flags & PICK_SAMPLED else None
    binds = [torch.empty((c.P,), dtype=torch.int32, device=dev) for _ in range(2)]
    out = {"config": name, "P": c.P, "N": c.N, "pick": "bestfit" if bestfit else "sampled", "steps": steps}
    with Evaluator(0) as ev:
        s = torch.cuda.current_stream()

        def ev_step(k):
            ev.eval_device(rc_t, rm_t, sel_t, tol_t, smp_t, flags, out_binding=binds[k & 1], stream=s)

        def loop(body):
            ev.set_nodes(**c.node_columns())
            for k in range(warmup):
                body(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                body(k)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e6

        out["a_eval_us"] = loop(ev_step)

        def dev_step(k):
            ev_step(k)
            if k & 1:  # release the previous step's bindings
                ev.apply_bindings_device(binds[(k - 1) & 1], rc_t, rm_t, flags=_lib.APPLY_RELEASE, stream=s)
            else:
                ev.apply_bindings_device(binds[k & 1], rc_t, rm_t, stream=s)
        out["b_eval_apply_device_us"] = loop(dev_step)

        host = {}

        def host_step(k):
            ev_step(k)
            if k == 0 or "cpu" not in host:
                host["cpu"], host["mem"] = c.avail_cpu.copy(), c.avail_mem.copy()
            if k & 1:
                b, sign = host["prev"], 1
            else:
                b, sign = binds[k & 1].cpu().numpy(), -1  # (the copy waits for the evaluation)
                host["prev"] = b
            keep = b >= 0
            nodes = b[keep]
            dc = np.zeros(c.N, dtype=np.int64)
            dm = np.zeros(c.N, dtype=np.int64)
            np.add.at(dc, nodes, c.req_cpu[keep])
            np.add.at(dm, nodes, c.req_mem[keep])
            touched = np.unique(nodes).astype(np.uint32)
            host["cpu"][touched] += sign * dc[touched]
            host["mem"][touched] += sign * dm[touched]
            ev.update_nodes(touched, host["cpu"][touched], host["mem"][touched])
        out["c_eval_host_apply_update_us"] = loop(host_step)

        # the device time of one apply of a full batch of bindings (events around it, behind a finished evaluation)
        ev.set_nodes(**c.node_columns())
        ev_step(0)
        torch.cuda.synchronize()
        spans = []
        for k in range(max(20, min(steps, 200))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            ev.apply_bindings_device(binds[0], rc_t, rm_t, flags=_lib.APPLY_RELEASE if k & 1 else 0, stream=s)
            e1.record(s)
            e1.synchronize()
            spans.append(e0.elapsed_time(e1) * 1e3)
        out["apply_device_us_median"] = float(np.median(spans))
        out["apply_device_us_min"] = float(np.min(spans))
        out["bound_pods"] = int((binds[0] >= 0).sum().item())
    out["b_over_a"] = out["b_eval_apply_device_us"] / out["a_eval_us"]
    out["c_over_b"] = out["c_eval_host_apply_update_us"] / out["b_eval_apply_device_us"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--bestfit", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for name in a.configs.split(","):
        r = run(name, a.steps, a.warmup, a.bestfit)
        line = json.dumps(r)
        print(f"{name}: (a) eval {r['a_eval_us']:.1f} us/step  (b) + device apply {r['b_eval_apply_device_us']:.1f}  "
              f"(c) + host apply + update_nodes {r['c_eval_host_apply_update_us']:.1f}  apply alone {r['apply_device_us_median']:.1f} us "
              f"(min {r['apply_device_us_min']:.1f})  b/a {r['b_over_a']:.2f}  c/b {r['c_over_b']:.2f}", flush=True)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
