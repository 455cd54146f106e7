#!/usr/bin/env python
"""Diagnostic: what ksched_summarize_device costs per call, against the only whole-cluster route there was before it (not a bench line).

At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000, FIT | SEL | TAINT), device events around every call,
warmed up, the candidates ALTERNATING in one process, medians over --calls calls (default 200):
  (1) ksched_summarize_device, default path (per-tile partial words + reduce kernel);
  (1b) the same with the cross-tile combine by atomic adds (KSCHED_OPT_DEBUG bit 30): the design that was measured against (1);
  (2) the yardstick: ksched_eval_device_pitched with KSCHED_WANT_FIT_MASK writing BOTH masks into library-allocated pitched buffers
      -- device time only, i.e. without the copy-back of the two masks and the host popcount that route also needs;
  (3) the direct summary kernel (KSCHED_OPT_KERNEL direct), fewer calls: the fallback for snapshots without a bitmap index.
Requirement: (1) <= (2) at both sizes.
--yardstick-only runs (2) alone and touches no entry point newer than ksched_eval_device_pitched, and --root DIR imports the package
from another checkout: together they time the yardstick on the PARENT commit's library in the same session, to show that the route is
the code this change did not touch (the two figures must agree within the run-to-run spread: run the same command twice).
Also printed: the bytes the summary moves by shape (no mask: 8 bytes per (pod, tile) written and read back, 16 bytes per pod out).
usage: python tools/summary_cost.py [--calls 200] [--warmup 20] [--configs C3,C5s] [--yardstick-only] [--root DIR] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {"C3": ("C3", None), "C5s": ("C5", 125_000)}


def timed(torch, s, calls, warmup, bodies):
    """alternate the candidate bodies; -> {name: [us per call]} from device events around each call"""
    spans = {k: [] for k in bodies}
    events = []
    for it in range(warmup + calls):
        for name, body in bodies.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            body()
            e1.record(s)
            if it >= warmup:
                events.append((name, e0, e1))
        if it % 16 == 15:
            torch.cuda.synchronize()  # (keeps the queue short: every call is measured with the device idle behind the one before)
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        spans[name].append(e0.elapsed_time(e1) * 1e3)
    return spans


def stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "min_us": float(v.min()), "p90_us": float(np.percentile(v, 90)), "calls": int(v.size)}


def run(name: str, calls: int, warmup: int, yardstick_only: bool) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import FIT, SEL, TAINT, WANT_FIT_MASK, Evaluator, _lib, synth
    cfg, P = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    flags = FIT | SEL | (TAINT if c.n_taints else 0)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    sel_t = t(c.pod_sel, np.int32) if c.n_keys else None
    tol_t = t(c.pod_tol, np.int64) if c.n_taints else None
    tiles = (c.N + 1023) // 1024
    out = {"config": name, "P": c.P, "N": c.N, "flags": flags, "tiles": tiles, "yardstick_only": yardstick_only,
           "bytes": {"two_masks_written": 2 * c.P * ((c.N + 63) // 64) * 8, "summary_partials_written_and_read": 2 * tiles * c.P * 8,
                     "summary_table_written": c.P * 16, "pod_operands_per_tile_block": c.P * (16 + 4 * min(c.n_keys, 8) + (8 if c.n_taints else 0))}}
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        s = torch.cuda.current_stream()
        feas, fit = ev.alloc_mask(c.P), ev.alloc_mask(c.P)
        bodies = {"two_masks": lambda: ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags | WANT_FIT_MASK, out_feasible=feas, out_fit=fit, stream=s)}
        if not yardstick_only:
            counts = torch.empty((c.P, 4), dtype=torch.int32, device=dev)
            counts_b = torch.empty((c.P, 4), dtype=torch.int32, device=dev)

            def atomic():
                ev.set_option(_lib.OPT_DEBUG, 0x40000000)
                ev.summarize_device(rc_t, rm_t, sel_t, tol_t, flags=flags, out=counts_b, stream=s)
                ev.set_option(_lib.OPT_DEBUG, 0)
            bodies = {"summarize": lambda: ev.summarize_device(rc_t, rm_t, sel_t, tol_t, flags=flags, out=counts, stream=s), "summarize_atomic": atomic,
                      **bodies}
        spans = timed(torch, s, calls, warmup, bodies)
        for k, v in spans.items():
            out[k] = stats(v)
        if not yardstick_only:
            assert torch.equal(counts, counts_b), "the two cross-tile combines disagree"
            assert int(counts.sum(dim=1).min()) == c.N == int(counts.sum(dim=1).max()), "a pod's four words must add up to N"
            m = feas.cpu().numpy().view(np.uint64)
            pc = np.bitwise_count(m).sum(axis=1) if hasattr(np, "bitwise_count") else np.unpackbits(m.view(np.uint8), axis=1).sum(axis=1)
            assert np.array_equal(counts[:, 0].cpu().numpy().astype(np.int64), pc.astype(np.int64)), "word 0 != popcount of the feasible mask"
            out["summarize_over_two_masks"] = out["summarize"]["median_us"] / out["two_masks"]["median_us"]
            out["requirement_met"] = out["summarize"]["median_us"] <= out["two_masks"]["median_us"]
            if name == "C3":  # the fallback, expected to be far slower: fewer calls
                ev.set_kernel("direct")
                d = timed(torch, s, max(10, calls // 10), 2, {"summarize_direct": lambda: ev.summarize_device(rc_t, rm_t, sel_t, tol_t, flags=flags, out=counts_b, stream=s)})
                ev.set_kernel("auto")
                out["summarize_direct"] = stats(d["summarize_direct"])
                assert torch.equal(counts, counts_b), "the direct and the indexed kernel disagree"
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package (and built library) is measured")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    for name in a.configs.split(","):
        r = run(name, a.calls, a.warmup, a.yardstick_only)
        r["root"] = os.path.relpath(os.path.abspath(a.root), ROOT)
        parts = [f"{k} {r[k]['median_us']:.1f} us (min {r[k]['min_us']:.1f}, p90 {r[k]['p90_us']:.1f})"
                 for k in ("summarize", "summarize_atomic", "two_masks", "summarize_direct") if k in r]
        tail = "" if a.yardstick_only else f"  summarize / two_masks {r['summarize_over_two_masks']:.3f}  requirement (1) <= (2): {'met' if r['requirement_met'] else 'NOT MET'}"
        print(f"{name} [{r['root']}]: " + "  ".join(parts) + tail, flush=True)
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
