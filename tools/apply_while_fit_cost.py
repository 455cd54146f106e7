#!/usr/bin/env python
"""Diagnostic: what admitting a batch's bindings in pod order while they fit (KSCHED_APPLY_WHILE_FIT) costs on the device, and what it
buys, against the one-pod-per-node rule (KSCHED_APPLY_FIRST_PER_NODE) -- not a bench line.

One process, device events around single applies on one stream, medians.  Every apply starts from the same snapshot: after a timed apply the
pods it reported APPLIED are released again (KSCHED_APPLY_RELEASE of those bindings, untimed), which restores the columns and the index bit
for bit.  Within one repetition the candidates alternate:

    FIRST_PER_NODE (place 1) -> WHILE_FIT -> FIRST_PER_NODE (place 2)

FIRST_PER_NODE is existing code: the difference between its two places is the session's own spread.  Cases:
  C3       100 000 pods x 5 000 nodes, FIT | SEL, the bindings of one sampled pick on the starting snapshot
  C5s      125 000 pods x 50 000 nodes, FIT | SEL | TAINT, likewise
  herd     C3's nodes, every pod with the same request, the bindings of one best-fit pick: pods of equal selectors share their node
           (long segments; each node takes what fits and defers the rest)
Per case: (a) microseconds per call, (b) pods admitted per call, (c) admitted pods per microsecond, for both rules.  Microseconds per KERNEL
come from a run of this script under `rocprofv3 --kernel-trace --stats` (a run of its own, fewer repetitions: tracing slows the host).
usage: python tools/apply_while_fit_cost.py [--reps 200] [--warmup 20] [--cases C3,C5s,herd] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, PICK_SAMPLED, SEL, TAINT, Evaluator, _lib, synth  # noqa: E402

CASES = {"C3": ("C3", None, FIT | SEL, False), "C5s": ("C5", 125_000, FIT | SEL | TAINT, False), "herd": ("C3", None, FIT | SEL, True)}
FPN, WF, REL = _lib.APPLY_FIRST_PER_NODE, _lib.APPLY_WHILE_FIT, _lib.APPLY_RELEASE


def run(name: str, reps: int, warmup: int) -> dict:
    import torch
    cfg, P, flags, herd = CASES[name]
    c = synth.make_config(cfg, P=P)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    req_cpu, req_mem = c.req_cpu, c.req_mem
    if herd:  # one request for everybody: the median pod's
        req_cpu = np.full_like(req_cpu, int(np.median(req_cpu)))
        req_mem = np.full_like(req_mem, int(np.median(req_mem)))
    rc_t, rm_t = t(req_cpu, np.int64), t(req_mem, np.int64)
    sel_t = t(c.pod_sel, np.int32) if c.n_keys else None
    tol_t = t(c.pod_tol, np.int64) if flags & TAINT else None
    smp_t = None if herd else t(c.samples, np.int32)
    bind = torch.empty((c.P,), dtype=torch.int32, device=dev)
    status = torch.empty((c.P,), dtype=torch.int32, device=dev)
    unbound = torch.full((c.P,), -1, dtype=torch.int32, device=dev)
    out = {"case": name, "P": c.P, "N": c.N, "pick": "bestfit" if herd else "sampled", "reps": reps}
    with Evaluator(0) as ev:
        s = torch.cuda.current_stream()
        ev.set_nodes(**c.node_columns())
        ev.eval_device(rc_t, rm_t, sel_t, tol_t, smp_t, flags | (PICK_BESTFIT if herd else PICK_SAMPLED), out_binding=bind, stream=s)
        torch.cuda.synchronize()
        start = ev.read_nodes()
        b = bind.cpu().numpy()
        out["bound_pods"] = int((b >= 0).sum())
        out["bound_nodes"] = int(len(np.unique(b[b >= 0])))
        out["longest_segment"] = int(np.bincount(b[b >= 0]).max()) if (b >= 0).any() else 0

        def one(rule):
            """one timed apply under `rule`, then the release of what it admitted -> (microseconds, admitted pods)"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            ev.apply_bindings_device(bind, rc_t, rm_t, flags=rule, status_out=status, stream=s)
            e1.record(s)
            taken = torch.where(status == _lib.APPLY_APPLIED, bind, unbound)
            ev.apply_bindings_device(taken, rc_t, rm_t, flags=REL, stream=s)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3, int((taken >= 0).sum().item())

        places = (("first_per_node_place1", FPN), ("while_fit", WF), ("first_per_node_place2", FPN))
        spans = {k: [] for k, _ in places}
        admitted = {}
        for r in range(warmup + reps):
            for k, rule in places:
                us, n = one(rule)
                if r >= warmup:
                    spans[k].append(us)
                assert admitted.setdefault(k, n) == n, f"{k}: {n} pods admitted, {admitted[k]} before: the snapshot was not restored"
        end = ev.read_nodes()
        assert np.array_equal(start[0], end[0]) and np.array_equal(start[1], end[1]), "the releases did not restore the snapshot"
        for k, _ in places:
            v = np.array(spans[k])
            out[k] = {"us_median": float(np.median(v)), "us_min": float(v.min()), "us_p90": float(np.percentile(v, 90)), "admitted": admitted[k],
                      "admitted_per_us": admitted[k] / float(np.median(v))}
    fp = 0.5 * (out["first_per_node_place1"]["us_median"] + out["first_per_node_place2"]["us_median"])
    out["spread_between_places_us"] = abs(out["first_per_node_place1"]["us_median"] - out["first_per_node_place2"]["us_median"])
    out["while_fit_over_first_per_node_time"] = out["while_fit"]["us_median"] / fp
    out["while_fit_over_first_per_node_admitted"] = out["while_fit"]["admitted"] / max(out["first_per_node_place1"]["admitted"], 1)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cases", default="C3,C5s,herd")
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    a = ap.parse_args()
    lines = []
    for name in a.cases.split(","):
        r = run(name, a.reps, a.warmup)
        f1, w, f2 = r["first_per_node_place1"], r["while_fit"], r["first_per_node_place2"]
        lines.append(f"{name}: {r['bound_pods']} pods bound to {r['bound_nodes']} nodes (longest segment {r['longest_segment']})  "
                     f"FIRST_PER_NODE {f1['us_median']:.1f} / {f2['us_median']:.1f} us (two places), {f1['admitted']} admitted, {f1['admitted_per_us']:.0f} / us  "
                     f"WHILE_FIT {w['us_median']:.1f} us (min {w['us_min']:.1f}, p90 {w['us_p90']:.1f}), {w['admitted']} admitted, {w['admitted_per_us']:.0f} / us  "
                     f"time x{r['while_fit_over_first_per_node_time']:.2f}, admitted x{r['while_fit_over_first_per_node_admitted']:.2f}")
        lines.append(json.dumps(r))
        print("\n".join(lines[-2:]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
