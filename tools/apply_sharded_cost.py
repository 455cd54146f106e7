#!/usr/bin/env python
"""Diagnostic: the device time of one ksched_apply_bindings_sharded_local call (not a bench line).

At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000, FIT | SEL | TAINT), with the bindings of one sampled
pick over the whole batch, it prints microseconds of
  (a) ksched_apply_bindings_device of the batch on one ctx (events around the call on its stream, median);
  (b) the sharded apply over a clique of `--ranks` ctxs, each applying its contiguous share of the rows (events around the call on
      rank 0's stream, median) -- with --ranks 1 and the real RCCL that is the one-rank call: (a) plus two small collectives and the merge;
  (c) the host route per batch: the bindings copied back, summed per node on the host and pushed with ksched_update_nodes;
and the bytes one rank's merge reads (nranks x n x 32).  Calls alternate between applying and releasing the batch, so the snapshot
stays near its start.  With more than one rank on one GPU (the test-only RCCL stand-in, $KSCHED_TEST_HOOKS=1 and $KSCHED_RCCL_LIB) the
ranks' work is serialised on one device and the stand-in's collective is device copies: that figure is labelled "stand-in, not a
scaling figure".
usage: python tools/apply_sharded_cost.py [--ranks 1] [--reps 200] [--configs C3,C5s] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kube_scheduler_rs_reference_amd import FIT, PICK_SAMPLED, SEL, TAINT, Evaluator, _lib, synth  # noqa: E402
from kube_scheduler_rs_reference_amd.dist import LocalClique  # noqa: E402

CONFIGS = {"C3": ("C3", None, FIT | SEL), "C5s": ("C5", 125_000, FIT | SEL | TAINT)}


def median_us(s, reps, call):
    import torch
    spans = []
    for k in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call(k)
        e1.record(s)
        e1.synchronize()
        spans.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(spans)), float(np.min(spans))


def run(name: str, ranks: int, reps: int) -> dict:
    import torch
    cfg, P, flags = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    out = {"config": name, "P": c.P, "N": c.N, "ranks": ranks, "reps": reps,
           "rccl": "stand-in" if os.environ.get("KSCHED_RCCL_LIB") else "real"}
    s = torch.cuda.current_stream()
    evs = [Evaluator(0) for _ in range(ranks)]
    one = Evaluator(0)
    try:
        for e in evs + [one]:
            e.set_nodes(**c.node_columns())
        b = torch.empty((c.P,), dtype=torch.int32, device=dev)
        one.eval_device(rc_t, rm_t, t(c.pod_sel, np.int32) if c.n_keys else None, t(c.pod_tol, np.int64) if flags & TAINT else None,
                        t(c.samples, np.int32), flags | PICK_SAMPLED, out_binding=b, stream=s)
        torch.cuda.synchronize()
        out["bound_pods"] = int((b >= 0).sum().item())
        rel = lambda k: _lib.APPLY_RELEASE if k & 1 else 0  # noqa: E731

        out["a_single_us"], out["a_single_us_min"] = median_us(s, reps, lambda k: one.apply_bindings_device(b, rc_t, rm_t, flags=rel(k), stream=s))

        cuts = [c.P * r // ranks for r in range(ranks + 1)]
        parts = [(b[cuts[r]:cuts[r + 1]], rc_t[cuts[r]:cuts[r + 1]], rm_t[cuts[r]:cuts[r + 1]]) for r in range(ranks)]
        with LocalClique(evs) as clique:
            def sharded(k):
                clique.apply_bindings([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts], cuts[:-1], flags=rel(k),
                                      streams=[s] * ranks)
            for k in range(10):  # (the first call allocates the scratch and the receive buffer)
                sharded(k)
            torch.cuda.synchronize()
            out["b_sharded_us"], out["b_sharded_us_min"] = median_us(s, reps, sharded)
        for k, e in enumerate(evs):  # every replica back where it started, like the single ctx
            cpu, mem = e.read_nodes()
            assert np.array_equal(cpu, c.avail_cpu) and np.array_equal(mem, c.avail_mem), f"rank {k} did not return to the start"
        out["merge_read_bytes_per_rank"] = ranks * c.N * 32

        host = {"cpu": c.avail_cpu.copy(), "mem": c.avail_mem.copy()}

        def host_route(k):
            bb = b.cpu().numpy()
            keep = bb >= 0
            nodes = bb[keep]
            dc = np.zeros(c.N, dtype=np.int64)
            dm = np.zeros(c.N, dtype=np.int64)
            np.add.at(dc, nodes, c.req_cpu[keep])
            np.add.at(dm, nodes, c.req_mem[keep])
            touched = np.unique(nodes).astype(np.uint32)
            sign = 1 if k & 1 else -1
            host["cpu"][touched] += sign * dc[touched]
            host["mem"][touched] += sign * dm[touched]
            one.update_nodes(touched, host["cpu"][touched], host["mem"][touched])
        out["c_host_route_us"], _ = median_us(s, max(20, reps // 10), host_route)
    finally:
        for e in evs + [one]:
            e.close()
    out["b_over_a"] = out["b_sharded_us"] / out["a_single_us"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    a.reps += a.reps & 1  # (an even count of alternating apply / release calls ends where it started)
    for name in a.configs.split(","):
        r = run(name, a.ranks, a.reps)
        label = "  (stand-in, not a scaling figure)" if r["rccl"] == "stand-in" else ""
        text = (f"{name} ({r['P']} x {r['N']}, {r['bound_pods']} pods bound), {a.ranks} rank(s), {r['rccl']} RCCL{label}: "
                f"single-ctx apply {r['a_single_us']:.1f} us, sharded apply {r['b_sharded_us']:.1f} us (min {r['b_sharded_us_min']:.1f}, "
                f"{r['b_over_a']:.2f}x), host route {r['c_host_route_us']:.0f} us; merge reads {r['merge_read_bytes_per_rank'] / 1e6:.2f} MB per rank")
        print(text, flush=True)
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n" + json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
