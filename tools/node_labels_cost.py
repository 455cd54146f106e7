#!/usr/bin/env python
"""Diagnostic: what keeping the snapshot current from node watch events costs (not a bench line).

At C3 (5 000 nodes) and at the C5 shard (50 000 nodes), both with 8 label keys and 16 taints, it prints the host time (the call returns)
and the ready time (the call returns and the device has finished it: a device synchronize after it), median over --reps calls, of
  - ksched_set_nodes of the whole snapshot;
  - ksched_update_node_labels of 1 node, of 16 nodes and of one node in every 1024-node tile, with the layout kept (ids at most each key's
    largest, taint bits inside the planned groups);
  - the same with a re-plan (one id above its key's largest: the whole index is rebuilt from the columns on the device);
and the first best-fit evaluation of 20 000 pods (bindings only) after a label-only change (the rows in best-fit order rebuilt alone)
against after a ksched_update_nodes (the order sorted again as well).
usage: python tools/node_labels_cost.py [--reps 30] [--configs C3,C5s] [--out FILE.json] [--table FILE.txt]
(--out: the JSON lines as printed; --table: the same figures as the table of profiles/node_labels_cost.txt)
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

from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, SEL, TAINT, Evaluator, synth  # noqa: E402

CONFIGS = {"C3": 5_000, "C5s": 50_000}


def run(name: str, reps: int) -> dict:
    import torch
    N = CONFIGS[name]
    c = synth.make_cluster(20_000, N, n_keys=8, n_taints=16, seed=0xCAB + N)
    cols = c.node_columns()
    lab, tnt = c.node_labels, c.node_taints
    lmax = lab.max(axis=1)
    rng = np.random.default_rng(1)
    out = {"config": name, "N": N, "keys": 8, "taints": 16, "reps": reps}
    with Evaluator(0) as ev:
        ev.set_nodes(**cols)
        torch.cuda.synchronize()

        def timed(fn, before=None):
            host, ready = [], []
            for _ in range(reps):
                if before is not None:
                    before()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                host.append((t1 - t0) * 1e6)
                ready.append((t2 - t0) * 1e6)
            return {"host_us": round(float(np.median(host)), 1), "ready_us": round(float(np.median(ready)), 1)}

        out["set_nodes"] = timed(lambda: ev.set_nodes(**cols))

        def rows_for(idx, replan):
            rows = (rng.integers(0, lmax[:, None].astype(np.int64) + 1, (8, idx.size))).astype(np.uint32)
            if replan:
                rows[0, 0] = lmax[0] + 1
            t = rng.integers(0, 1 << 16, idx.size, dtype=np.uint64)
            return rows, t

        tiles = (N + 1023) // 1024
        shapes = {"1": lambda: rng.integers(0, N, 1), "16": lambda: rng.choice(N, 16, replace=False),
                  "every_tile": lambda: np.minimum(np.arange(tiles) * 1024 + rng.integers(0, 1024, tiles), N - 1)}
        for replan in (False, True):
            for sname, mk in shapes.items():
                key = f"update_node_labels_{sname}_{'replan' if replan else 'kept'}"
                state = {}

                def before():
                    if replan:  # back to the planned maxima, so that every call re-plans
                        ev.set_nodes(**cols)
                    idx = mk().astype(np.uint32)
                    state["args"] = (idx, *rows_for(idx, replan))

                out[key] = timed(lambda: ev.update_node_labels(*state["args"]), before)
        ev.set_nodes(**cols)
        pc = c.pod_columns()
        fl = FIT | SEL | TAINT | PICK_BESTFIT

        def bestfit():
            ev.eval(pc["req_cpu_milli"], pc["req_mem_bytes"], pc["sel_val_ids"], pc["tolerations"], None, fl, want_mask=False)

        bestfit()

        def after_labels():
            idx = rng.integers(0, N, 1).astype(np.uint32)
            ev.update_node_labels(idx, *rows_for(idx, False))

        def after_update_nodes():
            idx = rng.integers(0, N, 1).astype(np.uint32)
            ev.update_nodes(idx, c.avail_cpu[idx] - 1, c.avail_mem[idx])

        out["bestfit_20000_after_label_change"] = timed(bestfit, after_labels)
        out["bestfit_20000_after_update_nodes"] = timed(bestfit, after_update_nodes)
        out["bestfit_20000_steady"] = timed(bestfit)
    return out


KEYS = ["set_nodes", "update_node_labels_1_kept", "update_node_labels_16_kept", "update_node_labels_every_tile_kept",
        "update_node_labels_1_replan", "update_node_labels_16_replan", "update_node_labels_every_tile_replan",
        "bestfit_20000_after_label_change", "bestfit_20000_after_update_nodes", "bestfit_20000_steady"]


def table(rows: list) -> str:
    out = [f"# tools/node_labels_cost.py --reps {rows[0]['reps']}: median over the calls, microseconds.",
           "# host = the call returns; ready = the call returns and a device synchronize after it returns.",
           "# 8 label keys, 16 taints; 'kept' = ids within each key's planned maximum (touched tiles re-indexed),",
           "# 'replan' = one id above its key's maximum (layout planned again, whole index rebuilt from the device columns).",
           "# best fit: 20 000 pods, FIT | SEL | TAINT, bindings only, first evaluation after one change of one node.", "",
           f"{'':40s}" + "".join(f"{r['config'] + ' host':>12s}{r['config'] + ' ready':>12s}" for r in rows)]
    for k in KEYS:
        out.append(f"{k:40s}" + "".join(f"{r[k]['host_us']:12.1f}{r[k]['ready_us']:12.1f}" for r in rows))
    out.append("")
    out.append("# " + ", ".join(f"{r['config']} = {r['N']} nodes" for r in rows) + ".  One-node update against ksched_set_nodes, ready:")
    for r in rows:
        faster = r["update_node_labels_1_kept"]["ready_us"] < r["set_nodes"]["ready_us"]
        out.append(f"#   {r['config']}: {r['update_node_labels_1_kept']['ready_us']} us against {r['set_nodes']['ready_us']} us"
                   f" ({'sooner' if faster else 'NOT sooner'}).")
    return "\n".join(out) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    lines, rows = [], []
    for name in a.configs.split(","):
        r = run(name, a.reps)
        rows.append(r)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if a.table:
        with open(a.table, "w") as f:
            f.write(table(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
