#!/usr/bin/env python
"""Diagnostic: what the operator kernel (KSCHED_SELOP_EXISTS / _GT / _LT, k_eval_selop) costs beside the direct kernel (not a bench line).

At C3 (100 000 pods x 5 000 nodes, 8 label keys, BASELINE's selector density), into a mask at the pitch ksched_mask_pitch(n) gives, with
KSCHED_OPT_TIMING = 1: the library brackets every mask kernel with stream events, so the figures are microseconds per LAUNCH of the kernel
alone, not per call.  Four candidates ALTERNATE in one process, warmed up, medians over --calls launches each (default 200):
  (d)  k_eval_direct on a KSCHED_SEL-only equality call (KSCHED_OPT_KERNEL = DIRECT): the yardstick -- the same label columns, the same
       selector entries, the same mask rows written;
  (e)  k_eval_selop<EXISTS>, (g) k_eval_selop<GT>, (l) k_eval_selop<LT> on KSCHED_SEL | the operator, over the same entries.
The whole measurement runs in --processes FRESH processes (default 3), one after the other; the spread of a candidate is the largest
minus the smallest of its per-process medians, and the session's spread is the yardstick's.
Expectation (reported, not gated): GT and LT do the direct kernel's compare work -- one v_cmp per constrained key and word column -- so
they should land near (d); EXISTS does scalar ANDs only and should land below.  An operator is called SLOWER when its median of medians
exceeds (d)'s by more than the session's spread.
Every candidate's mask is checked once against tests/selop_ref.py on the first 512 pods (the equality call against the oracle's rule
restated in numpy here).
Writes <out-dir>/selop_cost.txt (the lines printed) and <out-dir>/selop_cost.json (one JSON object per process).
usage: python tools/selop_cost.py [--calls 200] [--warmup 20] [--processes 3] [--out-dir profiles]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDER = ("d_direct_equality", "e_selop_exists", "g_selop_gt", "l_selop_lt")
CHECK_PODS = 512


def child(calls: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import SEL, SELOP_EXISTS, SELOP_GT, SELOP_LT, Evaluator, _lib, synth
    from tests import selop_ref
    c = synth.make_config("C3")
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t, sel_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64), t(c.pod_sel, np.int32)
    sel = np.ascontiguousarray(c.pod_sel)
    W = (c.N + 63) // 64
    out = {"config": "C3", "P": c.P, "N": c.N, "keys": c.n_keys, "W": W, "pitch_words": int(_lib.load().ksched_mask_pitch(c.N)),
           "constrained_entries_per_pod": float((sel != 0).sum() / c.P), "mask_bytes_written": c.P * W * 8}
    flags = {"d_direct_equality": SEL, "e_selop_exists": SEL | SELOP_EXISTS, "g_selop_gt": SEL | SELOP_GT, "l_selop_lt": SEL | SELOP_LT}
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        ev.set_kernel("direct")  # (the equality call's kernel; an operator call is not affected)
        s = torch.cuda.current_stream()
        masks = {k: ev.alloc_mask(c.P) for k in ORDER}
        names = {}
        # once, checked: the first CHECK_PODS rows of every candidate
        head = sel[:, :CHECK_PODS]
        eq = np.ones((CHECK_PODS, c.N), dtype=bool)
        for k in range(c.n_keys):
            e = head[k][:, None]
            eq &= (e == 0) | (e == c.node_labels[k][None, :])
        want = {"d_direct_equality": selop_ref.pack(eq), "e_selop_exists": selop_ref.selop_mask(c.node_labels, head, selop_ref.EXISTS),
                "g_selop_gt": selop_ref.selop_mask(c.node_labels, head, selop_ref.GT), "l_selop_lt": selop_ref.selop_mask(c.node_labels, head, selop_ref.LT)}
        for k in ORDER:
            ev.eval_device(rc_t, rm_t, sel_t, None, None, flags[k], out_feasible=masks[k], stream=s)
            names[k] = ev.last_kernel
            torch.cuda.synchronize()
            got = masks[k][:CHECK_PODS].contiguous().cpu().numpy().view(np.uint64)
            if not np.array_equal(got, want[k]):
                raise RuntimeError(f"{k}: the mask differs from the restatement")
        out["kernels"] = names
        spans = {k: [] for k in ORDER}
        ev.set_timing(True)
        ev.kernel_time_samples()  # (reading resets the samples)
        batch = 16
        for it0 in range(0, warmup + calls, batch):
            its = range(it0, min(it0 + batch, warmup + calls))
            for _ in its:
                for k in ORDER:
                    ev.eval_device(rc_t, rm_t, sel_t, None, None, flags[k], out_feasible=masks[k], stream=s)
            torch.cuda.synchronize()
            ms = ev.kernel_time_samples()  # in launch order: one sample per call (eight keys: one launch of either kernel)
            if len(ms) != len(its) * len(ORDER):
                raise RuntimeError(f"{len(ms)} timed launches for {len(its) * len(ORDER)} calls")
            for i, it in enumerate(its):
                if it >= warmup:
                    for j, k in enumerate(ORDER):
                        spans[k].append(float(ms[i * len(ORDER) + j]) * 1e3)
        ev.set_timing(False)
    for k in ORDER:
        v = np.asarray(spans[k])
        out[k] = {"median_us": float(np.median(v)), "min_us": float(v.min()), "p90_us": float(np.percentile(v, 90)), "launches": int(v.size)}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("SELOP_COST " + json.dumps(child(a.calls, a.warmup)), flush=True)
        return 0
    os.makedirs(a.out_dir, exist_ok=True)
    raw = []
    for i in range(a.processes):  # fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SELOP_COST ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {i} failed with status {r.returncode}")  # (nothing more is started on the device)
        raw.append(json.loads(line[-1][len("SELOP_COST "):]))
    r0 = raw[0]
    lines = [f"# tools/selop_cost.py --calls {a.calls} --warmup {a.warmup} --processes {a.processes}: us per LAUNCH of the mask kernel (KSCHED_OPT_TIMING = 1, stream events "
             "around the kernel), candidates alternating, per process the median (min, p90)",
             f"C3 ({r0['P']} x {r0['N']}, {r0['keys']} keys, {r0['constrained_entries_per_pod']:.2f} constrained entries per pod, W {r0['W']}, pitch {r0['pitch_words']} words, "
             f"{r0['mask_bytes_written'] / 1e6:.1f} MB of mask rows written per launch); kernels: {r0['kernels']}"]
    summary = {}
    for k in ORDER:
        med = [r[k]["median_us"] for r in raw]
        summary[k] = {"median_of_medians_us": float(np.median(med)), "spread_us": float(max(med) - min(med))}
        per = "; ".join(f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}, {r[k]['p90_us']:.1f})" for r in raw)
        tag, what = k.split("_", 1)
        lines.append(f"  ({tag}) {what:<16} median of medians {summary[k]['median_of_medians_us']:8.1f} us, spread over processes {summary[k]['spread_us']:.1f} us   [{per}]")
    d, spread = summary["d_direct_equality"]["median_of_medians_us"], summary["d_direct_equality"]["spread_us"]
    for k in ORDER[1:]:
        v = summary[k]["median_of_medians_us"]
        verdict = "SLOWER than the direct equality call by more than the session's spread" if v > d + spread else "within the session's spread of the direct equality call, or below it"
        lines.append(f"  {k.split('_', 1)[1]}: {v:.1f} us against (d) {d:.1f} us + spread {spread:.1f} us: {verdict}")
    print("\n".join(lines), flush=True)
    with open(os.path.join(a.out_dir, "selop_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "selop_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
