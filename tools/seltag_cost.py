#!/usr/bin/env python
"""Diagnostic: what the tagged kernel (KSCHED_SELOP_TAGGED, k_eval_seltag) costs beside the kernels it stands in for (not a bench line).

At C3 (100 000 pods x 5 000 nodes, 8 label keys, BASELINE's selector density), into masks at the pitch ksched_mask_pitch(n) gives, with
KSCHED_OPT_TIMING = 1: the library brackets every mask kernel with stream events, so the figures are microseconds per LAUNCH of the kernel
alone, not per call.  The candidates ALTERNATE in one process, warmed up, medians over --calls launches each (default 200):
 (a) untagged entries -- the same label columns, the same selector entries, the same mask rows written by every candidate:
  (d)  k_eval_direct on the KSCHED_SEL-only equality call (KSCHED_OPT_KERNEL = DIRECT): the yardstick;
  (t)  k_eval_seltag on KSCHED_SEL | KSCHED_SELOP_TAGGED over the same entries (untagged entries ARE tag EQ);
  (e)  k_eval_selop<EXISTS>, (g) k_eval_selop<GT>, (l) k_eval_selop<LT> over the same entries: E8's operators in the same run.
 (b) a mixed batch -- pod j's constrained entries under EQ, EXISTS, GT or LT by j % 4, a quarter of the pods each:
  (m)  ONE tagged call;
  (s)  the sequence that gives the same mask: the equality call on the EQ pods' entries, then three operator calls under
       KSCHED_COMBINE_AND, each on its own pods' entries (the other pods unconstrained).  (s) is the SUM of the four mask kernels'
       launches -- the three combine passes are not in the library's bracket, so this figure flatters the sequence -- and, beside it,
       (M) and (S) are the one call and the whole sequence between stream events of the tool's own, combine passes included.
     The two masks are compared in full and must be equal.
The whole measurement runs in --processes FRESH processes (default 3), one after the other; the spread of a candidate is the largest
minus the smallest of its per-process medians.
Reported, not gated: the ratio (t) / (d), and whether it lies above the slowest operator's; whether (m) lies below (s), and (M) below (S),
by more than the spreads.
(t) and (m) are checked once against tests/seltag_ref.py on the first 512 pods.
Writes <out-dir>/seltag_cost.txt (the lines printed) and <out-dir>/seltag_cost.json (one JSON object per process).
usage: python tools/seltag_cost.py [--calls 200] [--warmup 20] [--processes 3] [--out-dir profiles]
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

SINGLE = ("d_direct_equality", "t_seltag_untagged", "e_selop_exists", "g_selop_gt", "l_selop_lt", "m_seltag_mixed")
SEQ = ("s0_equality", "s1_exists_and", "s2_gt_and", "s3_lt_and")
ORDER = SINGLE + ("s_sequence_kernels", "M_seltag_mixed_call", "S_sequence_calls")
CHECK_PODS = 512


def child(calls: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import (COMBINE_AND, SEL, SEL_NEVER, SELOP_EXISTS, SELOP_GT, SELOP_LT, SELOP_TAGGED, SELTAG_EQ, SELTAG_EXISTS,
                                                 SELTAG_GT, SELTAG_ID_MASK, SELTAG_LT, Evaluator, _lib, seltag, synth)
    from tests import seltag_ref
    c = synth.make_config("C3")
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    sel = np.ascontiguousarray(c.pod_sel)
    if not (((sel == SEL_NEVER) | (sel <= SELTAG_ID_MASK)).all() and c.node_labels.max() <= SELTAG_ID_MASK):
        raise RuntimeError("the config's ids do not fit a tagged entry")
    plain = (sel != 0) & (sel != SEL_NEVER)
    # the mixed batch, and the four selector arrays of the sequence it replaces
    mixed = np.zeros_like(sel)
    parts = []
    for q, tag in enumerate((SELTAG_EQ, SELTAG_EXISTS, SELTAG_GT, SELTAG_LT)):
        part = np.zeros_like(sel)
        part[:, q::4] = sel[:, q::4]
        parts.append(part)
        mixed[:, q::4] = np.where(plain[:, q::4], seltag(tag, sel[:, q::4] & SELTAG_ID_MASK), sel[:, q::4])
    share = [float(plain[:, q::4].sum() / plain.sum()) for q in range(4)]
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    sel_t, mixed_t, parts_t = t(sel, np.int32), t(mixed, np.int32), [t(p_, np.int32) for p_ in parts]
    W = (c.N + 63) // 64
    out = {"config": "C3", "P": c.P, "N": c.N, "keys": c.n_keys, "W": W, "pitch_words": int(_lib.load().ksched_mask_pitch(c.N)),
           "constrained_entries_per_pod": float((sel != 0).sum() / c.P), "mask_bytes_written": c.P * W * 8,
           "mixed_share_eq_exists_gt_lt": share}
    T = SEL | SELOP_TAGGED
    calls_of = {"d_direct_equality": (sel_t, SEL), "t_seltag_untagged": (sel_t, T), "e_selop_exists": (sel_t, SEL | SELOP_EXISTS),
                "g_selop_gt": (sel_t, SEL | SELOP_GT), "l_selop_lt": (sel_t, SEL | SELOP_LT), "m_seltag_mixed": (mixed_t, T),
                "s0_equality": (parts_t[0], SEL), "s1_exists_and": (parts_t[1], SEL | SELOP_EXISTS | COMBINE_AND),
                "s2_gt_and": (parts_t[2], SEL | SELOP_GT | COMBINE_AND), "s3_lt_and": (parts_t[3], SEL | SELOP_LT | COMBINE_AND)}
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        ev.set_kernel("direct")  # (the equality calls' kernel; an operator call and a tagged call are not affected)
        s = torch.cuda.current_stream()
        masks = {k: ev.alloc_mask(c.P) for k in SINGLE}
        seq_mask = ev.alloc_mask(c.P)
        for k in SEQ:
            masks[k] = seq_mask
        names = {}

        def run(k):
            ev.eval_device(rc_t, rm_t, calls_of[k][0], None, None, calls_of[k][1], out_feasible=masks[k], stream=s)
        # once, checked: the tagged masks against the restatement on the first CHECK_PODS rows, the sequence's mask against the one call's in full
        for k in SINGLE + SEQ:
            run(k)
            names[k] = ev.last_kernel
        torch.cuda.synchronize()
        for k, entries in (("t_seltag_untagged", sel), ("m_seltag_mixed", mixed)):
            got = masks[k][:CHECK_PODS].contiguous().cpu().numpy().view(np.uint64)
            if not np.array_equal(got, seltag_ref.seltag_mask(c.node_labels, entries[:, :CHECK_PODS])):
                raise RuntimeError(f"{k}: the mask differs from the restatement")
        if not torch.equal(masks["t_seltag_untagged"], masks["d_direct_equality"]):
            raise RuntimeError("untagged entries: the tagged call's mask differs from the equality call's")
        if not torch.equal(masks["m_seltag_mixed"], seq_mask):
            raise RuntimeError("the mixed batch: the one tagged call's mask differs from the four-call sequence's")
        out["kernels"] = names
        out["masks_equal"] = True
        spans = {k: [] for k in ORDER}
        ev.set_timing(True)
        ev.kernel_time_samples()  # (reading resets the samples)
        batch = 8
        per_it = len(SINGLE) + len(SEQ) + 1 + len(SEQ)  # the alternation, then the one call and the sequence between the tool's own events
        for it0 in range(0, warmup + calls, batch):
            its = range(it0, min(it0 + batch, warmup + calls))
            events = []
            for _ in its:
                for k in SINGLE + SEQ:
                    run(k)
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record(s)
                run("m_seltag_mixed")
                e1.record(s)
                for k in SEQ:
                    run(k)
                e2.record(s)
                events.append((e0, e1, e2))
            torch.cuda.synchronize()
            ms = ev.kernel_time_samples()  # in launch order: one sample per call (eight keys: one launch of each mask kernel)
            if len(ms) != len(its) * per_it:
                raise RuntimeError(f"{len(ms)} timed launches for {len(its) * per_it} calls")
            for i, it in enumerate(its):
                if it < warmup:
                    continue
                row = [float(x) * 1e3 for x in ms[i * per_it:(i + 1) * per_it]]
                for j, k in enumerate(SINGLE):
                    spans[k].append(row[j])
                spans["s_sequence_kernels"].append(sum(row[len(SINGLE):len(SINGLE) + len(SEQ)]))
                e0, e1, e2 = events[i]
                spans["M_seltag_mixed_call"].append(e0.elapsed_time(e1) * 1e3)
                spans["S_sequence_calls"].append(e1.elapsed_time(e2) * 1e3)
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
        print("SELTAG_COST " + json.dumps(child(a.calls, a.warmup)), flush=True)
        return 0
    os.makedirs(a.out_dir, exist_ok=True)
    raw = []
    for i in range(a.processes):  # fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SELTAG_COST ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {i} failed with status {r.returncode}")  # (nothing more is started on the device)
        raw.append(json.loads(line[-1][len("SELTAG_COST "):]))
    r0 = raw[0]
    share = ", ".join(f"{x:.2f}" for x in r0["mixed_share_eq_exists_gt_lt"])
    lines = [f"# tools/seltag_cost.py --calls {a.calls} --warmup {a.warmup} --processes {a.processes}: us per LAUNCH of the mask kernel (KSCHED_OPT_TIMING = 1, stream events "
             "around the kernel), candidates alternating, per process the median (min, p90); (M), (S): us per call / per four-call sequence between the tool's own stream events",
             f"C3 ({r0['P']} x {r0['N']}, {r0['keys']} keys, {r0['constrained_entries_per_pod']:.2f} constrained entries per pod, W {r0['W']}, pitch {r0['pitch_words']} words, "
             f"{r0['mask_bytes_written'] / 1e6:.1f} MB of mask rows written per launch); the mixed batch's constrained entries under EQ, EXISTS, GT, LT: {share}; "
             f"its mask equals the sequence's: {all(r['masks_equal'] for r in raw)}; kernels: {r0['kernels']}"]
    summary = {}
    for k in ORDER:
        med = [r[k]["median_us"] for r in raw]
        summary[k] = {"median_of_medians_us": float(np.median(med)), "spread_us": float(max(med) - min(med))}
        per = "; ".join(f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}, {r[k]['p90_us']:.1f})" for r in raw)
        tag, what = k.split("_", 1)
        lines.append(f"  ({tag}) {what:<18} median of medians {summary[k]['median_of_medians_us']:8.1f} us, spread over processes {summary[k]['spread_us']:.1f} us   [{per}]")
    mm = lambda k: summary[k]["median_of_medians_us"]  # noqa: E731
    sp = lambda *ks: max(summary[k]["spread_us"] for k in ks)  # noqa: E731
    slowest = max(("e_selop_exists", "g_selop_gt", "l_selop_lt"), key=mm)
    lines.append(f"  (a) untagged entries: seltag {mm('t_seltag_untagged'):.1f} us against direct equality {mm('d_direct_equality'):.1f} us: ratio "
                 f"{mm('t_seltag_untagged') / mm('d_direct_equality'):.3f}; E8's slowest operator in this run: {slowest.split('_', 1)[1]} {mm(slowest):.1f} us, ratio "
                 f"{mm(slowest) / mm('d_direct_equality'):.3f}: the tagged kernel lies {'ABOVE' if mm('t_seltag_untagged') > mm(slowest) else 'at or below'} it")
    for one, seq, what in (("m_seltag_mixed", "s_sequence_kernels", "mask kernels alone (the sequence's three combine passes not counted)"),
                           ("M_seltag_mixed_call", "S_sequence_calls", "whole calls, combine passes included")):
        gap, spread = mm(seq) - mm(one), sp(one, seq)
        verdict = "the one call is CHEAPER by more than the spread" if gap > spread else "the one call is NOT cheaper by more than the spread"
        lines.append(f"  (b) the mixed batch, {what}: one tagged call {mm(one):.1f} us against the sequence {mm(seq):.1f} us: {mm(seq) / mm(one):.2f} times, "
                     f"gap {gap:.1f} us, spread {spread:.1f} us: {verdict}")
    print("\n".join(lines), flush=True)
    with open(os.path.join(a.out_dir, "seltag_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "seltag_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
