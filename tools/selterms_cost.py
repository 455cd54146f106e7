#!/usr/bin/env python
"""Diagnostic: what ONE tagged call with a term count (KSCHED_SEL_TERMS, k_eval_selterms) costs beside the sequence it replaces (not a bench line).

At C3 (100 000 pods x 5 000 nodes, 8 label keys), into masks at the pitch ksched_mask_pitch(n) gives.  The rows: term t of pod j is BASELINE's
selector row of pod (j + 7919 t) mod p, so every term has the config's selector density (a pod whose row would be all zeros -- it would
pass every node and end the OR -- constrains one key by an id some node carries).  For T in --terms (default 2, 4):
  all  -- every pod has T real terms;
  1pct -- one pod in a hundred has T real terms, the rest are all zeros in every term (no affinity).
The candidates ALTERNATE in one process, warmed up, medians over --calls rounds each (default 100):
  (one)  ONE call, KSCHED_SEL | KSCHED_SELOP_TAGGED | KSCHED_SEL_TERMS(T), over the [T][8][p] rows;
  (seq)  the sequence that gives the same mask with what existed before: a tagged call on term 0, then T - 1 tagged calls under
         KSCHED_COMBINE_OR on the other terms (existing kernels only: k_eval_seltag and k_mask_combine -- the yardstick).
Both between stream events of the tool's own (us per call / per sequence, combine passes included), and -- with KSCHED_OPT_TIMING = 1 --
the mask kernels alone as the library brackets them: one launch of k_eval_selterms against the SUM of the T launches of k_eval_seltag
(the T - 1 combine passes are not in the library's bracket, so that figure flatters the sequence).  The two masks are compared in full
and must be equal, and the one call's first 512 rows are checked against tests/selterms_ref.py.
The whole measurement runs in --processes FRESH processes (default 3), one after the other; the spread of a candidate is the largest
minus the smallest of its per-process medians.  Reported, not gated: whether the one call lies below the sequence by more than the
spreads, and whether the 1pct case costs what the all case costs.
Writes <out-dir>/selterms_cost.txt (the lines printed) and <out-dir>/selterms_cost.json (one JSON object per process).
usage: python tools/selterms_cost.py [--calls 100] [--warmup 10] [--processes 3] [--terms 2 4] [--out-dir profiles]
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

CHECK_PODS = 512
SHIFT_PODS = 7919


def rows_for(c, T: int, share: str):
    """[T][keys][p] tagged rows: see the module docstring"""
    from kube_scheduler_rs_reference_amd import SEL_NEVER, SELTAG_ID_MASK
    base = np.ascontiguousarray(c.pod_sel).copy()
    if not (((base == SEL_NEVER) | (base <= SELTAG_ID_MASK)).all() and c.node_labels.max() <= SELTAG_ID_MASK):
        raise RuntimeError("the config's ids do not fit a tagged entry")
    empty = np.nonzero(~(base != 0).any(axis=0))[0]
    base[0, empty] = c.node_labels[0, empty % c.N].clip(min=1)  # untagged: tag EQ
    sel = np.stack([np.roll(base, -SHIFT_PODS * t, axis=1) for t in range(T)])
    if share == "1pct":
        keep = np.zeros(c.P, dtype=bool)
        keep[::100] = True
        sel[:, :, ~keep] = 0
    return np.ascontiguousarray(sel)


def child(calls: int, warmup: int, terms) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import COMBINE_OR, SEL, SELOP_TAGGED, Evaluator, _lib, sel_terms, synth
    from tests import selterms_ref
    c = synth.make_config("C3")
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = t(c.req_cpu, np.int64), t(c.req_mem, np.int64)
    W = (c.N + 63) // 64
    TG = SEL | SELOP_TAGGED
    out = {"config": "C3", "P": c.P, "N": c.N, "keys": c.n_keys, "W": W, "pitch_words": int(_lib.load().ksched_mask_pitch(c.N)), "mask_bytes_written": c.P * W * 8,
           "cases": {}}
    cases = [(T, share) for T in terms for share in ("all", "1pct")]
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        s = torch.cuda.current_stream()
        one_mask, seq_mask = ev.alloc_mask(c.P), ev.alloc_mask(c.P)
        data = {}
        for T, share in cases:
            sel = rows_for(c, T, share)
            data[(T, share)] = (sel, t(sel, np.int32), [t(sel[i], np.int32) for i in range(T)])

        def run_one(T, share):
            ev.eval_device(rc_t, rm_t, data[(T, share)][1], None, None, TG | sel_terms(T), out_feasible=one_mask, stream=s)

        def run_seq(T, share):
            for i, term in enumerate(data[(T, share)][2]):
                ev.eval_device(rc_t, rm_t, term, None, None, TG | (COMBINE_OR if i else 0), out_feasible=seq_mask, stream=s)
        # once, checked: the one call against the restatement on the first CHECK_PODS rows, the sequence's mask against the one call's in full
        for T, share in cases:
            run_one(T, share)
            name_one = ev.last_kernel
            run_seq(T, share)
            name_seq = ev.last_kernel
            torch.cuda.synchronize()
            got = one_mask[:CHECK_PODS].contiguous().cpu().numpy().view(np.uint64)
            sel = data[(T, share)][0]
            if not np.array_equal(got, selterms_ref.selterms_mask(c.node_labels, sel[:, :, :CHECK_PODS])):
                raise RuntimeError(f"T = {T}, {share}: the one call's mask differs from the restatement")
            if not torch.equal(one_mask, seq_mask):
                raise RuntimeError(f"T = {T}, {share}: the one call's mask differs from the sequence's")
            full = int((one_mask[:, :W - 1] == -1).all(dim=1).sum())
            out["cases"][f"T{T}_{share}"] = {"T": T, "share": share, "kernels": [name_one, name_seq], "masks_equal": True,
                                             "constrained_entries_per_pod_and_term": float((sel != 0).sum() / (c.P * T)), "rows_with_every_node": full}
        spans = {key: {"one_call": [], "seq_calls": [], "one_kernel": [], "seq_kernels": []} for key in out["cases"]}
        ev.set_timing(True)
        ev.kernel_time_samples()  # (reading resets the samples)
        for it in range(warmup + calls):
            events = []
            for T, share in cases:  # the candidates alternate: one, sequence, the next case
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record(s)
                run_one(T, share)
                e1.record(s)
                run_seq(T, share)
                e2.record(s)
                events.append((e0, e1, e2))
            torch.cuda.synchronize()
            ms = [float(x) * 1e3 for x in ev.kernel_time_samples()]  # in launch order: one sample per mask kernel (eight keys: one launch each)
            if len(ms) != sum(1 + T for T, _ in cases):
                raise RuntimeError(f"{len(ms)} timed launches for {sum(1 + T for T, _ in cases)} calls")
            if it < warmup:
                continue
            at = 0
            for (T, share), (e0, e1, e2) in zip(cases, events):
                sp = spans[f"T{T}_{share}"]
                sp["one_kernel"].append(ms[at])
                sp["seq_kernels"].append(sum(ms[at + 1:at + 1 + T]))
                at += 1 + T
                sp["one_call"].append(e0.elapsed_time(e1) * 1e3)
                sp["seq_calls"].append(e1.elapsed_time(e2) * 1e3)
        ev.set_timing(False)
    for key, sp in spans.items():
        for what, v in sp.items():
            v = np.asarray(v)
            out["cases"][key][what] = {"median_us": float(np.median(v)), "min_us": float(v.min()), "p90_us": float(np.percentile(v, 90)), "rounds": int(v.size)}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--terms", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("SELTERMS_COST " + json.dumps(child(a.calls, a.warmup, a.terms)), flush=True)
        return 0
    os.makedirs(a.out_dir, exist_ok=True)
    raw = []
    for i in range(a.processes):  # fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup), "--terms", *map(str, a.terms)],
                           capture_output=True, text=True, timeout=420)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SELTERMS_COST ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {i} failed with status {r.returncode}")  # (nothing more is started on the device)
        raw.append(json.loads(line[-1][len("SELTERMS_COST "):]))
        print(f"process {i} done", flush=True)
    r0 = raw[0]
    lines = [f"# tools/selterms_cost.py --calls {a.calls} --warmup {a.warmup} --processes {a.processes} --terms {' '.join(map(str, a.terms))}: candidates alternating, per process the "
             "median (min, p90); call / sequence: us between the tool's own stream events, combine passes included; kernel(s): us per launch as KSCHED_OPT_TIMING brackets the "
             "mask kernels (one k_eval_selterms launch against the SUM of T k_eval_seltag launches, the T - 1 combine passes not counted)",
             f"C3 ({r0['P']} x {r0['N']}, {r0['keys']} keys, W {r0['W']}, pitch {r0['pitch_words']} words, {r0['mask_bytes_written'] / 1e6:.1f} MB of mask rows written per launch)"]
    summary = {}
    for key, c0 in r0["cases"].items():
        lines.append(f"T = {c0['T']}, {c0['share']}: {c0['constrained_entries_per_pod_and_term']:.2f} constrained entries per pod and term, {c0['rows_with_every_node']} rows with every node; "
                     f"kernels {c0['kernels']}; the one call's mask equals the sequence's: {all(r['cases'][key]['masks_equal'] for r in raw)}")
        summary[key] = {}
        for what, label in (("one_call", "(one) the one call"), ("seq_calls", "(seq) the sequence of calls"), ("one_kernel", "(one) its kernel alone"),
                            ("seq_kernels", "(seq) its mask kernels alone")):
            med = [r["cases"][key][what]["median_us"] for r in raw]
            summary[key][what] = (float(np.median(med)), float(max(med) - min(med)))
            per = "; ".join(f"{r['cases'][key][what]['median_us']:.1f} ({r['cases'][key][what]['min_us']:.1f}, {r['cases'][key][what]['p90_us']:.1f})" for r in raw)
            lines.append(f"  {label:<30} median of medians {summary[key][what][0]:8.1f} us, spread over processes {summary[key][what][1]:.1f} us   [{per}]")
        for one, seq, what in (("one_call", "seq_calls", "whole calls"), ("one_kernel", "seq_kernels", "mask kernels alone")):
            (mo, so), (ms_, ss) = summary[key][one], summary[key][seq]
            gap, spread = ms_ - mo, max(so, ss)
            verdict = "the one call is CHEAPER by more than the spread" if gap > spread else "the one call is NOT cheaper by more than the spread"
            lines.append(f"  {what}: one {mo:.1f} us against the sequence {ms_:.1f} us: ratio {ms_ / mo:.2f}, gap {gap:.1f} us, spread {spread:.1f} us: {verdict}")
    for T in a.terms:
        if f"T{T}_all" in summary and f"T{T}_1pct" in summary:
            (ma, sa), (m1, s1) = summary[f"T{T}_all"]["one_call"], summary[f"T{T}_1pct"]["one_call"]
            same = abs(ma - m1) <= max(sa, s1)
            lines.append(f"T = {T}: the one call with 1 % of the pods constrained {m1:.1f} us against {ma:.1f} us with all of them: ratio {m1 / ma:.2f}: "
                         f"{'the 1 % case COSTS WHAT the all-pods case costs (within the spread)' if same else 'the two differ by more than the spread'}")
    print("\n".join(lines), flush=True)
    with open(os.path.join(a.out_dir, "selterms_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "selterms_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
