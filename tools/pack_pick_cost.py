#!/usr/bin/env python
"""Diagnostic: what the pack pick (KSCHED_PICK_PACK, k_pick_pack) costs, and what it buys in the live loop (not a bench line).

1. k_pick_pack against k_pick_spread.  At C3 (100 000 pods x 5 000 nodes, FIT | SEL) and at the C5 shard (125 000 x 50 000,
   FIT | SEL | TAINT), d = 2 and d = 5: device events around every call, warmed up, the candidates ALTERNATING in one process, medians
   over --calls calls (default 200); every candidate is ksched_pick_device on one mask (written once, before the loop, into a
   library-allocated pitched buffer).  The spread pick -- existing code, whose device code this flag's change does not alter -- is timed
   at two places of the alternation, (a) and (b): |median(a) - median(b)| is the session's own run-to-run spread for that d.  The two
   kernels read the same bytes, so the expectation is parity: the pack pick's median inside [min(a, b) - |a - b|, max(a, b) + |a - b|].
2. The live loop at the C5 shard: one step = [evaluate + pick (bindings only), ksched_apply_bindings_device(APPLY_WHILE_FIT)], timed with
   device events around the two calls (and one between them: the evaluation's share); what the apply admitted is released again outside the timed span, so every step's evaluation
   follows a snapshot change.  KSCHED_PICK_BESTFIT (whose order every change makes stale) against KSCHED_PICK_PACK with d = 5,
   alternating, medians over --steps steps (default 50).
3. The herd: C3's nodes, every pod with the same request (tools/apply_while_fit_cost.py's "herd" inputs), one evaluation + one
   APPLY_WHILE_FIT under best fit and under the pack pick with d = 2 and d = 5: bound pods, distinct nodes, the most pods on one node,
   pods admitted.
Writes <out-dir>/pack_pick_cost.txt (the lines printed) and <out-dir>/pack_pick_cost.json (one JSON object per part and configuration).
usage: python tools/pack_pick_cost.py [--calls 200] [--warmup 20] [--steps 50] [--configs C3,C5s] [--out-dir profiles]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.summary_cost import CONFIGS, stats, timed  # noqa: E402  (the same configurations, the same timing loop)

DS = (2, 5)


def device_columns(torch, c, req_cpu=None, req_mem=None):
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    return (t(c.req_cpu if req_cpu is None else req_cpu, np.int64), t(c.req_mem if req_mem is None else req_mem, np.int64),
            t(c.pod_sel, np.int32) if c.n_keys else None, t(c.pod_tol, np.int64) if c.n_taints else None), t


def kernels(name: str, calls: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import FIT, PICK_PACK, PICK_SPREAD, SEL, TAINT, Evaluator, synth
    cfg, P = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    flags = FIT | SEL | (TAINT if c.n_taints else 0)
    (rc_t, rm_t, sel_t, tol_t), t = device_columns(torch, c)
    draws = np.random.default_rng(0xE5).integers(0, 1 << 32, size=(c.P, max(DS)), dtype=np.uint64).astype(np.uint32)
    tables = {d: t(draws[:, :d], np.int32) for d in DS}
    W = (c.N + 63) // 64
    with Evaluator(0) as ev:
        ev.set_nodes(**c.node_columns())
        s = torch.cuda.current_stream()
        mask = ev.alloc_mask(c.P)
        ev.eval_device(rc_t, rm_t, sel_t, tol_t, None, flags, out_feasible=mask, stream=s)
        torch.cuda.synchronize()
        keys = [f"{k}{d}" for d in DS for k in ("a", "p", "b")]
        outs = {k: torch.full((c.P,), -7, dtype=torch.int32, device=torch.device("cuda:0")) for k in keys}
        pick = lambda flag, d, k: (lambda: ev.pick_device(mask, flag, outs[k], samples=tables[d], stream=s))  # noqa: E731
        bodies = {}
        for d in DS:
            bodies[f"a{d}_spread_d{d}"] = pick(PICK_SPREAD, d, f"a{d}")
            bodies[f"p{d}_pack_d{d}"] = pick(PICK_PACK, d, f"p{d}")
        for d in DS:
            bodies[f"b{d}_spread_d{d}_again"] = pick(PICK_SPREAD, d, f"b{d}")
        out = {"part": "kernels", "config": name, "P": c.P, "N": c.N, "flags": flags, "W": W, "pitch_words": int(mask.stride(0))}
        for k, v in timed(torch, s, calls, warmup, bodies).items():
            out[k] = stats(v)
        # the candidates computed what they should: the same pods bound by either pick, each to a set bit of its row; the pack pick's node
        # never has more (memory, cpu) than the spread pick's (both choose among the same candidates)
        m = mask.cpu().numpy().view(np.uint64)
        some = m.any(axis=1)
        mem, cpu = c.avail_mem, c.avail_cpu
        for d in DS:
            assert torch.equal(outs[f"a{d}"], outs[f"b{d}"])
            sp, pk = outs[f"a{d}"].cpu().numpy(), outs[f"p{d}"].cpu().numpy()
            assert np.array_equal(pk >= 0, some) and np.array_equal(sp >= 0, some), "a binding must exist exactly where a node is feasible"
            rows = np.nonzero(some)[0]
            assert ((m[rows, pk[rows] >> 6] >> (pk[rows] & 63).astype(np.uint64)) & np.uint64(1)).all(), "a chosen node's bit must be set"
            a, b = pk[rows], sp[rows]
            assert ((mem[a] < mem[b]) | ((mem[a] == mem[b]) & (cpu[a] <= cpu[b]))).all(), "the pack pick's node is no tighter than the spread pick's"
            out[f"d{d}_pods_bound_to_different_nodes"] = float((a != b).mean())
        out["inside"] = {}
        for d in DS:
            a, b, pk = out[f"a{d}_spread_d{d}"]["median_us"], out[f"b{d}_spread_d{d}_again"]["median_us"], out[f"p{d}_pack_d{d}"]["median_us"]
            out["inside"][f"d{d}"] = {"spread_a_us": a, "spread_b_us": b, "pack_us": pk, "low_us": min(a, b) - abs(a - b), "high_us": max(a, b) + abs(a - b),
                                      "pack_inside": bool(min(a, b) - abs(a - b) <= pk <= max(a, b) + abs(a - b)), "pack_over_spread": pk / (0.5 * (a + b))}
    return out


def live_loop(name: str, steps: int, warmup: int) -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, PICK_PACK, SEL, TAINT, Evaluator, _lib, synth
    cfg, P = CONFIGS[name]
    c = synth.make_config(cfg, P=P)
    flags = FIT | SEL | (TAINT if c.n_taints else 0)
    (rc_t, rm_t, sel_t, tol_t), t = device_columns(torch, c)
    smp = t(np.random.default_rng(0xE55).integers(0, 1 << 32, size=(c.P, 5), dtype=np.uint64).astype(np.uint32), np.int32)
    dev = torch.device("cuda:0")
    bind, status = torch.empty((c.P,), dtype=torch.int32, device=dev), torch.empty((c.P,), dtype=torch.int32, device=dev)
    unbound = torch.full((c.P,), -1, dtype=torch.int32, device=dev)
    out = {"part": "live_loop", "config": name, "P": c.P, "N": c.N, "steps": steps}
    with Evaluator(0) as ev:
        s = torch.cuda.current_stream()
        ev.set_nodes(**c.node_columns())
        start = ev.read_nodes()

        def step(pick, samples):
            e0, em, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s)
            ev.eval_device(rc_t, rm_t, sel_t, tol_t, samples, flags | pick, out_binding=bind, stream=s)
            em.record(s)
            ev.apply_bindings_device(bind, rc_t, rm_t, flags=_lib.APPLY_WHILE_FIT, status_out=status, stream=s)
            e1.record(s)
            taken = torch.where(status == _lib.APPLY_APPLIED, bind, unbound)
            ev.apply_bindings_device(taken, rc_t, rm_t, flags=_lib.APPLY_RELEASE, stream=s)  # (a change again: the next step's evaluation follows it)
            e1.synchronize()
            return (e0.elapsed_time(e1) * 1e3, e0.elapsed_time(em) * 1e3), int((bind >= 0).sum().item()), int((taken >= 0).sum().item())

        picks = (("bestfit", PICK_BESTFIT, None), ("pack_d5", PICK_PACK, smp))
        last_pick = {}
        spans = {k: [] for k, _, _ in picks}
        evals = {k: [] for k, _, _ in picks}
        for r in range(warmup + steps):
            for k, pick, samples in picks:
                (us, eval_us), bound, admitted = step(pick, samples)
                if r >= warmup:
                    spans[k].append(us)
                    evals[k].append(eval_us)
                last_pick[k] = ev.last_pick
                out.setdefault(k + "_bound", bound)
                out.setdefault(k + "_admitted", admitted)
                assert out[k + "_admitted"] == admitted, "the snapshot was not restored between the steps"
        end = ev.read_nodes()
        assert np.array_equal(start[0], end[0]) and np.array_equal(start[1], end[1]), "the releases did not restore the snapshot"
        for k, _, _ in picks:
            out[k] = stats(spans[k])
            out[k + "_evaluate_and_pick"] = stats(evals[k])
            out[k + "_last_pick"] = last_pick[k]
    out["pack_over_bestfit_step_time"] = out["pack_d5"]["median_us"] / out["bestfit"]["median_us"]
    return out


def herd() -> dict:
    import torch
    from kube_scheduler_rs_reference_amd import FIT, PICK_BESTFIT, PICK_PACK, SEL, Evaluator, _lib, synth
    c = synth.make_config("C3")
    flags = FIT | SEL
    req_cpu = np.full_like(c.req_cpu, int(np.median(c.req_cpu)))  # one request for everybody: the median pod's
    req_mem = np.full_like(c.req_mem, int(np.median(c.req_mem)))
    (rc_t, rm_t, sel_t, _), t = device_columns(torch, c, req_cpu, req_mem)
    draws = np.random.default_rng(0xE56).integers(0, 1 << 32, size=(c.P, 5), dtype=np.uint64).astype(np.uint32)
    dev = torch.device("cuda:0")
    bind, status = torch.empty((c.P,), dtype=torch.int32, device=dev), torch.empty((c.P,), dtype=torch.int32, device=dev)
    out = {"part": "herd", "P": c.P, "N": c.N}
    for k, pick, d in (("bestfit", PICK_BESTFIT, 0), ("pack_d2", PICK_PACK, 2), ("pack_d5", PICK_PACK, 5)):
        with Evaluator(0) as ev:
            s = torch.cuda.current_stream()
            ev.set_nodes(**c.node_columns())
            ev.eval_device(rc_t, rm_t, sel_t, None, t(draws[:, :d], np.int32) if d else None, flags | pick, out_binding=bind, stream=s)
            ev.apply_bindings_device(bind, rc_t, rm_t, flags=_lib.APPLY_WHILE_FIT, status_out=status, stream=s)
            torch.cuda.synchronize()
            b, st = bind.cpu().numpy(), status.cpu().numpy()
            out[k] = {"bound_pods": int((b >= 0).sum()), "bound_nodes": int(len(np.unique(b[b >= 0]))),
                      "most_pods_on_one_node": int(np.bincount(b[b >= 0]).max()) if (b >= 0).any() else 0,
                      "admitted": int((st == _lib.APPLY_APPLIED).sum()), "deferred": int((st == _lib.APPLY_DEFERRED).sum())}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--configs", default="C3,C5s")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    lines, raw = [f"# tools/pack_pick_cost.py --calls {a.calls} --warmup {a.warmup} --steps {a.steps} --configs {a.configs}: median us (min, p90), device events, candidates alternating"], []

    def emit(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    emit("1. k_pick_pack against k_pick_spread: ksched_pick_device on one mask")
    for name in a.configs.split(","):
        r = kernels(name, a.calls, a.warmup)
        raw.append(r)
        emit(f"{name} ({r['P']} x {r['N']}, W {r['W']}, pitch {r['pitch_words']} words):")
        for k in [k for k in r if k[0] in "apb" and k[1:2].isdigit()]:
            tag, what = k.split("_", 1)
            emit(f"  ({tag}) {what:<18} {r[k]['median_us']:9.1f} us  (min {r[k]['min_us']:.1f}, p90 {r[k]['p90_us']:.1f})")
        for d, v in r["inside"].items():
            emit(f"  {d}: spread {v['spread_a_us']:.1f} / {v['spread_b_us']:.1f} us, pack {v['pack_us']:.1f} us = {v['pack_over_spread']:.3f} x; inside "
                 f"[{v['low_us']:.1f}, {v['high_us']:.1f}]: {v['pack_inside']}; {100 * r[d + '_pods_bound_to_different_nodes']:.1f} % of the bound pods get another node than from the spread pick")
    emit("2. the live loop: [evaluate + pick, apply WHILE_FIT] per step, every evaluation behind a snapshot change")
    if "C5s" in a.configs.split(","):
        r = live_loop("C5s", a.steps, max(3, a.warmup // 4))
        raw.append(r)
        emit(f"C5s ({r['P']} x {r['N']}, {r['steps']} steps each, alternating):")
        for k in ("bestfit", "pack_d5"):
            emit(f"  {k:<8} {r[k]['median_us']:9.1f} us per step (min {r[k]['min_us']:.1f}, p90 {r[k]['p90_us']:.1f}), of which evaluate + pick {r[k + '_evaluate_and_pick']['median_us']:.1f} us "
                 f"(ksched_last_pick \"{r[k + '_last_pick']}\"); {r[k + '_bound']} pods bound, {r[k + '_admitted']} admitted per call")
        emit(f"  pack / bestfit step time: {r['pack_over_bestfit_step_time']:.3f}")
    emit("3. the herd: C3's nodes, every pod with the median request, one evaluation + one APPLY_WHILE_FIT")
    r = herd()
    raw.append(r)
    for k in ("bestfit", "pack_d2", "pack_d5"):
        v = r[k]
        emit(f"  {k:<8} {v['bound_pods']} pods bound to {v['bound_nodes']} nodes (most on one node: {v['most_pods_on_one_node']}); admitted {v['admitted']}, deferred {v['deferred']}")
    with open(os.path.join(a.out_dir, "pack_pick_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out_dir, "pack_pick_cost.json"), "w") as f:
        for r in raw:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
