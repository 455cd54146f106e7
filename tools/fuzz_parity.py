#!/usr/bin/env python
"""Randomised differential test of the HIP path against the oracle (GPU box): random shapes, key counts and cardinalities (incl.
list keys and > 8 keys), taints, predicate subsets, the sampled and best-fit picks, snapshot updates between evaluations (ksched_update_nodes or,
as its alternative, ksched_update_node_labels: ids within each key's current maximum, or above it -- the layout is planned again -- with taints
now and then), both kernels, per-pair reasons (ksched_explain), per-pod node counts by reason (ksched_summarize),
the uniform pick (KSCHED_PICK_UNIFORM) at every step of every case -- both kernels, with and without the mask, now and then with
WANT_FIT_MASK, full-range 32-bit draws with an occasional all-zero or all-ones column -- against tests/uniform_ref.py on the oracle's mask,
and through ksched_pick (the oracle's mask and a thinned one), the row shards and the multi-device sequence below; about one case in ten
has 8192, 8193 or 12 500 nodes (rows of more than 128 words: the two-pass form of k_pick_uniform),
the spread pick (KSCHED_PICK_SPREAD) at every step of every case as well -- d drawn from 1, 2, 3, 5, 8, 33, 64, both kernels, with and without the
mask -- against tests/spread_ref.py on the oracle's mask AND on the step's restated columns: it is the one pick that reads the values an update or an
apply has just written, so a column left stale shows as a few wrong bindings; through ksched_pick, the row shards and the multi-device sequence too,
the latter followed by a sharded apply of the gathered bindings over the same replicas and a second sequence on the columns that apply left (no
ksched_set_nodes in between); the wide cases take k_pick_spread's two-pass form, with draws that arrive out of chunk order,
the pack pick (KSCHED_PICK_PACK) at every step of every case too -- the same table of draws, d drawn from the same list, both kernels, with and without
the mask -- against tests/pack_ref.py on the oracle's mask and the step's restated columns; with the hooks through the spread pick's multi-device
route (the sequence, a sharded apply of the gathered bindings, the sequence again),
one combining chain at every step (KSCHED_COMBINE_AND / _OR / _ANDNOT, KSCHED_COMBINE_SOFT at random on AND and AND-NOT): 2 to 4 calls of
ksched_eval_device on one mask, each with a random non-empty predicate subset, into a view at pitch W, W + 1 or ksched_mask_pitch(n) that starts at
an even or an odd word of a buffer of sentinel words, the mask copied on the stream after every link, a random pick or none in the last link --
against tests/combine_ref.py / tests/soft_ref.py on the oracle's per-link masks and the pick restatements on the final mask; with the hooks the same
chain on every replica after the pack pick's sharded apply, on the columns it left,
one operator call (KSCHED_SELOP_EXISTS / _GT / _LT at random, on the step's selector table) and one tagged call (KSCHED_SELOP_TAGGED, on a table of
its own: all six tags, now and then tag 6 or 7, ids drawn from the nodes' ids, those ids + / - 1, and 0, 1 and 0x1FFFFFFF) at every step, over the
batch's first 200 pods -- each into a view with sentinel words around it at pitch W, W + 1 or ksched_mask_pitch(n), about half of them as one more
link on the final mask of the step's combining chain (a random op, KSCHED_COMBINE_SOFT at random), with a random pick or none -- against
tests/selop_ref.py / tests/seltag_ref.py on the labels as the step's updates left them (apply_rows), tests/combine_ref.py / tests/soft_ref.py and the
pick restatements on the resulting mask and the step's columns; both also through ksched_eval_begin / _end over 1 to 5 row shards with the uniform
pick (sel_stride > p); where the whole batch gives a block of the operator kernel two pod tiles to walk, one more operator call over all its
pods, compared on 1024 rows or fewer; with the hooks both calls on every replica after the pack pick's sharded apply,
one terms call (KSCHED_SEL_TERMS: SEL | SELOP_TAGGED | sel_terms(T), T of 1, 2, 3, 15) at every step with keys, on a table [T][n_keys][p] of its
own built like the tagged call's -- per-pod term counts with SEL_NEVER padding behind them, in a share of the pods a zero term behind a real
one -- over the batch's first pods (200 at most, about 600 / T): the bare mask and the call as one more link on the step's chain under a drawn
op (KSCHED_COMBINE_SOFT at random) with a drawn pick, against tests/selterms_ref.py on the labels as the step's updates left them; through
ksched_eval_begin / _end over 1 to 5 row shards, column (t, k) at (t * n_keys + k) * sel_stride; with the hooks on every replica likewise,
on-device applies of the previous evaluation's bindings between evaluations (ksched_apply_bindings_device; with the hooks on, now and then
ksched_apply_bindings_sharded_local over 2 .. 4 replicas with ragged cuts; about one apply in four with KSCHED_APPLY_WHILE_FIT, against
tests/admit_ref.py -- the sharded entry point must then refuse with KSCHED_E_UNSUPPORTED and leave every replica as it was; tallies
'apply-while-fit', 'apply-while-fit-deferred' for those that deferred a pod, 'while-fit-refused-sharded'),
the two halves of ksched_eval over 1 .. 5 row shards (ksched_shard_bounds / ksched_eval_begin / ksched_eval_end) and -- with the test hooks on
(KSCHED_TEST_HOOKS=1 KSCHED_RCCL_LIB=tests/cpp/libfake_rccl.so) -- the whole multi-device sequence over 2 .. 4 evaluators on the one GPU:
ksched_comm_create_local, ksched_eval_begin on every replica, ksched_gather_buffer, ksched_allgather_bindings_local, ksched_eval_end(gathered_0).
A case's decisions come from three generators seeded from the case seed: `r` draws what the tool has always drawn, in the same order (a
case that keeps its node count is the case an older log names by that seed), `r2` every decision added with the uniform pick (the uniform legs,
the wider snapshots, the label updates), in its order, and `r3` every decision added since (the spread legs): a seed names the case it named
before the spread legs, with those legs added; `r4` every decision of the pack legs and the combining chains, likewise; `r5` every decision of
the operator and the tagged calls, likewise; `r6` every decision of the terms call, likewise.
The summary's tallies: pick launches by name ('uniform': evaluations whose last_pick was "uniform"; 'uniform-ranked': those in which some
pod had two or more feasible nodes, so the rank arithmetic ran), 'labels' (label updates), 'apply', 'host-masks', 'sharded-halves',
'gathered-over-n' (and their 'uniform-' and 'spread-' twins), 'summarize'; 'spread': evaluations whose last_pick was "spread" (one per
ksched_eval; a multi-device sequence counts as one, whatever the number of replicas, as it does for 'uniform');
'spread-ranked': those in which some pod was bound to another node than its candidate 0; 'spread-tied': those in which some pod's winner was
decided by cpu or by the node index (two distinct candidates with the same, largest memory); 'spread-gathered-moved': second sequences in which
the columns from before the gathered apply would have given some pod another binding; 'pack', 'pack-ranked', 'pack-gathered-over-N' and
'pack-gathered-moved' as their spread twins; 'combine': chains run on `ev`; 'soft-narrowed', 'soft-dropped', 'soft-empty': chains in which a
soft link narrowed a row, was dropped for one, met an empty one; 'combine-on-replicas': cases whose chain ran on every replica;
'selop', 'seltag': operator and tagged calls run on `ev` through ksched_eval_device; 'seltag-negated-padding': tagged calls with a pod constrained
through NE / ABSENT entries only on a node count that is no multiple of 64 (valid-bits applied before the negation would set padding bits);
'selop-two-pass': operator calls on more than eight keys; 'selop-two-tiles': operator calls over a whole batch whose blocks walk two pod tiles or
more; 'selop-sharded-halves': operator and tagged calls through the two halves; 'selop-on-replicas': cases whose two calls ran on every replica;
'selterms': terms calls run on `ev` through ksched_eval_device; 'selterms-wide': those on more than eight keys (k_eval_selterms_wide);
'selterms-late-full': those with a pod whose row is full although term 0's row is not (a term behind term 0 completes it);
'selterms-sharded-halves': terms calls through the two halves; 'selterms-on-replicas': cases whose terms call ran on every replica.
usage: python tools/fuzz_parity.py [seconds] [seed]       prints one line per failure and a summary; exit code 1 on any failure"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kube_scheduler_rs_reference_amd import Evaluator, _lib as L
from oracle import capi
# the exact-integer apply rule (oracle_ref.apply_bindings_exact) under the name the GPU tests import it by: through that name the tool
# also runs with an oracle/ that predates the shared restatement
from tests.test_gpu_apply_bindings import restate as apply_bindings_exact
from tests.admit_ref import apply_while_fit_exact  # KSCHED_APPLY_WHILE_FIT restated
from tests.test_gpu_node_labels import apply_rows  # the columns after ksched_update_node_labels: a node listed twice takes its last row
from tests.uniform_ref import uniform_pick  # KSCHED_PICK_UNIFORM restated
from tests.spread_ref import best_of, spread_candidates_listed  # KSCHED_PICK_SPREAD restated: every draw's candidate, the best of them
from tests.pack_ref import tightest_of  # KSCHED_PICK_PACK restated: the tightest of the same candidates
from tests import combine_ref, soft_ref  # KSCHED_COMBINE_AND / _OR / _ANDNOT and KSCHED_COMBINE_SOFT restated
from tests import selop_ref, seltag_ref  # KSCHED_SELOP_EXISTS / _GT / _LT and KSCHED_SELOP_TAGGED restated
from tests import selterms_ref  # KSCHED_SEL_TERMS restated
from tests.knife_edges import sampled as sampled_from_bits  # ksched_pick's rule for PICK_SAMPLED on a [p, n] table of bits
from tests.test_gpu_combine_soft import old_mask_for  # an old mask whose neighbouring rows narrow, are dropped, are empty and are random

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
ev = Evaluator(0)
# the multi-device sequence with n > 1 needs the TEST-ONLY librccl stand-in (one GPU stands for n ranks): replicas + one clique per n, made on first use
HOOKS = os.environ.get("KSCHED_TEST_HOOKS") == "1" and bool(os.environ.get("KSCHED_RCCL_LIB"))
if HOOKS and not hasattr(L.load(), "ksched_test_hooks_linked"):  # the stand-in is loadable by the TEST build of the library only (KSCHED_LIB=tests/cpp/hooks/libksched_hip.so)
    print("fuzz: KSCHED_TEST_HOOKS is set but the loaded library is the shipped one (no hooks): the n > 1 multi-device cases are left out; set KSCHED_LIB=tests/cpp/hooks/libksched_hip.so", flush=True)
    HOOKS = False
replicas, cliques = [], {}


def uniform_pick_blocks(mask, draws, n, cells=1 << 24):
    """uniform_pick in blocks of pods: the restatement holds a [pods, n] int64 table, and a case here has up to 52 225 pods"""
    step = max(1, cells // max(int(n), 1))
    if mask.shape[0] <= step:
        return uniform_pick(mask, draws, n)
    return np.concatenate([uniform_pick(mask[lo:lo + step], draws[lo:lo + step], n) for lo in range(0, mask.shape[0], step)])


def spread_restated(mask, draws, n, mem, cpu, cells=1 << 24):
    """tests/spread_ref.py in blocks of pods (spread_pick_blocks, keeping the candidates for the tallies) -> (the bindings, whether some pod
    is bound to another node than its candidate 0, whether some pod's largest memory is shared by two distinct candidates)"""
    step = max(1, cells // max(int(n), 1))
    out, ranked, tied = [], False, False
    for lo in range(0, mask.shape[0], step):
        cand = spread_candidates_listed(mask[lo:lo + step], draws[lo:lo + step], n)
        b = best_of(cand, mem, cpu)
        out.append(b)
        ranked = ranked or bool(((b >= 0) & (b != cand[:, 0])).any())
        v = cand[cand[:, 0] >= 0].astype(np.int64)
        if v.size and not tied:
            m = mem[v]
            top = m == m.max(axis=1, keepdims=True)
            tied = bool((np.where(top, v, n).min(axis=1) != np.where(top, v, -1).max(axis=1)).any())
    return np.concatenate(out), ranked, tied


def pack_restated(mask, draws, n, mem, cpu, cells=1 << 24):
    """tests/pack_ref.py in blocks of pods -> (the bindings, whether some pod is bound to another node than its candidate 0, False)"""
    step = max(1, cells // max(int(n), 1))
    out, ranked = [], False
    for lo in range(0, mask.shape[0], step):
        cand = spread_candidates_listed(mask[lo:lo + step], draws[lo:lo + step], n)
        b = tightest_of(cand, mem, cpu)
        out.append(b)
        ranked = ranked or bool(((b >= 0) & (b != cand[:, 0])).any())
    return np.concatenate(out), ranked, False


def pick_on_mask(pick, cur, draws, N, cpu, mem):
    """what a pick in a combining (or an operator, or a tagged) call binds: ksched_pick's rule on the resulting mask `cur` with the pick
    flag alone; None without a pick"""
    if pick == L.PICK_UNIFORM:
        return uniform_pick_blocks(cur, draws[:, 0], N)
    if pick == L.PICK_SPREAD:
        return spread_restated(cur, draws, N, mem, cpu)[0]
    if pick == L.PICK_PACK:
        return pack_restated(cur, draws, N, mem, cpu)[0]
    if not pick:
        return None
    from kube_scheduler_rs_reference_amd.evaluator import unpack_mask
    bits = unpack_mask(cur, N)
    if pick == L.PICK_SAMPLED:
        return sampled_from_bits(bits, draws)
    # best fit, not told that the mask includes the fit: the set bit with the smallest (avail_mem, avail_cpu, node)
    order = np.lexsort((np.arange(N), cpu, mem))
    f = bits[:, order]
    return np.where(f.any(axis=1), order[f.argmax(axis=1)], -1).astype(np.int32)


CHAIN_PODS = 2000  # a combining chain takes the batch's first pods, at most so many (the oracle runs once per link)
SENTINEL, GUARD_ROWS = 0x5A5A5A5A5A5A5A5A, 2


def draw_chain(g, N, P, K, nt):
    """one combining chain of 2 to 4 links: per link a non-empty predicate subset, an op and (on AND and AND-NOT, at random)
    KSCHED_COMBINE_SOFT; the view's pitch (W, W + 1 or ksched_mask_pitch(n)) and whether it starts at an even or an odd word of its
    buffer; the pick of the last link, or none; the kernel choice"""
    W = (N + 63) // 64
    avail = [L.FIT] + ([L.SEL] if K else []) + ([L.TAINT] if nt else [])
    links = []
    for _ in range(int(g.integers(2, 5))):
        sub = 0
        while not sub:
            sub = sum(f for f in avail if g.random() < 0.5)
        op = int(g.choice(combine_ref.OPS))
        links.append((sub, op, soft_ref.SOFT if op != combine_ref.OR and g.random() < 0.5 else 0))
    return dict(links=links, pitch=int(g.choice([W, W + 1, int(ev._lib.ksched_mask_pitch(N))])), offset=int(g.integers(0, 2)),
                pick=int(g.choice([0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_UNIFORM, L.PICK_SPREAD, L.PICK_PACK])),
                kernel=str(g.choice(["auto", "direct"])), seed=int(g.integers(0, 1 << 31)))


def run_chain(e, cs, where, spec, cpu, mem, lab, taints, N, P, K, nt, rc, rm, sel, tol, smp, smp_u, smp_s):
    """the chain `spec` on evaluator `e`, whose snapshot should hold cpu / mem: every link a ksched_eval_device into one [p, W] view with
    sentinel words around it, the mask copied on the stream after every link.  Expected: tests/combine_ref.py / tests/soft_ref.py on the
    oracle's per-link masks (on cpu / mem), from an old mask whose rows narrow, are dropped and are empty under the first link
    (old_mask_for), and for the last link's pick the restatement of ksched_pick's rule on the final mask.  -> the number of failures"""
    import torch
    dev = torch.device("cuda:0")
    p, W = min(P, CHAIN_PODS), (N + 63) // 64
    pitch, offset, pick = spec["pitch"], spec["offset"], spec["pick"]
    if pick == L.PICK_BESTFIT and any(a.size and (int(a.min()) < -(1 << 61) or int(a.max()) > (1 << 61)) for a in (cpu, mem, rc, rm)):
        pick = L.PICK_PACK  # (best fit ranks by the residual, which orders as `available` only while the subtraction stays inside int64)
    rc_p, rm_p = np.ascontiguousarray(rc[:p]), np.ascontiguousarray(rm[:p])
    sel_p = np.ascontiguousarray(sel[:, :p]) if K else None
    tol_p = np.ascontiguousarray(tol[:p]) if nt else None
    new = [capi.eval_encoded(cpu, mem, lab, taints if (sub & L.TAINT) else None, rc_p, rm_p, sel_p, tol_p if (sub & L.TAINT) else None, None, sub)[0]
           for sub, _, _ in spec["links"]]
    op0 = spec["links"][0][1]
    old = old_mask_for(new[0], combine_ref.AND if op0 == combine_ref.OR else op0, N, np.random.default_rng(spec["seed"]))
    want, cur, seen_dec = [], old, set()
    for (sub, op, soft), m in zip(spec["links"], new):
        if soft:
            seen_dec.update(np.unique(soft_ref.decisions(cur, m, op, N)).tolist())
            cur = soft_ref.soft_combine(cur, m, op, N)
        else:
            cur = combine_ref.combine(cur, m, op, N)
        want.append(cur)
    draws = {L.PICK_SAMPLED: smp, L.PICK_UNIFORM: smp_u, L.PICK_SPREAD: smp_s, L.PICK_PACK: smp_s}.get(pick)
    draws = None if draws is None else np.ascontiguousarray(draws[:p])
    want_b = pick_on_mask(pick, cur, draws, N, cpu, mem)
    spec["final"] = cur  # (the step's selector calls combine into it)
    rows = p + GUARD_ROWS
    host = np.full(offset + rows * pitch + 1, SENTINEL, dtype=np.uint64)
    host[offset:offset + rows * pitch].reshape(rows, pitch)[:p, :W] = old
    buf = torch.from_numpy(host.view(np.int64)).to(dev)
    view = buf[offset:offset + rows * pitch].view(rows, pitch)[:p, :W]
    td = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t, sel_t, tol_t, smp_t = td(rc_p, np.int64), td(rm_p, np.int64), td(sel_p, np.int32), td(tol_p, np.int64), td(draws, np.int32)
    out = torch.full((p + 4,), -7, dtype=torch.int32, device=dev)
    e.set_kernel(spec["kernel"])
    copies = []
    for i, (sub, op, soft) in enumerate(spec["links"]):
        last = i == len(spec["links"]) - 1
        e.eval_device(rc_t, rm_t, sel_t if (sub & L.SEL) else None, tol_t if (sub & L.TAINT) else None, smp_t if last and pick else None,
                      sub | op | soft | (pick if last else 0), out_feasible=view, out_binding=out[:p] if last and pick else None)
        copies.append(buf.clone())
    torch.cuda.synchronize()
    e.set_kernel("auto")
    bad = 0
    what = (f"case seed {cs} {where}: N={N} p={p} K={K} nt={nt} links={[(hex(a), combine_ref.NAMES[b] + ('-soft' if c else '')) for a, b, c in spec['links']]} "
            f"pitch={pitch} offset={offset} pick={pick:#x} kernel={spec['kernel']}")
    for i, (c, w) in enumerate(zip(copies, want)):
        got = c.cpu().numpy().view(np.uint64)
        body = got[offset:offset + rows * pitch].reshape(rows, pitch)
        pad = body[:p, W:]
        if not np.array_equal(body[:p, :W], w):
            bad += 1
            print(f"FAIL combine {what}: the mask after link {i} ({int((body[:p, :W] != w).any(axis=1).sum())} rows differ)", flush=True)
            break
        if not (((pad == SENTINEL) | (pad == 0)).all() and (body[p:] == SENTINEL).all() and (got[:offset] == SENTINEL).all() and got[-1] == SENTINEL):
            bad += 1
            print(f"FAIL combine {what}: link {i} wrote outside words [0, W) of the view's rows", flush=True)
            break
    if pick:
        b = out.cpu().numpy()
        if not (np.array_equal(b[:p], want_b) and (b[p:] == -7).all()):
            bad += 1
            print(f"FAIL combine {what}: the last link's pick ({int((b[:p] != want_b).sum())} bindings differ)", flush=True)
    picks["combine"] = picks.get("combine", 0) + 1
    for k, name in ((soft_ref.NARROWED, "soft-narrowed"), (soft_ref.DROPPED, "soft-dropped"), (soft_ref.EMPTY, "soft-empty")):
        if k in seen_dec:
            picks[name] = picks.get(name, 0) + 1
    return bad


SELOP_FLAGS = (L.SELOP_EXISTS, L.SELOP_GT, L.SELOP_LT)
SELCALL_PODS = 200  # an operator / tagged call takes the batch's first pods, at most so many (the restatements' time)
assert SELOP_FLAGS == selop_ref.OPS and L.SELOP_TAGGED == seltag_ref.TAGGED


def in_pod_blocks(fn, entries, n, cells=1 << 25):
    """fn(entries [K][pods]) -> packed rows, in blocks of pods (the restatements hold [pods, n] tables)"""
    step = max(1, cells // max(int(n), 1))
    return np.concatenate([fn(np.ascontiguousarray(entries[:, lo:lo + step])) for lo in range(0, entries.shape[1], step)])


def draw_selcalls(g, lab, N, P, K):
    """the step's operator call and tagged call (generator r5): the operator; the tagged table [K][P] -- per entry constrained with a
    probability drawn per step, all six tags, now and then tag 6 or 7, the id one of the key's node ids, such an id + / - 1, or 0, 1 or
    0x1FFFFFFF --; per call the view's pitch (W, W + 1 or ksched_mask_pitch(n)) and its even or odd start, whether it runs as a link on the
    step's combining chain (about half: then with a random op, KSCHED_COMBINE_SOFT at random on AND and AND-NOT) and the pick or none;
    the shard count of the two halves; and, where the whole batch would give a block of the operator kernel more than one pod tile to walk
    (plan_selop_launch: ceil(P / 64) > ceil(2048 / ceil(W / 16)) -- here 40 000 pods or more on 2500 nodes or more), the rows of one more
    operator call over all P pods that are compared: the first and the last 256 and 512 random ones"""
    W = (N + 63) // 64
    tsel = None
    if K:
        pk = float(g.choice([0.05, 0.3, 0.9]))
        near = lab[np.arange(K)[:, None], g.integers(0, N, (K, P))].astype(np.int64) + g.integers(-1, 2, (K, P))
        ident = np.where(g.random((K, P)) < 0.8, near, g.choice(np.array([0, 1, seltag_ref.ID_MASK]), (K, P))) & seltag_ref.ID_MASK
        tags = np.where(g.random((K, P)) < 0.03, g.integers(6, 8, (K, P)), g.integers(0, 6, (K, P)))
        tsel = np.ascontiguousarray(np.where(g.random((K, P)) < pk, seltag_ref.entry(tags, ident), 0).astype(np.uint32))

    gx = (W + 15) // 16
    whole = None
    if (P + 63) // 64 > (2048 + gx - 1) // gx:
        whole = np.unique(np.concatenate([np.arange(min(P, 256)), np.arange(max(P - 256, 0), P), g.integers(0, P, 512)]))

    def call():
        op = int(g.choice(combine_ref.OPS))
        return dict(pitch=int(g.choice([W, W + 1, int(ev._lib.ksched_mask_pitch(N))])), offset=int(g.integers(0, 2)), link=bool(g.random() < 0.5), comb=op,
                    soft=soft_ref.SOFT if op != combine_ref.OR and g.random() < 0.5 else 0,
                    pick=int(g.choice([0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_UNIFORM, L.PICK_SPREAD, L.PICK_PACK])))
    return dict(op=int(g.choice(SELOP_FLAGS)), tsel=tsel, calls=(call(), call()), whole=whole, shards=int(g.choice([1, 2, 3, 5])))


def selcall_masks(spec, lab, sel, N, P, K):
    """the expected bare masks of the step's two calls on the labels `lab` (the updated ones after a label update): -> (p, the operator
    call's mask [p, W] from tests/selop_ref.py on sel, the tagged call's from tests/seltag_ref.py on spec's table -- None without keys)"""
    p = min(P, SELCALL_PODS)
    if not K:
        return p, selop_ref.selop_mask(np.zeros((0, N), np.uint32), None, spec["op"], p=p), None
    return (p, in_pod_blocks(lambda e: selop_ref.selop_mask(lab, e, spec["op"]), sel[:, :p], N),
            in_pod_blocks(lambda e: seltag_ref.seltag_mask(lab, e), spec["tsel"][:, :p], N))


def run_one_selcall(e, cs, where, name, kernel, flags, entries, new, c, p, chain_final, cpu, mem, N, K, rc, rm, smp, smp_u, smp_s):
    """one selector call (operator, tagged or terms) on evaluator `e`: a ksched_eval_device of the first p pods of `entries` ([...][pods]) into
    a [p, W] view with sentinel words around it -- plain, or as one more link on the final mask of the step's combining chain (the first p
    rows of `chain_final`) -- with the call's pick (`c`: pitch, offset, link, comb, soft, pick).  Expected: `new`, the call's bare mask from
    its restatement, combined by tests/combine_ref.py / tests/soft_ref.py, and the pick restated on the resulting mask; last_kernel must be
    `kernel`.  -> the number of failures"""
    import torch
    dev = torch.device("cuda:0")
    W = (N + 63) // 64
    td = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    rc_t, rm_t = td(rc[:p], np.int64), td(rm[:p], np.int64)
    bad = 0
    pitch, offset, pick = c["pitch"], c["offset"], c["pick"]
    link = c["link"] and chain_final is not None and chain_final.shape[0] >= p
    old = np.ascontiguousarray(chain_final[:p]) if link else None
    if pick == L.PICK_BESTFIT and any(a.size and (int(a.min()) < -(1 << 61) or int(a.max()) > (1 << 61)) for a in (cpu, mem)):
        pick = L.PICK_PACK  # (as in run_chain)
    comb = (c["comb"] | c["soft"]) if link else 0
    if link:
        want = soft_ref.soft_combine(old, new, c["comb"], N) if c["soft"] else combine_ref.combine(old, new, c["comb"], N)
    else:
        want = new
    draws = {L.PICK_SAMPLED: smp, L.PICK_UNIFORM: smp_u, L.PICK_SPREAD: smp_s, L.PICK_PACK: smp_s}.get(pick)
    draws = None if draws is None else np.ascontiguousarray(draws[:p])
    want_b = pick_on_mask(pick, want, draws, N, cpu, mem)
    rows = p + GUARD_ROWS
    host = np.full(offset + rows * pitch + 1, SENTINEL, dtype=np.uint64)
    if link:
        host[offset:offset + rows * pitch].reshape(rows, pitch)[:p, :W] = old
    buf = torch.from_numpy(host.view(np.int64)).to(dev)
    view = buf[offset:offset + rows * pitch].view(rows, pitch)[:p, :W]
    out = torch.full((p + 4,), -7, dtype=torch.int32, device=dev)
    e.eval_device(rc_t, rm_t, td(entries[..., :p], np.int32) if K else None, None, td(draws, np.int32) if pick else None, flags | comb | pick,
                  out_feasible=view, out_binding=out[:p] if pick else None)
    ran = e.last_kernel
    torch.cuda.synchronize()
    what = (f"case seed {cs} {where}: N={N} p={p} K={K} flags={flags | comb | pick:#x} pitch={pitch} offset={offset}" +
            (" on the step's chain" if link else ""))
    got = buf.cpu().numpy().view(np.uint64)
    body = got[offset:offset + rows * pitch].reshape(rows, pitch)
    pad = body[:p, W:]
    if ran != kernel:
        bad += 1
        print(f"FAIL {name} call {what}: ran as {ran!r}", flush=True)
    if not np.array_equal(body[:p, :W], want):
        bad += 1
        print(f"FAIL {name} call {what}: the mask ({int((body[:p, :W] != want).any(axis=1).sum())} rows differ)", flush=True)
    elif not (((pad == SENTINEL) | (pad == 0)).all() and (body[p:] == SENTINEL).all() and (got[:offset] == SENTINEL).all() and got[-1] == SENTINEL):
        bad += 1
        print(f"FAIL {name} call {what}: wrote outside words [0, W) of the view's rows", flush=True)
    if pick:
        b = out.cpu().numpy()
        if not (np.array_equal(b[:p], want_b) and (b[p:] == -7).all()):
            bad += 1
            print(f"FAIL {name} call {what}: the pick ({int((b[:p] != want_b).sum())} bindings differ)", flush=True)
    return bad


def run_selcalls(e, cs, where, spec, masks, chain_final, cpu, mem, N, P, K, rc, rm, sel, smp, smp_u, smp_s, tally=True):
    """the step's operator call and tagged call on evaluator `e` (whose labels should be the ones `masks` was computed on, whose columns
    cpu / mem): each through run_one_selcall, against `masks` (selcall_masks).  -> the number of failures"""
    p, want_op, want_tag = masks
    bad = 0
    for name, kernel, flags, entries, new, c in (("operator", "selop", L.SEL | spec["op"], sel, want_op, spec["calls"][0]),
                                                 ("tagged", "seltag", L.SEL | L.SELOP_TAGGED, spec["tsel"], want_tag, spec["calls"][1])):
        if new is None:
            continue
        bad += run_one_selcall(e, cs, where, name, kernel, flags, entries, new, c, p, chain_final, cpu, mem, N, K, rc, rm, smp, smp_u, smp_s)
        if not tally:
            continue
        picks[kernel] = picks.get(kernel, 0) + 1
        if kernel == "selop":
            if K > 8:
                picks["selop-two-pass"] = picks.get("selop-two-pass", 0) + 1
        elif N % 64:  # a pod constrained through NE / ABSENT entries only, in rows whose last word has padding bits
            ent = entries[:, :p]
            tag = ent >> np.uint32(seltag_ref.SHIFT)
            neg = (ent != 0) & ((tag == seltag_ref.NE) | (tag == seltag_ref.ABSENT))
            if ((ent != 0).any(axis=0) & (neg == (ent != 0)).all(axis=0)).any():
                picks["seltag-negated-padding"] = picks.get("seltag-negated-padding", 0) + 1
    return bad


def draw_selterms(g, lab, N, P, K):
    """the step's terms call (KSCHED_SEL_TERMS; generator r6), None without keys: the term count T of {1, 2, 3, 15}; the pods (the batch's
    first ones, at most SELCALL_PODS and, for the restatement's time, about 600 / T, never fewer than 65 where the batch has them: a second
    pod tile); the entries [T][K][p], built as draw_selcalls builds its tagged table -- constrained with a probability drawn per step, all six
    tags, now and then tag 6 or 7, ids from beside the nodes' ids or 0, 1, 0x1FFFFFFF --; a term count c of 1 .. T per pod, every term at or
    behind it the documented padding (all zeros, SEL_NEVER in one drawn key); in about a seventh of the pods with c >= 2 term 1 all zeros, a
    zero term behind a real one; the decisions of the bare call and of the combining call (draw_selcalls' call()); the shard count of the
    two halves"""
    if not K:
        return None
    W = (N + 63) // 64
    T = int(g.choice([1, 2, 3, selterms_ref.MAX_TERMS]))
    p = min(P, SELCALL_PODS, max(65, 600 // T))
    pk = float(g.choice([0.05, 0.3, 0.9]))
    near = lab[np.arange(K)[None, :, None], g.integers(0, N, (T, K, p))].astype(np.int64) + g.integers(-1, 2, (T, K, p))
    ident = np.where(g.random((T, K, p)) < 0.8, near, g.choice(np.array([0, 1, seltag_ref.ID_MASK]), (T, K, p))) & seltag_ref.ID_MASK
    tags = np.where(g.random((T, K, p)) < 0.03, g.integers(6, 8, (T, K, p)), g.integers(0, 6, (T, K, p)))
    ent = np.where(g.random((T, K, p)) < pk, seltag_ref.entry(tags, ident), 0).astype(np.uint32)
    c = g.integers(1, T + 1, p)
    pad_key = g.integers(0, K, (T, p))
    for r in range(1, T):
        pods = np.nonzero(c <= r)[0]
        ent[r][:, pods] = 0
        ent[r][pad_key[r][pods], pods] = L.SEL_NEVER
    if T >= 2:
        ent[1][:, (g.random(p) < 0.15) & (c >= 2)] = 0

    def call(link):
        op = int(g.choice(combine_ref.OPS))
        return dict(pitch=int(g.choice([W, W + 1, int(ev._lib.ksched_mask_pitch(N))])), offset=int(g.integers(0, 2)), link=link, comb=op,
                    soft=soft_ref.SOFT if op != combine_ref.OR and g.random() < 0.5 else 0,
                    pick=int(g.choice([0, L.PICK_SAMPLED, L.PICK_BESTFIT, L.PICK_UNIFORM, L.PICK_SPREAD, L.PICK_PACK])) if link else 0)
    return dict(T=T, p=p, ent=np.ascontiguousarray(ent), calls=(call(False), call(True)), shards=int(g.choice([1, 2, 3, 5])))


def selterms_masks(spec, lab, N):
    """the expected bare mask of the step's terms call on the labels `lab`, from tests/selterms_ref.py, and whether a pod's row is full
    although term 0's row is not (a term behind term 0 completes it): -> (mask [p, W], late_full)"""
    want = in_pod_blocks(lambda e: selterms_ref.selterms_mask(lab, e), spec["ent"], N)
    first = in_pod_blocks(lambda e: seltag_ref.seltag_mask(lab, e), spec["ent"][0], N)
    return want, bool(((row_popcounts(want) == N) & (row_popcounts(first) < N)).any())


def run_selterms(e, cs, where, spec, masks, chain_final, cpu, mem, N, P, K, rc, rm, smp, smp_u, smp_s, tally=True):
    """the step's terms call on evaluator `e`, twice through ksched_eval_device (run_one_selcall's views, sentinels and comparisons): the bare
    mask, and as one more link on the final mask of the step's combining chain under the drawn op (KSCHED_COMBINE_SOFT at random) with the
    drawn pick in it.  -> the number of failures"""
    want, late = masks
    flags = L.SEL | L.SELOP_TAGGED | L.sel_terms(spec["T"])
    calls = [spec["calls"][0]]
    if chain_final is not None and chain_final.shape[0] >= spec["p"]:
        calls.append(spec["calls"][1])
    bad = 0
    for c in calls:
        bad += run_one_selcall(e, cs, where, "terms", "selterms", flags, spec["ent"], want, c, spec["p"], chain_final, cpu, mem, N, K, rc, rm, smp, smp_u, smp_s)
    if tally:
        picks["selterms"] = picks.get("selterms", 0) + len(calls)
        if K > 8:
            picks["selterms-wide"] = picks.get("selterms-wide", 0) + len(calls)
        if late:
            picks["selterms-late-full"] = picks.get("selterms-late-full", 0) + len(calls)
    return bad


def selterms_halves(cs, spec, masks, N, K, rc, rm, smp_u, att_u):
    """the terms call through ksched_eval_begin / _end over spec's 1 to 5 row shards of its p pods: the entries as [T * K][p], a shard's
    pointer at its first pod and sel_stride = p, so column (t, k) starts at (t * K + k) * sel_stride; with the uniform pick so that the
    second half has bindings to hand back.  -> the number of failures"""
    p, T = spec["p"], spec["T"]
    draws = np.ascontiguousarray(smp_u[:p])
    return shard_halves(None, cs, "selterms-", N, p, K, 0, L.SEL, L.SEL | L.SELOP_TAGGED | L.sel_terms(T) | L.PICK_UNIFORM, rc[:p], rm[:p],
                        spec["ent"].reshape(T * K, p), None, draws, att_u, (masks[0], None, uniform_pick_blocks(masks[0], draws[:, 0], N)), n_sh=spec["shards"])


def run_selop_whole(e, cs, where, spec, lab, sel, N, P, K, rc, rm):
    """one more operator call over ALL P pods of a batch long enough for two pod tiles per block (spec["whole"]: the rows compared, against
    tests/selop_ref.py on those rows' entries), into a view at pitch W + 1 with sentinel words behind every row and behind the last one.
    -> the number of failures"""
    import torch
    dev = torch.device("cuda:0")
    rows, W = spec["whole"], (N + 63) // 64
    pitch = W + 1
    want = selop_ref.selop_mask(lab, np.ascontiguousarray(sel[:, rows]), spec["op"]) if K else selop_ref.selop_mask(np.zeros((0, N), np.uint32), None, spec["op"], p=rows.size)
    buf = torch.full(((P + GUARD_ROWS) * pitch,), SENTINEL, dtype=torch.int64, device=dev)
    view = buf.view(P + GUARD_ROWS, pitch)[:P, :W]
    td = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    e.eval_device(td(rc, np.int64), td(rm, np.int64), td(sel, np.int32) if K else None, None, None, L.SEL | spec["op"], out_feasible=view)
    ran = e.last_kernel
    torch.cuda.synchronize()
    body = buf.cpu().numpy().view(np.uint64).reshape(P + GUARD_ROWS, pitch)
    bad = 0
    if ran != "selop" or not np.array_equal(body[rows, :W], want) or not (body[:, W:] == SENTINEL).all() or not (body[P:] == SENTINEL).all():
        bad += 1
        print(f"FAIL operator call over the whole batch case seed {cs} {where}: N={N} P={P} K={K} flags={L.SEL | spec['op']:#x} kernel={ran} "
              f"({int((body[rows, :W] != want).any(axis=1).sum())} of {rows.size} compared rows differ)", flush=True)
    picks["selop"] = picks.get("selop", 0) + 1
    picks["selop-two-tiles"] = picks.get("selop-two-tiles", 0) + 1
    return bad


def selcall_halves(cs, spec, masks, N, K, rc, rm, sel, smp_u, att_u):
    """both calls through ksched_eval_begin / _end over spec's 1 to 5 row shards of the first p pods (shard_halves: the selector columns
    addressed inside the whole array, so sel_stride > p on every real shard), with the uniform pick so that the second half has bindings
    to hand back.  -> the number of failures"""
    p, want_op, want_tag = masks
    bad = 0
    for flags, entries, want in ((L.SEL | spec["op"], sel, want_op), (L.SEL | L.SELOP_TAGGED, spec["tsel"], want_tag)):
        ent = np.ascontiguousarray(entries[:, :p])
        draws = np.ascontiguousarray(smp_u[:p])
        bad += shard_halves(None, cs, "selop-", N, p, K, 0, L.SEL, flags | L.PICK_UNIFORM, rc[:p], rm[:p], ent, None, draws, att_u,
                            (want, None, uniform_pick_blocks(want, draws[:, 0], N)), n_sh=spec["shards"])
    return bad


def clique(n_sh):
    """the first n_sh replicas and their comms (ksched_comm_create_local), made on first use"""
    import ctypes as C
    while len(replicas) < n_sh:
        replicas.append(Evaluator(0))
    reps = replicas[:n_sh]
    if n_sh not in cliques:
        ctxs = (C.c_void_p * n_sh)(*[e._h for e in reps])
        comms = (C.c_void_p * n_sh)()
        rcode = ev._lib.ksched_comm_create_local(ctxs, n_sh, comms)
        if rcode != 0:
            raise L.KschedError(rcode, "ksched_comm_create_local", ev._lib.ksched_comm_last_error().decode())
        cliques[n_sh] = comms
    return reps, cliques[n_sh]


def sharded_apply(reps, comms, cut, bt, rct, rmt, okt, af, wait=True):
    """ksched_apply_bindings_sharded_local over `reps`: replica q applies rows [cut[q], cut[q + 1]) of the device tensors.  -> the
    statuses of all rows after a host wait; with wait=False the status tensors at once, the applies still in flight"""
    import ctypes as C
    import torch
    n_sh = len(reps)
    sts = [torch.full((cut[q + 1] - cut[q],), -7, dtype=torch.int32, device=bt.device) for q in range(n_sh)]
    ptrs = lambda xs: (C.c_void_p * n_sh)(*xs)  # noqa: E731
    part = lambda x, q, w: None if x is None or cut[q + 1] == cut[q] else x.data_ptr() + w * cut[q]  # noqa: E731
    rcode = ev._lib.ksched_apply_bindings_sharded_local(
        C.cast(ptrs([e._h for e in reps]), C.c_void_p), C.cast(comms, C.c_void_p), n_sh,
        C.cast((C.c_uint32 * n_sh)(*[cut[q + 1] - cut[q] for q in range(n_sh)]), C.c_void_p), C.cast((C.c_uint32 * n_sh)(*cut[:n_sh]), C.c_void_p),
        C.cast(ptrs([part(bt, q, 4) for q in range(n_sh)]), C.c_void_p), C.cast(ptrs([part(rct, q, 8) for q in range(n_sh)]), C.c_void_p),
        C.cast(ptrs([part(rmt, q, 8) for q in range(n_sh)]), C.c_void_p), C.cast(ptrs([part(okt, q, 1) for q in range(n_sh)]), C.c_void_p) if okt is not None else None,
        af, C.cast(ptrs([s_.data_ptr() if s_.numel() else None for s_ in sts]), C.c_void_p), None)
    if rcode != 0:
        raise L.KschedError(rcode, "ksched_apply_bindings_sharded_local", ev._lib.ksched_comm_last_error().decode())
    if not wait:
        return sts
    torch.cuda.synchronize()
    return np.concatenate([s_.cpu().numpy() for s_ in sts])


def apply_step(r, cs, cpu, mem, lab, taints, bindings, rc, rm, relabelled=False):
    """apply `bindings` (the previous evaluation's) on the device -- random flags, ok, now and then RELEASE; with the hooks, now and then
    also as a sharded apply over replicas with ragged cuts, every replica then equal to `ev` -- and advance cpu / mem (in place) by the
    exact-integer restatement.  -> the number of failures"""
    import ctypes as C
    import torch
    P, N = bindings.shape[0], cpu.shape[0]
    okv = np.where(r.random(P) < 0.15, 0, r.integers(1, 256, P)).astype(np.uint8) if r.random() < 0.5 else None
    af = int(r.choice([0, L.APPLY_FIRST_PER_NODE])) | (L.APPLY_RELEASE if r.random() < 0.2 else 0)
    # (a decision added after the sequence of `r` was fixed: its own generator, one per apply of the case)
    admit = np.random.default_rng([cs, 0xAD3, picks.get("apply", 0)]).random() < 0.25
    if admit:
        af = L.APPLY_WHILE_FIT
        ncpu, nmem, want_st = apply_while_fit_exact(cpu, mem, bindings, rc, rm, okv)
    else:
        ncpu, nmem, want_st = apply_bindings_exact(cpu, mem, bindings, rc, rm, okv, af)
    dev = torch.device("cuda:0")
    bt, rct, rmt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (bindings, rc, rm))
    okt = None if okv is None else torch.from_numpy(okv).to(dev)
    bad = 0
    if HOOKS and r.random() < 0.5:
        n_sh = int(r.choice([2, 3, 4]))
        reps, comms = clique(n_sh)
        for e in reps:
            e.set_nodes(cpu, mem, lab, taints)
        cut = [0] + sorted(int(x) for x in r.integers(0, P + 1, n_sh - 1)) + [P]
        if admit:  # the sharded entry point refuses the flag and leaves every replica as it was
            try:
                sharded_apply(reps, comms, cut, bt, rct, rmt, okt, af)
                refused = False
            except L.KschedError as e:
                refused = e.code == L.E_UNSUPPORTED
            if not (refused and all(np.array_equal(c_[0], cpu) and np.array_equal(c_[1], mem) for c_ in (e.read_nodes() for e in reps))):
                bad += 1
                print(f"FAIL sharded refusal of APPLY_WHILE_FIT case seed {cs}: N={N} P={P} cuts={cut}", flush=True)
            picks["while-fit-refused-sharded"] = picks.get("while-fit-refused-sharded", 0) + 1
            reps = []
        st_sh = sharded_apply(reps, comms, cut, bt, rct, rmt, okt, af) if reps else None
        cols = [e.read_nodes() for e in reps]
        if reps and not (np.array_equal(st_sh, want_st) and all(np.array_equal(c_[0], ncpu) and np.array_equal(c_[1], nmem) for c_ in cols)):
            bad += 1
            print(f"FAIL sharded apply case seed {cs}: N={N} P={P} flags={af} ok={okv is not None} cuts={cut}", flush=True)
        if reps:
            picks[f"sharded-apply-over-{n_sh}"] = picks.get(f"sharded-apply-over-{n_sh}", 0) + 1
    else:
        reps = []
    st = torch.full((P,), -7, dtype=torch.int32, device=dev)
    ev.apply_bindings_device(bt, rct, rmt, okt, af, st)
    torch.cuda.synchronize()
    got = ev.read_nodes()
    if not (np.array_equal(st.cpu().numpy(), want_st) and np.array_equal(got[0], ncpu) and np.array_equal(got[1], nmem)):
        bad += 1
        print(f"FAIL apply case seed {cs}: N={N} P={P} flags={af} ok={okv is not None}", flush=True)
    # the replicas were set afresh; `ev` after ksched_update_node_labels keeps a layout planned for the union of the old and the new maxima
    # (include/ksched.h), so its index is comparable with theirs only while its labels are the ones it was set with -- else the replicas among themselves
    if reps and any(e.index_checksum() != (reps[0] if relabelled else ev).index_checksum() for e in reps):
        bad += 1
        print(f"FAIL sharded apply index case seed {cs}: N={N} P={P} flags={af} replicas={len(reps)}", flush=True)
    picks["apply"] = picks.get("apply", 0) + 1
    if admit:
        picks["apply-while-fit"] = picks.get("apply-while-fit", 0) + 1
        if (want_st == L.APPLY_DEFERRED).any():
            picks["apply-while-fit-deferred"] = picks.get("apply-while-fit-deferred", 0) + 1
    cpu[:], mem[:] = ncpu, nmem
    return bad


def row_popcounts(m):
    """set bits per mask row"""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(m).sum(axis=1)
    return np.unpackbits(np.ascontiguousarray(m).view(np.uint8), axis=1).sum(axis=1)


def shard_halves(g, cs, tag, N, P, K, nt, preds, flags, rc, rm, sel, tol, smp, attempts, want, n_sh=None):
    """the host-side row shard (include/ksched.h "one host thread, several devices"): the batch cut into 1 .. 5 shards with
    ksched_shard_bounds, every shard through ksched_eval_begin (selector columns addressed inside the whole batch's array with its
    stride, the draws `smp` [P, attempts] at 4 * attempts * lo bytes, bindings padded to ceil(P / n) with -1) + ksched_eval_end, merged
    like an all-gathered table -- on this one evaluator, shard after shard.  `g` draws the shard count (n_sh given: that many, and `g` is
    not asked).  -> the number of failures"""
    bad = 0
    import ctypes as C
    n_sh = int(g.choice([1, 2, 3, 5])) if n_sh is None else n_sh
    W = ev.W
    lo_, hi_, cpr_ = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc_c, rm_c = np.ascontiguousarray(rc), np.ascontiguousarray(rm)
    sel_c = np.ascontiguousarray(sel) if K else None
    tol_c = np.ascontiguousarray(tol) if (preds & L.TAINT) else None
    smp_c = np.ascontiguousarray(smp) if smp is not None else None
    feas_s = np.zeros((P, W), dtype=np.uint64)
    fit_s = np.zeros((P, W), dtype=np.uint64)
    bind_s = np.full((P,), 777, dtype=np.int32)
    for rank in range(n_sh):
        ev._lib.ksched_shard_bounds(P, n_sh, rank, C.byref(lo_), C.byref(hi_), C.byref(cpr_))
        lo, hi, cpr = lo_.value, hi_.value, cpr_.value
        dev_b, stream = C.c_void_p(), C.c_void_p()
        rcode = ev._lib.ksched_eval_begin(
            ev._h, hi - lo, C.c_void_p(rc_c.ctypes.data + 8 * lo), C.c_void_p(rm_c.ctypes.data + 8 * lo),
            C.c_void_p(sel_c.ctypes.data + 4 * lo) if K else None, P, C.c_void_p(tol_c.ctypes.data + 8 * lo) if tol_c is not None else None,
            C.c_void_p(smp_c.ctypes.data + 4 * attempts * lo) if smp_c is not None else None, attempts, flags,
            C.c_void_p(feas_s.ctypes.data + 8 * W * lo), C.c_void_p(fit_s.ctypes.data + 8 * W * lo) if flags & L.WANT_FIT_MASK else None, cpr,
            C.byref(dev_b), C.byref(stream))
        if rcode != 0:
            raise L.KschedError(rcode, "ksched_eval_begin", ev._lib.ksched_last_error(ev._h).decode())
        part = np.full((cpr,), 555, dtype=np.int32)
        rcode = ev._lib.ksched_eval_end(ev._h, dev_b, cpr, part.ctypes.data_as(C.c_void_p))
        if rcode != 0:
            raise L.KschedError(rcode, "ksched_eval_end", ev._lib.ksched_last_error(ev._h).decode())
        bind_s[lo:hi] = part[:hi - lo]
        if not (part[hi - lo:] == -1).all():
            bad += 1
            print(f"FAIL {tag}shard padding case seed {cs}: P={P} shards={n_sh} rank={rank}", flush=True)
    if not (np.array_equal(feas_s, want[0]) and (not (flags & L.WANT_FIT_MASK) or np.array_equal(fit_s, want[1])) and np.array_equal(bind_s, want[2])):
        bad += 1
        print(f"FAIL {tag}sharded halves case seed {cs}: N={N} P={P} K={K} nt={nt} flags={flags:#x} attempts={attempts} shards={n_sh}", flush=True)
    picks[tag + "sharded-halves"] = picks.get(tag + "sharded-halves", 0) + 1
    return bad


def gathered_sequence(g, cs, tag, cpu, mem, lab, taints, N, P, K, nt, preds, flags, rc, rm, sel, tol, smp, attempts, want, n_sh=None):
    """the whole multi-device sequence over 2 .. 4 replicas on the one GPU (test hooks): ksched_eval_begin on every replica,
    ksched_gather_buffer, ksched_allgather_bindings_local, ksched_eval_end(gathered_0).  `g` draws the replica count and the replicas'
    options.  With n_sh given, that many replicas evaluate on the snapshots they hold (nothing is drawn, nothing set: the columns are what
    the calls before left on each).  -> (the number of failures, the last_pick names of the replicas whose shard held a pod)"""
    bad = 0
    ran = []
    import ctypes as C
    keep = n_sh is not None
    n_sh = n_sh if keep else int(g.choice([2, 3, 4]))
    reps, comms = clique(n_sh)
    lib = ev._lib
    for e in ([] if keep else reps):  # the snapshot is replicated (the current values: the updates above are in cpu / mem)
        e.set_option(L.OPT_BESTFIT_STAGES, int(g.choice([0, 1, 2])))
        e.set_nodes(cpu, mem, lab, taints)
    W = ev.W
    lo_, hi_, cpr_ = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc_c, rm_c = np.ascontiguousarray(rc), np.ascontiguousarray(rm)
    sel_c = np.ascontiguousarray(sel) if K else None
    tol_c = np.ascontiguousarray(tol) if (preds & L.TAINT) else None
    smp_c = np.ascontiguousarray(smp) if smp is not None else None
    feas_s, fit_s = np.zeros((P, W), dtype=np.uint64), np.zeros((P, W), dtype=np.uint64)
    local, gathered, streams = (C.c_void_p * n_sh)(), (C.c_void_p * n_sh)(), (C.c_void_p * n_sh)()
    lib.ksched_shard_bounds(P, n_sh, 0, C.byref(lo_), C.byref(hi_), C.byref(cpr_))
    cpr = cpr_.value
    for rank, e in enumerate(reps):
        lib.ksched_shard_bounds(P, n_sh, rank, C.byref(lo_), C.byref(hi_), C.byref(cpr_))
        lo, hi = lo_.value, hi_.value
        dev_b, stream = C.c_void_p(), C.c_void_p()
        rcode = lib.ksched_eval_begin(
            e._h, hi - lo, C.c_void_p(rc_c.ctypes.data + 8 * lo), C.c_void_p(rm_c.ctypes.data + 8 * lo),
            C.c_void_p(sel_c.ctypes.data + 4 * lo) if K else None, P, C.c_void_p(tol_c.ctypes.data + 8 * lo) if tol_c is not None else None,
            C.c_void_p(smp_c.ctypes.data + 4 * attempts * lo) if smp_c is not None else None, attempts, flags,
            C.c_void_p(feas_s.ctypes.data + 8 * W * lo), C.c_void_p(fit_s.ctypes.data + 8 * W * lo) if flags & L.WANT_FIT_MASK else None, cpr,
            C.byref(dev_b), C.byref(stream))
        if rcode != 0:
            raise L.KschedError(rcode, "ksched_eval_begin", lib.ksched_last_error(e._h).decode())
        local[rank], streams[rank] = dev_b.value, stream.value
        if hi > lo:
            ran.append(e)
        gbuf = C.c_void_p()
        rcode = lib.ksched_gather_buffer(e._h, n_sh * cpr, C.byref(gbuf))
        if rcode != 0:
            raise L.KschedError(rcode, "ksched_gather_buffer", lib.ksched_last_error(e._h).decode())
        gathered[rank] = gbuf.value
    rcode = lib.ksched_allgather_bindings_local(comms, n_sh, local, gathered, cpr, streams)
    if rcode != 0:
        raise L.KschedError(rcode, "ksched_allgather_bindings_local", lib.ksched_comm_last_error().decode())
    table = np.full((n_sh * cpr,), 555, dtype=np.int32)
    for rank, e in enumerate(reps):
        rcode = lib.ksched_eval_end(e._h, C.c_void_p(gathered[0]) if rank == 0 else None, n_sh * cpr if rank == 0 else 0,
                                    table.ctypes.data_as(C.c_void_p) if rank == 0 else None)
        if rcode != 0:
            raise L.KschedError(rcode, "ksched_eval_end", lib.ksched_last_error(e._h).decode())
    bind_s = np.full((P,), 777, dtype=np.int32)
    pad_ok = True
    for rank in range(n_sh):
        lib.ksched_shard_bounds(P, n_sh, rank, C.byref(lo_), C.byref(hi_), C.byref(cpr_))
        bind_s[lo_.value:hi_.value] = table[rank * cpr: rank * cpr + hi_.value - lo_.value]
        pad_ok = pad_ok and bool((table[rank * cpr + hi_.value - lo_.value: (rank + 1) * cpr] == -1).all())
    if not (pad_ok and np.array_equal(feas_s, want[0]) and (not (flags & L.WANT_FIT_MASK) or np.array_equal(fit_s, want[1])) and np.array_equal(bind_s, want[2])):
        bad += 1
        print(f"FAIL {tag}multi-device sequence case seed {cs}: N={N} P={P} K={K} nt={nt} flags={flags:#x} attempts={attempts} replicas={n_sh}{' (on the snapshots the replicas held)' if keep else ''}", flush=True)
    picks[f"{tag}gathered-over-{n_sh}"] = picks.get(f"{tag}gathered-over-{n_sh}", 0) + 1
    return bad, {e.last_pick for e in ran}


def spread_gathered(g, cs, cpu, mem, lab, taints, N, P, K, nt, preds, flags, rc, rm, sel, tol, smp, d, want, ranked, tied,
                    name="spread", restate=None, chain=None, after=None, after_terms=False):
    """the multi-device sequence with the spread pick, twice: on freshly set replicas; then -- after ksched_apply_bindings_sharded_local of
    the gathered bindings over the same replicas, ragged cuts, no ksched_set_nodes -- on the columns that apply left on every replica: the
    oracle's mask and the restatement on the exact-integer apply of those bindings.  A replica whose columns the gathered commit left behind
    ranks its rows by old values.  Every replica's pick must run as "spread".  `ev`, cpu and mem are not touched.  -> the number of failures.
    name="pack", restate=pack_restated: the same for the pack pick (flags carry PICK_PACK).  chain=(spec, smp, smp_u, smp_s): after the
    sharded apply and the second sequence that combining chain runs on every replica, against the columns the apply left; behind it
    after(e, where, ncpu, nmem) -> failures: the step's operator and tagged calls on that replica, on the same columns (after_terms: the
    step's terms call is among them, tallied as 'selterms-on-replicas')."""
    import torch
    restate = restate or spread_restated
    tag, pick_flag = name + "-", {"spread": L.PICK_SPREAD, "pack": L.PICK_PACK}[name]
    n_sh = int(g.choice([2, 3, 4]))
    for e in clique(n_sh)[0]:
        e.set_nodes(cpu, mem, lab, taints)
    bad, names = gathered_sequence(g, cs, tag, cpu, mem, lab, taints, N, P, K, nt, preds, flags, rc, rm, sel, tol, smp, d, want, n_sh=n_sh)
    tally = [(names, ranked, tied)]
    af = int(g.choice([0, L.APPLY_FIRST_PER_NODE])) | (L.APPLY_RELEASE if g.random() < 0.2 else 0)
    ncpu, nmem, want_st = apply_bindings_exact(cpu, mem, want[2], rc, rm, None, af)
    reps, comms = clique(n_sh)
    dev = torch.device("cuda:0")
    bt, rct, rmt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (want[2], rc, rm))
    cut = [0] + sorted(int(x) for x in g.integers(0, P + 1, n_sh - 1)) + [P]
    sts = sharded_apply(reps, comms, cut, bt, rct, rmt, None, af, wait=False)  # no host wait before the replicas evaluate again
    picks[f"{tag}gathered-apply-over-{n_sh}"] = picks.get(f"{tag}gathered-apply-over-{n_sh}", 0) + 1
    want2 = capi.eval_encoded(ncpu, nmem, lab, taints if (preds & L.TAINT) else None, rc, rm, sel, tol if (preds & L.TAINT) else None, None, flags & ~pick_flag)
    b2, ranked2, tied2 = restate(want2[0], smp, N, nmem, ncpu)
    bad2, names2 = gathered_sequence(g, cs, tag, ncpu, nmem, lab, taints, N, P, K, nt, preds, flags, rc, rm, sel, tol, smp, d, (want2[0], want2[1], b2), n_sh=n_sh)
    tally.append((names2, ranked2, tied2))
    torch.cuda.synchronize()
    if not np.array_equal(np.concatenate([s_.cpu().numpy() for s_ in sts]), want_st):
        bad += 1
        print(f"FAIL {name} gathered apply case seed {cs}: N={N} P={P} flags={af} cuts={cut}: statuses", flush=True)
    if not np.array_equal(b2, restate(want2[0], smp, N, mem, cpu)[0]):  # (the old columns would show)
        picks[f"{tag}gathered-moved"] = picks.get(f"{tag}gathered-moved", 0) + 1
    for nm, rk, td in tally:
        if nm == {name}:
            picks[name] = picks.get(name, 0) + len(nm)
            picks[f"{tag}ranked"] = picks.get(f"{tag}ranked", 0) + int(rk) * len(nm)
            if name == "spread":
                picks["spread-tied"] = picks.get("spread-tied", 0) + int(td) * len(nm)
        else:
            bad += 1
            print(f"FAIL {name} multi-device sequence case seed {cs}: N={N} P={P} d={d}: the replicas' picks ran as {sorted(nm)}", flush=True)
    if chain is not None:  # the step's combining chain on every replica, on the columns the sharded apply left there
        for q, e in enumerate(reps):
            bad += run_chain(e, cs, f"replica {q} of {n_sh} after a sharded apply", chain[0], ncpu, nmem, lab, taints, N, P, K, nt, rc, rm, sel, tol, *chain[1:])
            if after is not None:
                bad += after(e, f"replica {q} of {n_sh} after a sharded apply", ncpu, nmem)
        picks["combine-on-replicas"] = picks.get("combine-on-replicas", 0) + 1
        if after is not None:
            picks["selop-on-replicas"] = picks.get("selop-on-replicas", 0) + 1
            if after_terms:
                picks["selterms-on-replicas"] = picks.get("selterms-on-replicas", 0) + 1
    return bad + bad2


t_end = time.time() + budget
cases = fails = 0
picks = {}
I64 = np.iinfo(np.int64)
while time.time() < t_end:
    cases += 1
    cs = int(rng.integers(0, 1 << 31))
    r = np.random.default_rng(cs)
    r2 = np.random.default_rng([cs, 0x0E3])  # every decision added after the sequence of `r` was fixed (see the docstring)
    r3 = np.random.default_rng([cs, 0x5E4])  # every decision added after the sequence of `r2` was fixed: the spread legs
    r4 = np.random.default_rng([cs, 0xC0B])  # every decision added after the sequence of `r3` was fixed: the pack legs and the combining chains
    r5 = np.random.default_rng([cs, 0xE95])  # every decision added after the sequence of `r4` was fixed: the operator and the tagged selector calls
    r6 = np.random.default_rng([cs, 0xE10])  # every decision added after the sequence of `r5` was fixed: the terms call
    wide = int(r2.choice([8192, 8193, 12_500])) if r2.random() < 0.1 else 0  # rows of more than 128 words: k_pick_uniform's two-pass form (8192: the longest one-pass row)
    N = int(r.choice([1, 2, 63, 64, 65, 300, 1023, 1024, 1025, 2500, 4097, 6000]))
    P = int(r.choice([1, 7, 64, 65, 500, 1500, 3000]))
    N = wide or N
    if r.random() < 0.05:  # now and then a batch long enough for two or more rounds per wave of a whole-chip launch (run_fused's chunk-count rule, the riding pick's longer forms)
        P = int(r.choice([12_000, 20_011, 40_000, 52_225]))
    if wide:
        P = min(P, 1500)  # the oracle's time
    K = int(r.choice([0, 1, 3, 8, 9, 12]))
    cards = [int(r.choice([1, 2, 5, 40, 300, N, 4 * N + 7])) for _ in range(K)]
    scale = int(r.choice([10, 1000, 1 << 20]))
    cpu = r.integers(-scale, 64 * scale, N).astype(np.int64)
    mem = r.integers(-scale, 64 * scale, N).astype(np.int64)
    if r.random() < 0.1:
        cpu[r.integers(0, N, 3)] = r.choice([I64.min, I64.max, 0])
    lab = np.stack([r.integers(0, c + 1, N).astype(np.uint32) for c in cards]) if K else None
    nt = int(r.choice([0, 0, 3, 16, 60]))
    taints = (r.integers(0, 1 << nt, N).astype(np.uint64) & r.integers(0, 1 << nt, N).astype(np.uint64)) if nt else None
    rc = r.integers(-5, 70 * scale, P).astype(np.int64)
    rm = r.integers(-5, 70 * scale, P).astype(np.int64)
    pk = float(r.choice([0.05, 0.3, 0.9]))
    sel = np.stack([np.where(r.random(P) < pk, r.integers(1, c + 3, P), 0).astype(np.uint32) for c in cards]) if K else None
    if K and r.random() < 0.5:
        sel[r.integers(0, K), r.integers(0, P, max(1, P // 20))] = L.SEL_NEVER
    tol = r.integers(0, 1 << nt, P).astype(np.uint64) if nt else None
    smp = r.integers(0, N + (2 if r.random() < 0.2 else 0), (P, 5)).astype(np.uint32)
    preds = int(r.choice([L.FIT, L.FIT | L.SEL, L.FIT | L.SEL | L.TAINT, L.SEL, L.SEL | L.TAINT, L.FIT | L.TAINT]))
    if not K:
        preds &= ~L.SEL
    if not nt:
        preds &= ~L.TAINT
    if preds == 0:
        preds = L.FIT
    pick = int(r.choice([0, L.PICK_SAMPLED, L.PICK_BESTFIT]))
    flags = preds | pick | (L.WANT_FIT_MASK if r.random() < 0.5 else 0)
    # the uniform pick's draws: full-range 32-bit, column 0 (the one that is read) now and then all zero or all ones
    att_u = int(r2.choice([1, 3, 5]))
    smp_u = r2.integers(0, 1 << 32, (P, att_u), dtype=np.uint64).astype(np.uint32)
    if r2.random() < 0.15:
        smp_u[:, int(r2.integers(0, att_u))] = 0 if r2.random() < 0.5 else 0xFFFFFFFF
    if r2.random() < 0.1:
        smp_u[:, 0] = 0 if r2.random() < 0.5 else 0xFFFFFFFF
    # the spread pick's draws: full-range 32-bit, 64 columns of which a step reads the first d; now and then a column all zero or all ones
    smp_s64 = r3.integers(0, 1 << 32, (P, 64), dtype=np.uint64).astype(np.uint32)
    if r3.random() < 0.15:
        smp_s64[:, int(r3.integers(0, 8))] = 0 if r3.random() < 0.5 else 0xFFFFFFFF
    try:
        ev.set_option(L.OPT_BESTFIT_STAGES, int(r.choice([0, 1, 2])))
        ev.set_option(L.OPT_GRID_CUS, int(r.choice([0, 0, 0, 8, 17, 96, 200])))  # fewer compute units per launch: same results
        ev.set_option(L.OPT_ROUND_ORDER, int(r.choice([0, 0, 1, 2])))  # which wave takes which round: same results
        ev.set_option(L.OPT_FUSED_PICK, int(r.choice([0, 1, 1, 2])))  # 3 (tile tests or E_UNSUPPORTED) below, where it applies
        ev.set_nodes(cpu, mem, lab, taints)
        last_b, relabelled = None, False
        for step in range(int(r.choice([1, 2, 3]))):
            if step and last_b is not None and r.random() < 0.6:  # the previous evaluation's bindings applied on the device
                fails += apply_step(r, cs, cpu, mem, lab, taints, last_b, rc, rm, relabelled)
            elif step:  # a snapshot update between evaluations
                idx = r.integers(0, N, int(r.choice([1, 5, 40, N]))).astype(np.uint32)
                nc, nm = r.integers(-scale, 64 * scale, idx.size).astype(np.int64), r.integers(-scale, 64 * scale, idx.size).astype(np.int64)
                if (K or nt) and r2.random() < 0.5:  # instead: the labels (and taints) of random rows change
                    lidx = r2.integers(0, N, int(r2.choice([1, 5, 40, N]))).astype(np.uint32)
                    lmax = lab.max(axis=1).astype(np.int64) if K else None
                    rows_t = None
                    if r2.random() < 2 / 3:  # ids within each key's current maximum, taint bits within the highest one
                        rows = r2.integers(0, lmax[:, None] + 1, (K, lidx.size)).astype(np.uint32) if K else None
                        if nt and (not K or r2.random() < 0.5):  # (without label keys the taints are all the call can change)
                            rows_t = r2.integers(0, 1 << nt, lidx.size, dtype=np.uint64) & r2.integers(0, 1 << nt, lidx.size, dtype=np.uint64)
                    else:  # ids above a key's maximum (the layout is planned again), some pods selecting them; now and then a taint bit above the others
                        rows = np.ascontiguousarray(lab[:, lidx]) if K else None
                        if K:
                            key = int(r2.integers(0, K))
                            rows[key, : max(1, lidx.size // 2)] = lmax[key] + 1 + r2.integers(0, 3, max(1, lidx.size // 2))
                            sel[key, r2.integers(0, P, max(1, P // 10))] = lmax[key] + 1
                        if nt and (not K or r2.random() < 0.3):
                            top = np.uint64(1) << np.uint64(min(nt, 63))
                            rows_t = taints[lidx] | top
                            tol[r2.integers(0, P, max(1, P // 2))] |= top
                    ev.update_node_labels(lidx, rows, rows_t)
                    lab, taints = apply_rows(lab, taints, lidx, rows, rows_t)
                    lab = None if lab is None else np.ascontiguousarray(lab)
                    picks["labels"] = picks.get("labels", 0) + 1
                    relabelled = True
                else:
                    ev.update_nodes(idx, nc, nm)
                    for j in range(idx.size):
                        cpu[idx[j]], mem[idx[j]] = nc[j], nm[j]
            want = capi.eval_encoded(cpu, mem, lab, taints if (preds & L.TAINT) else None, rc, rm, sel, tol if (preds & L.TAINT) else None, smp, flags)
            for kernel in ("auto", "direct"):
                ev.set_kernel(kernel)
                got = ev.eval(rc, rm, sel if K else None, tol if (preds & L.TAINT) else None, smp if pick == L.PICK_SAMPLED else None, flags)
                ok = np.array_equal(got.feasible, want[0]) and (not (flags & L.WANT_FIT_MASK) or np.array_equal(got.fit, want[1])) and \
                    (not pick or np.array_equal(got.binding, want[2]))
                if not ok:
                    fails += 1
                    print(f"FAIL case seed {cs}: N={N} P={P} K={K} cards={cards} nt={nt} flags={flags:#x} kernel={kernel}/{ev.last_kernel} pick={ev.last_pick} step={step}", flush=True)
                picks[ev.last_pick] = picks.get(ev.last_pick, 0) + 1
                if pick:
                    last_b = got.binding.copy()
            if pick == L.PICK_SAMPLED and K <= 8 and not (preds & L.TAINT):  # the tile-test form of the riding pick, forced
                ev.set_kernel("fused")
                ev.set_option(L.OPT_FUSED_PICK, 3)
                try:
                    got = ev.eval(rc, rm, sel if K else None, None, smp, flags)
                    if not (np.array_equal(got.feasible, want[0]) and np.array_equal(got.binding, want[2])):
                        fails += 1
                        print(f"FAIL tile pick case seed {cs}: N={N} P={P} K={K} cards={cards} flags={flags:#x} pick={ev.last_pick} step={step}", flush=True)
                    picks[ev.last_pick] = picks.get(ev.last_pick, 0) + 1
                except L.KschedError as e:
                    if e.code != L.E_UNSUPPORTED:
                        raise
                    picks["tile-unsupported"] = picks.get("tile-unsupported", 0) + 1
                ev.set_option(L.OPT_FUSED_PICK, 1)
            # the uniform pick on the same snapshot: both kernels, with and without the mask, now and then with the fit mask (where the
            # oracle computed one) -- against the restatement on the oracle's mask
            want_u = uniform_pick_blocks(want[0], smp_u[:, 0], N)
            ranked = bool((row_popcounts(want[0]) >= 2).any())
            fl_u = preds | L.PICK_UNIFORM | (L.WANT_FIT_MASK if (flags & L.WANT_FIT_MASK) and r2.random() < 0.5 else 0)
            for kernel in ("auto", "direct"):
                ev.set_kernel(kernel)
                for want_mask in (True, False):
                    fl = fl_u if want_mask else fl_u & ~L.WANT_FIT_MASK
                    got = ev.eval(rc, rm, sel if K else None, tol if (preds & L.TAINT) else None, smp_u, fl, want_mask=want_mask)
                    ok = (not want_mask or np.array_equal(got.feasible, want[0])) and np.array_equal(got.binding, want_u) and \
                        (not (fl & L.WANT_FIT_MASK) or np.array_equal(got.fit, want[1]))
                    if not ok:
                        fails += 1
                        print(f"FAIL uniform case seed {cs}: N={N} P={P} K={K} cards={cards} nt={nt} flags={fl_u:#x} kernel={kernel}/{ev.last_kernel} pick={ev.last_pick} mask={want_mask} step={step}", flush=True)
                    if ev.last_pick == "uniform":
                        picks["uniform"] = picks.get("uniform", 0) + 1
                        picks["uniform-ranked"] = picks.get("uniform-ranked", 0) + int(ranked)
                    else:  # a KSCHED_PICK_UNIFORM request has one launch form
                        fails += 1
                        print(f"FAIL uniform case seed {cs}: N={N} P={P} K={K} flags={fl_u:#x} kernel={kernel} mask={want_mask} step={step}: the pick ran as {ev.last_pick!r}", flush=True)
            # the spread pick on the same snapshot, d drawn anew at every step: both kernels, with and without the mask -- against the
            # restatement on the oracle's mask and on cpu / mem as the updates and applies above left them
            d_s = int(r3.choice([1, 2, 3, 5, 8, 33, 64]))
            smp_s = np.ascontiguousarray(smp_s64[:, :d_s])
            want_s, ranked_s, tied_s = spread_restated(want[0], smp_s, N, mem, cpu)
            fl_s = preds | L.PICK_SPREAD | (L.WANT_FIT_MASK if (flags & L.WANT_FIT_MASK) and r3.random() < 0.5 else 0)
            for kernel in ("auto", "direct"):
                ev.set_kernel(kernel)
                for want_mask in (True, False):
                    fl = fl_s if want_mask else fl_s & ~L.WANT_FIT_MASK
                    got = ev.eval(rc, rm, sel if K else None, tol if (preds & L.TAINT) else None, smp_s, fl, want_mask=want_mask)
                    ok = (not want_mask or np.array_equal(got.feasible, want[0])) and np.array_equal(got.binding, want_s) and \
                        (not (fl & L.WANT_FIT_MASK) or np.array_equal(got.fit, want[1]))
                    if not ok:
                        fails += 1
                        print(f"FAIL spread case seed {cs}: N={N} P={P} K={K} cards={cards} nt={nt} flags={fl_s:#x} d={d_s} kernel={kernel}/{ev.last_kernel} pick={ev.last_pick} mask={want_mask} step={step}"
                              f" ({int((got.binding != want_s).sum())} bindings differ)", flush=True)
                    if ev.last_pick == "spread":
                        picks["spread"] = picks.get("spread", 0) + 1
                        picks["spread-ranked"] = picks.get("spread-ranked", 0) + int(ranked_s)
                        picks["spread-tied"] = picks.get("spread-tied", 0) + int(tied_s)
                    else:  # a KSCHED_PICK_SPREAD request has one launch form
                        fails += 1
                        print(f"FAIL spread case seed {cs}: N={N} P={P} K={K} flags={fl_s:#x} d={d_s} kernel={kernel} mask={want_mask} step={step}: the pick ran as {ev.last_pick!r}", flush=True)
            # the pack pick on the same snapshot and the same table of draws, d drawn anew from the spread pick's list: both kernels, with and
            # without the mask -- against tests/pack_ref.py on the oracle's mask and on cpu / mem as the updates and applies above left them
            d_k = int(r4.choice([1, 2, 3, 5, 8, 33, 64]))
            smp_k = np.ascontiguousarray(smp_s64[:, :d_k])
            want_k, ranked_k, _ = pack_restated(want[0], smp_k, N, mem, cpu)
            fl_k = preds | L.PICK_PACK
            for kernel in ("auto", "direct"):
                ev.set_kernel(kernel)
                for want_mask in (True, False):
                    got = ev.eval(rc, rm, sel if K else None, tol if (preds & L.TAINT) else None, smp_k, fl_k, want_mask=want_mask)
                    if not ((not want_mask or np.array_equal(got.feasible, want[0])) and np.array_equal(got.binding, want_k)):
                        fails += 1
                        print(f"FAIL pack case seed {cs}: N={N} P={P} K={K} cards={cards} nt={nt} flags={fl_k:#x} d={d_k} kernel={kernel}/{ev.last_kernel} pick={ev.last_pick} mask={want_mask} step={step}"
                              f" ({int((got.binding != want_k).sum())} bindings differ)", flush=True)
                    if ev.last_pick == "pack":
                        picks["pack"] = picks.get("pack", 0) + 1
                        picks["pack-ranked"] = picks.get("pack-ranked", 0) + int(ranked_k)
                    else:  # a KSCHED_PICK_PACK request has one launch form
                        fails += 1
                        print(f"FAIL pack case seed {cs}: N={N} P={P} K={K} flags={fl_k:#x} d={d_k} kernel={kernel} mask={want_mask} step={step}: the pick ran as {ev.last_pick!r}", flush=True)
            # one combining chain on the same snapshot (draw_chain, run_chain)
            chain = draw_chain(r4, N, P, K, nt)
            fails += run_chain(ev, cs, f"step {step}", chain, cpu, mem, lab, taints, N, P, K, nt, rc, rm, sel, tol, smp, smp_u, smp_s)
            # one operator call and one tagged call on the same snapshot (draw_selcalls, run_selcalls), on the labels as the updates above left
            # them; and both through the two halves of ksched_eval over row shards
            selc = draw_selcalls(r5, lab, N, P, K)
            selm = selcall_masks(selc, lab, sel, N, P, K)
            fails += run_selcalls(ev, cs, f"step {step}", selc, selm, chain["final"], cpu, mem, N, P, K, rc, rm, sel, smp, smp_u, smp_s)
            if K:
                fails += selcall_halves(cs, selc, selm, N, K, rc, rm, sel, smp_u, att_u)
            if selc["whole"] is not None:
                fails += run_selop_whole(ev, cs, f"step {step}", selc, lab, sel, N, P, K, rc, rm)
            # the terms call on the same snapshot and labels (draw_selterms, run_selterms): bare, under a drawn combine with a drawn pick, and
            # through the two halves over row shards
            selt = draw_selterms(r6, lab, N, P, K)
            if selt is not None:
                seltm = selterms_masks(selt, lab, N)
                fails += run_selterms(ev, cs, f"step {step}", selt, seltm, chain["final"], cpu, mem, N, P, K, rc, rm, smp, smp_u, smp_s)
                fails += selterms_halves(cs, selt, seltm, N, K, rc, rm, smp_u, att_u)
        ev.set_kernel("auto")
        want3_u = (want[0], want[1], want_u)
        want3_s = (want[0], want[1], want_s)
        if r3.random() < 0.4:  # ksched_pick with the spread pick: the oracle's mask, and that mask thinned by random words -- the restatement on either, on the current columns
            thin_s = want[0] & r3.integers(0, 1 << 63, want[0].shape, dtype=np.uint64)
            if not (np.array_equal(ev.pick(want[0], L.PICK_SPREAD, samples=smp_s), want_s) and
                    np.array_equal(ev.pick(thin_s, L.PICK_SPREAD, samples=smp_s), spread_restated(thin_s, smp_s, N, mem, cpu)[0])):
                fails += 1
                print(f"FAIL spread ksched_pick case seed {cs}: N={N} P={P} K={K} nt={nt} preds={preds:#x} d={d_s} step={step}", flush=True)
            picks["spread-host-masks"] = picks.get("spread-host-masks", 0) + 1
        if r3.random() < 0.35:
            fails += shard_halves(r3, cs, "spread-", N, P, K, nt, preds, fl_s, rc, rm, sel, tol, smp_s, d_s, want3_s)
        if HOOKS and r3.random() < 0.35:
            fails += spread_gathered(r3, cs, cpu, mem, lab, taints, N, P, K, nt, preds, fl_s, rc, rm, sel, tol, smp_s, d_s, want3_s, ranked_s, tied_s)
        if HOOKS and r4.random() < 0.5:  # the pack pick through the multi-device sequence and a sharded apply of its gathered bindings; then the chain on every replica
            fails += spread_gathered(r4, cs, cpu, mem, lab, taints, N, P, K, nt, preds, fl_k, rc, rm, sel, tol, smp_k, d_k, (want[0], want[1], want_k), ranked_k, False,
                                     name="pack", restate=pack_restated, chain=(chain, smp, smp_u, smp_s),
                                     after=lambda e, where, ncpu, nmem: run_selcalls(e, cs, where, selc, selm, chain["final"], ncpu, nmem, N, P, K, rc, rm, sel,
                                                                                     smp, smp_u, smp_s, tally=False) +
                                     (run_selterms(e, cs, where, selt, seltm, chain["final"], ncpu, nmem, N, P, K, rc, rm, smp, smp_u, smp_s, tally=False)
                                      if selt is not None else 0), after_terms=selt is not None)
        if r2.random() < 0.4:  # ksched_pick with the uniform pick: the oracle's mask, and that mask thinned by random words -- the restatement on either
            thin_u = want[0] & r2.integers(0, 1 << 63, want[0].shape, dtype=np.uint64)
            if not (np.array_equal(ev.pick(want[0], L.PICK_UNIFORM, samples=smp_u), want_u) and
                    np.array_equal(ev.pick(thin_u, L.PICK_UNIFORM, samples=smp_u), uniform_pick_blocks(thin_u, smp_u[:, 0], N))):
                fails += 1
                print(f"FAIL uniform ksched_pick case seed {cs}: N={N} P={P} K={K} nt={nt} preds={preds:#x}", flush=True)
            picks["uniform-host-masks"] = picks.get("uniform-host-masks", 0) + 1
        if r2.random() < 0.35:
            fails += shard_halves(r2, cs, "uniform-", N, P, K, nt, preds, fl_u, rc, rm, sel, tol, smp_u, att_u, want3_u)
        if HOOKS and r2.random() < 0.35:
            bad_u, names = gathered_sequence(r2, cs, "uniform-", cpu, mem, lab, taints, N, P, K, nt, preds, fl_u, rc, rm, sel, tol, smp_u, att_u, want3_u)
            fails += bad_u
            if names == {"uniform"}:
                picks["uniform"] = picks.get("uniform", 0) + 1
                picks["uniform-ranked"] = picks.get("uniform-ranked", 0) + int(ranked)
            else:
                fails += 1
                print(f"FAIL uniform multi-device sequence case seed {cs}: the replicas' picks ran as {sorted(names)}", flush=True)
        if pick and r.random() < 0.4:
            # the pick alone from HOST masks (ksched_pick, what a selector evaluated in key groups uses): from the oracle's mask it is the oracle's
            # binding; from that mask thinned by random words (an AND with another group's mask) the sampled pick is the first draw whose bit is set
            got_b = ev.pick(want[0], pick | (preds & L.FIT), req_mem_bytes=rm if (preds & L.FIT) else None, samples=smp if pick == L.PICK_SAMPLED else None)
            ok = np.array_equal(got_b, want[2])
            if ok and pick == L.PICK_SAMPLED:
                thin = want[0] & r.integers(0, 1 << 63, want[0].shape, dtype=np.uint64)
                got_t = ev.pick(thin, L.PICK_SAMPLED, samples=smp)
                bit = lambda row, n: n < N and bool((int(thin[row, n >> 6]) >> (n & 63)) & 1)  # noqa: E731
                want_t = np.array([next((int(x) for x in smp[i] if bit(i, int(x))), -1) for i in range(P)], dtype=np.int32)
                ok = np.array_equal(got_t, want_t)
            if not ok:
                fails += 1
                print(f"FAIL ksched_pick case seed {cs}: N={N} P={P} K={K} nt={nt} flags={flags:#x}", flush=True)
            picks["host-masks"] = picks.get("host-masks", 0) + 1
        if pick and r.random() < 0.35:
            # the host-side row shard (include/ksched.h "one host thread, several devices"): the batch cut into 1 .. 5 shards with
            # ksched_shard_bounds, every shard through ksched_eval_begin (selector columns addressed inside the whole batch's array with its
            # stride, bindings padded to ceil(P / n) with -1) + ksched_eval_end, merged like an all-gathered table -- on this one evaluator,
            # shard after shard
            fails += shard_halves(r, cs, "", N, P, K, nt, preds, flags, rc, rm, sel, tol, smp if pick == L.PICK_SAMPLED else None,
                                  5 if pick == L.PICK_SAMPLED else 0, want)
        if HOOKS and pick and r.random() < 0.35:
            fails += gathered_sequence(r, cs, "", cpu, mem, lab, taints, N, P, K, nt, preds, flags, rc, rm, sel, tol,
                                       smp if pick == L.PICK_SAMPLED else None, 5 if pick == L.PICK_SAMPLED else 0, want)[0]
        if r.random() < 0.3:  # ksched_explain on random pairs == the reason rebuilt from three single-predicate oracle masks
            from kube_scheduler_rs_reference_amd.evaluator import unpack_mask
            one = lambda f: unpack_mask(capi.eval_encoded(cpu, mem, lab, taints, rc, rm, sel, tol, None, f)[0], N)  # noqa: E731
            ok_f = one(L.FIT) if preds & L.FIT else np.ones((P, N), bool)
            ok_s = one(L.SEL) if preds & L.SEL else np.ones((P, N), bool)
            ok_t = one(L.TAINT) if preds & L.TAINT else np.ones((P, N), bool)
            want_r = np.where(~ok_f, L.REASON_NOT_ENOUGH_RESOURCES, np.where(~ok_s, L.REASON_NODE_SELECTOR_MISMATCH, np.where(~ok_t, L.REASON_TAINT_NOT_TOLERATED, L.REASON_OK)))
            pp, pn = r.integers(0, P, 4000).astype(np.uint32), r.integers(0, N, 4000).astype(np.uint32)
            got_r = ev.explain(rc, rm, sel if K else None, tol if (preds & L.TAINT) else None, pp, pn, preds)
            if not np.array_equal(got_r, want_r[pp, pn]):
                fails += 1
                print(f"FAIL explain case seed {cs}: N={N} P={P} K={K} cards={cards} nt={nt} preds={preds:#x}", flush=True)
        # ksched_summarize of the batch just evaluated == the popcounts of three single-predicate oracle masks, in check_node_validity's
        # order.  The decision comes from a generator of its own: the sequence of cases of a seed is what it was without this step.
        r_sum = np.random.default_rng([cs, 0x5C0])
        if r_sum.random() < 0.25:
            full = np.full((P, (N + 63) // 64), np.uint64(0xFFFFFFFFFFFFFFFF))
            if N % 64:
                full[:, -1] = np.uint64((1 << (N % 64)) - 1)
            mask = lambda f: capi.eval_encoded(cpu, mem, lab, taints, rc, rm, sel, tol, None, f)[0] if preds & f else full  # noqa: E731
            mF, mS, mT = mask(L.FIT), mask(L.SEL), mask(L.TAINT)
            pop = lambda m: np.bitwise_count(m).sum(axis=1) if hasattr(np, "bitwise_count") else np.unpackbits(np.ascontiguousarray(m).view(np.uint8), axis=1).sum(axis=1)  # noqa: E731
            want_c = np.stack([pop(mF & mS & mT), N - pop(mF), pop(mF & ~mS), pop(mF & mS & ~mT)], axis=1).astype(np.uint32)
            ev.set_kernel(str(r_sum.choice(["auto", "auto", "direct"])))
            got_c = ev.summarize(rc, rm, sel if K else None, tol if (preds & L.TAINT) else None, preds)
            ev.set_kernel("auto")
            if not np.array_equal(got_c, want_c):
                fails += 1
                print(f"FAIL summarize case seed {cs}: N={N} P={P} K={K} cards={cards} nt={nt} preds={preds:#x} kernel={ev.last_kernel}", flush=True)
            picks["summarize"] = picks.get("summarize", 0) + 1
    except Exception as e:  # noqa: BLE001
        fails += 1
        print(f"EXCEPTION case seed {cs}: N={N} P={P} K={K} cards={cards} nt={nt} flags={flags:#x}: {e}", flush=True)
        ev.set_kernel("auto")
print(f"fuzz: {cases} cases, {fails} failures, seed {seed}, pick launches {picks}")
sys.exit(1 if fails else 0)
