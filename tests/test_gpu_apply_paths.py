"""Every evaluation path after ksched_apply_bindings_device on one ctx, against the oracle on the columns the exact-integer restatement
gives (tests/apply_paths_worker.py; one child process per case).

The apply writes `available` into the columns, the node records and the dirty tiles of the bitmap index.  After each apply these run:
the fused, direct and auto kernels; no pick, the sampled pick in every form (its own launch "select", riding as waves "fused" or as tile
tests "fused-tile", from the mask) and best fit (bitmap rows in one or two stages, the list-key lists, from the mask); ksched_eval and
ksched_eval_device with and without a mask; ksched_pick from the oracle's host mask; ksched_explain on 4000 random pairs.  Snapshots: up to
eight keys with taints, ten keys, a list key, and one that indexed_plan refuses (no index: every evaluation reads columns and records).
The uniform pick runs on every kernel choice, bindings only, through ksched_eval_device and ksched_pick, against tests/uniform_ref.py.
The spread pick -- the one pick that reads the VALUES of the columns an apply has just written -- runs against tests/spread_ref.py on the
oracle's mask and the restated columns: d = 5 beside the mask on every kernel choice, d = 2 bindings only (host and device pointers),
ksched_eval_device beside a mask, ksched_pick with d = 64, d = 1 against the restatement's uniform pick.  Real bindings come from the
sampled, the uniform and the spread pick in turn.  Two input conditions keep the spread legs from passing vacuously (walk_single; asserted
without a GPU by tests/test_apply_paths_host.py): before any apply 35 % of the pods or more bind to another node than their candidate 0,
and at every node count from 1025 on the columns from before an apply of real bindings would change at least one spread binding.
Admission in pod order (KSCHED_APPLY_WHILE_FIT) stands in all six children, each expectation tests/admit_ref.py's: one more round
[admit -> the whole matrix] at every node count of the four walks, on real bindings at 63 and 4097 nodes and on random ones at 1, 1025
and 50 000; in the sizes case an admit behind two applies and two updates with no host wait, at 4097 nodes a second one that outgrows the
admit scratch; in the large case an admit of 600 000 pods before the four other flag sets.  Their input conditions (deferrals, pods
admitted behind a deferred one, columns unlike what flags = 0 and FIRST_PER_NODE leave) are asserted from the restatement in the
worker before the device is compared, and without a GPU by tests/test_apply_paths_host.py.
The pack pick (KSCHED_PICK_PACK) has the spread pick's legs one for one, against tests/pack_ref.py on the same draws: it reads the same two
columns through a kernel of its own, so its stale-column count is printed and asserted beside the spread pick's.  The combining calls
(KSCHED_COMBINE_AND / _OR / _ANDNOT, KSCHED_COMBINE_SOFT) run per predicate set and kernel choice as chains of ksched_eval_device calls on
one mask, packed under one kernel choice and pitched under the next, filled with ones beforehand and compared after every link with
tests/combine_ref.py / tests/soft_ref.py on the oracle's masks: FIT then the other predicates with AND (== the one call); FIT, AND-NOT, OR
(== the fit mask again); and a soft chain -- the hard mask, two soft tiers on the selector table rolled by one and by two pods -- whose last
link carries the pack, spread, uniform, sampled and best-fit pick in turn.  So every combining call evaluates into the ctx's scratch mask
after an apply, on list-key, ten-key and unindexed snapshots; the sizes case enqueues the soft chain with PICK_PACK behind its queued
applies and updates with no host wait, while that scratch mask shrinks in need to one node and regrows to 60 000.  Floors on what the tiers
narrow, drop, find empty and change, on the bindings they move and on fit & ~feasible are asserted from the restatements first.
The operator and the tagged selector calls (KSCHED_SELOP_EXISTS / _GT / _LT -> k_eval_selop, KSCHED_SELOP_TAGGED -> k_eval_seltag) run once
per predicate set in every matrix, so after every apply and on every kind of snapshot: the bare masks through ksched_eval against
tests/selop_ref.py on the selector table and tests/seltag_ref.py on a tagged copy of it (every id entry under one of the six tags, drawn
uniformly); the plain table under the tagged call against the oracle's SEL-only mask; and a chain on one mask filled with ones -- the other
predicates, the tagged call with AND, EXISTS with AND-NOT, GT with OR, LT with the soft AND -- compared after every link, whose last link
carries the pack, spread, uniform, sampled and best-fit pick in turn, compared with the pick's restatement on the expected mask and the
restated columns.  The ten-key and the list-key snapshot take the kernels' second key pass.  The sizes case enqueues the chain with
PICK_SPREAD behind the soft chain, still with no host wait: with 3000 pods at 50 000 and 60 000 nodes its operator kernels walk two pod
tiles per block.  Floors on the rows that are neither full nor empty, on the pods constrained through negated tags only, on the pods that
constrain keys of both passes and on what every link changes are asserted from the references first.
The terms call (KSCHED_SEL_TERMS: SEL | SELOP_TAGGED | sel_terms(T) -> k_eval_selterms, k_eval_selterms_wide past eight keys) runs beside them,
once per predicate set in every matrix: the bare mask of a three-term table (the tagged table, the tagged selectors of the two pods before,
per-pod term counts with SEL_NEVER padding, a zero term behind a real one) against tests/selterms_ref.py; the tagged table under
sel_terms(1) against tests/seltag_ref.py; the plain table with padding behind it against the oracle's SEL-only mask; and a chain on one mask
filled with ones -- the other predicates, the terms call with AND, the table rolled by one pod with the soft AND -- compared after every
link, whose last link carries each of the five picks in turn.  The ten-key and the list-key snapshot take the wide kernel.  The sizes case
enqueues that chain with PICK_PACK on a third mask behind the selector chain: the standing terms call with two pod tiles per block.  Floors
on the rows that are neither empty nor full, that differ from every single term's row, that are full although term 0's is not, that an
and-of-ors kernel would get wrong, on the term counts and on what every link changes are asserted from the references first.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = [1, 63, 1025, 4097, 50_000]
SINGLE = {"nodes": NODES, "pods": 2000, "pods_big": 600, "rounds": 3}  # (tests/test_apply_paths_host.py walks the same specs without a GPU)
SIZES = {"nodes": [50_000, 300, 4097, 1, 60_000]}
LARGE = {"pods": 600_000}


def run(case, spec, timeout=300):
    r = subprocess.run([sys.executable, "-m", "tests.apply_paths_worker", case, json.dumps(spec)], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-6000:]
    assert r.stdout.rstrip().endswith(f"ok {case}")
    return r.stdout


@pytest.mark.parametrize("kind", ["taints", "many-keys", "list-key", "unindexed"])
def test_every_path_after_an_apply(built, kind):
    """per node count: the matrix, then three rounds of [apply -> the matrix]; the applies rotate over plain, FIRST_PER_NODE, RELEASE and
    both, with and without ok, on the previous evaluation's device bindings and on random ones; then the admit round, [apply with
    WHILE_FIT -> the matrix], on real bindings at 63 and 4097 nodes and on random ones at the others"""
    out = run("single", dict(SINGLE, kind=kind))
    reached = out.rsplit("picks reached", 1)[-1]
    assert "'spread'" in reached, "the spread pick is not among the picks reached"
    assert "'pack'" in reached, "the pack pick is not among the picks reached"
    for pick in ("pack", "spread", "uniform", "sampled", "bestfit"):
        assert f"'chain-{pick}'" in reached, f"no soft chain carried the {pick} pick in its last link"
        assert f"'selchain-{pick}'" in reached, f"no selector chain carried the {pick} pick in its last link"
        assert f"'termchain-{pick}'" in reached, f"no terms chain carried the {pick} pick in its last link"
    for N in NODES:
        assert f"{kind} N={N} admit round (" in out, f"no admit round at {N} nodes"


def test_snapshot_sizes_and_updates_between_applies_on_one_ctx(built):
    """50 000 -> 300 -> 4097 -> 1 -> 60 000 nodes on one ctx: the apply scratch is kept while the snapshot shrinks and regrows, then
    reallocated; per snapshot an apply, an update of the applied tiles, an apply, an update, an apply with WHILE_FIT and at 4097 nodes a
    second one of four times the pods (the admit scratch reallocated behind a queued admit), no host wait"""
    out = run("sizes", SIZES)
    assert out.count(": admit of ") == len(SIZES["nodes"]) + 1
    assert out.count("chain: the pack pick (d = 5) on the tier-2 mask binds") == 3  # the chain's floors, at the three snapshots from 1025 nodes on
    assert out.count("selchain: the selector chain's links change") == 3  # and the selector chain's, at the same three
    assert out.count("termchain: the terms chain's links change") == 3  # and the terms chain's


def test_a_batch_longer_than_one_stride_of_the_pod_kernels(built):
    """600 000 pods (the pod passes launch at most 2048 x 256 threads): some nodes' first eligible pod lies past pod 524 288; WHILE_FIT
    first (segments of more than 10 000 pods with admits and deferrals mixed, ten merge passes), then the four other flag sets"""
    out = run("large", LARGE, timeout=600)
    assert f"P={LARGE['pods']} admit:" in out
