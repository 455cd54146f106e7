"""A short run of the randomised differential test (tools/fuzz_parity.py): random shapes, key counts / cardinalities (rows, list
keys, more than eight keys), taints, predicate subsets, the sampled and best-fit picks, snapshot updates (available, or labels and taints)
and on-device applies of the previous evaluation's bindings between evaluations, both kernels -- every mask word and binding against the
oracle; and at every step the uniform pick against tests/uniform_ref.py on the oracle's mask, and the spread pick (d of 1, 2, 3, 5, 8, 33,
64; both kernels, with and without the mask) against tests/spread_ref.py on the oracle's mask and on the columns the step's updates and
applies must have left -- the one pick that goes wrong, for a few pods, when a column is stale.  With the hooks the spread pick also goes
through the multi-device sequence, a sharded apply of its gathered bindings and the sequence again on the replicas' columns.  Likewise at
every step the pack pick (the same draws and d; tests/pack_ref.py) and one combining chain of 2 to 4 ksched_eval_device calls on one mask --
random predicate subsets and ops, KSCHED_COMBINE_SOFT at random, odd pitches and bases with sentinel words around the view, a random pick
in the last link -- against tests/combine_ref.py / tests/soft_ref.py on the oracle's per-link masks; with the hooks the pack pick takes the
spread pick's multi-device route and the chain runs on every replica after the sharded apply.  And at every step one operator call
(KSCHED_SELOP_EXISTS / _GT / _LT at random) and one tagged call (KSCHED_SELOP_TAGGED: all six tags, now and then tags 6 and 7, ids at and
beside the nodes' ids and 0, 1, 0x1FFFFFFF) against tests/selop_ref.py / tests/seltag_ref.py on the labels as the step's updates left them --
into a sentinel-surrounded view at an odd pitch or base, about half of them as one more link on the step's combining chain, with a random
pick -- and both through ksched_eval_begin / _end over 1 to 5 row shards (sel_stride > p); with the hooks both run on every replica after
the sharded apply.  Asserted here: the tallies 'selop', 'seltag', 'seltag-negated-padding' (a pod constrained through NE / ABSENT only, in
rows with padding bits) and 'selop-sharded-halves' in both runs, 'selop-on-replicas' with the hooks; 'selop-two-pass' and
'selop-two-tiles' are recorded from a long run.  And at every step with keys one terms call (KSCHED_SEL_TERMS: 1, 2, 3 or 15 terms per pod of such
tagged entries, per-pod term counts with SEL_NEVER padding, now and then a zero term behind a real one) against tests/selterms_ref.py:
the bare mask, the call under a drawn combine with a drawn pick, and the two halves over 1 to 5 row shards (column (t, k) at
(t * n_keys + k) * sel_stride); with the hooks on every replica after the sharded apply.  Asserted here: 'selterms', 'selterms-late-full' (a
pod whose row a term behind term 0 completes) and 'selterms-sharded-halves' in both runs, 'selterms-on-replicas' with the hooks;
'selterms-wide' (more than eight keys) is recorded from a long run.  (240 s runs of the same tool: profiles/uniform_pick_standing_checks.txt,
profiles/spread_pick_standing_checks.txt, profiles/combine_pack_standing_checks.txt, profiles/selop_seltag_standing_checks.txt,
profiles/selterms_standing_checks.txt.)"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tally(out, name):
    m = re.search(rf"'{re.escape(name)}': (\d+)", out)
    return int(m.group(1)) if m else 0


def assert_new_tallies(out):
    print(out[-1500:])
    assert tally(out, "uniform") > 0, "no evaluation ran the uniform pick"
    assert tally(out, "uniform-ranked") > 0, "no uniform pick chose among two or more feasible nodes"
    assert tally(out, "labels") > 0, "no case updated node labels between evaluations"
    assert tally(out, "pack") > 0, "no evaluation ran the pack pick"
    assert tally(out, "pack-ranked") > 0, "no pack pick bound a pod to another node than its candidate 0"
    assert tally(out, "combine") > 0, "no combining chain ran"
    assert tally(out, "soft-narrowed") > 0, "no soft link narrowed a row"
    assert tally(out, "soft-dropped") > 0, "no soft link was dropped for a row"
    assert tally(out, "soft-empty") > 0, "no soft link met an empty row"
    assert tally(out, "selop") > 0, "no operator call ran"
    assert tally(out, "seltag") > 0, "no tagged call ran"
    assert tally(out, "seltag-negated-padding") > 0, "no tagged call had a pod constrained through NE / ABSENT only in rows with padding bits"
    assert tally(out, "selop-sharded-halves") > 0, "no operator or tagged call went through ksched_eval_begin / _end over row shards"
    assert tally(out, "selterms") > 0, "no terms call ran"
    assert tally(out, "selterms-late-full") > 0, "no terms call had a pod whose row is completed by a term behind term 0"
    assert tally(out, "selterms-sharded-halves") > 0, "no terms call went through ksched_eval_begin / _end over row shards"


def test_fuzz_parity_short(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "12", "20260923"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 failures" in r.stdout
    assert "'apply': " in r.stdout, "no case applied an evaluation's bindings on the device"
    assert_new_tallies(r.stdout)
    assert tally(r.stdout, "spread") > 0, "no evaluation ran the spread pick"
    assert tally(r.stdout, "spread-ranked") > 0, "no spread pick bound a pod to another node than its candidate 0"


def test_fuzz_parity_short_with_the_multi_device_sequence(built):
    """The same run with the test hooks on: about a third of the cases with a pick also go through the WHOLE multi-device sequence --
    ksched_comm_create_local over 2 .. 4 evaluators on the one GPU (TEST-ONLY librccl stand-in), ksched_eval_begin on every replica,
    ksched_gather_buffer, ksched_allgather_bindings_local, ksched_eval_end(gathered_0) -- and must merge to the oracle's bindings and masks."""
    fake = os.path.join(ROOT, "tests", "cpp", "libfake_rccl.so")
    if not os.path.exists(fake):
        subprocess.check_call(["make", "-C", ROOT, "-s", "host"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "12", "777001"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, KSCHED_TEST_HOOKS="1", KSCHED_LIB=os.path.join(ROOT, "tests", "cpp", "hooks", "libksched_hip.so"), KSCHED_RCCL_LIB=fake))
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "gathered-over-" in r.stdout and " 0 failures" in r.stdout
    assert "'apply': " in r.stdout and "'sharded-apply-over-" in r.stdout, "no case applied bindings on the device, or none over replicas"
    assert_new_tallies(r.stdout)
    assert re.search(r"'gathered-over-\d': [1-9]", r.stdout), "no sampled or best-fit case went through the multi-device sequence"
    assert re.search(r"'uniform-gathered-over-\d': [1-9]", r.stdout), "no uniform pick went through the multi-device sequence"
    assert re.search(r"'spread-gathered-over-\d': [1-9]", r.stdout), "no spread pick went through the multi-device sequence"
    assert re.search(r"'pack-gathered-over-\d': [1-9]", r.stdout), "no pack pick went through the multi-device sequence"
    assert tally(r.stdout, "combine-on-replicas") > 0, "no combining chain ran on the replicas after a sharded apply"
    assert tally(r.stdout, "selop-on-replicas") > 0, "no operator and tagged call ran on the replicas after a sharded apply"
    assert tally(r.stdout, "selterms-on-replicas") > 0, "no terms call ran on the replicas after a sharded apply"
