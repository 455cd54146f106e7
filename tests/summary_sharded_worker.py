"""Child process of tests/test_gpu_summary.py: the sharded form of the summary, n ranks on one GPU.

    python -m tests.summary_sharded_worker

Runs against the test build of the library (tests/cpp/hooks/libksched_hip.so, $KSCHED_TEST_HOOKS=1) with the RCCL stand-in
(tests/cpp/libfake_rccl.so) that lets one GPU hold every rank of a dist.LocalClique.  Pod rows shard (ksched_shard_bounds), the
snapshot is replicated: LocalClique.summarize must give the table ONE ctx gives for the whole batch, which in turn is the
restatement's (tests/summary_ref.py).  Prints one JSON line: {"cases": k, "failures": [...]}.
"""
from __future__ import annotations

import json

import numpy as np

from kube_scheduler_rs_reference_amd import FIT, SEL, TAINT, Evaluator, synth
from kube_scheduler_rs_reference_amd.dist import LocalClique
from tests import summary_ref as ref


def main():
    flags = FIT | SEL | TAINT
    failures, cases = [], 0
    # (n ranks, pods): ragged shards, and with 5 pods over 4 ranks count_per_rank = 2 leaves the last rank an EMPTY shard
    for n, P in ((2, 1001), (3, 1000), (4, 5), (3, 2)):
        c = synth.make_cluster(P, 3100, n_keys=8, n_taints=16, seed=0x50 + n)
        evs = [Evaluator(0) for _ in range(n)]
        one = Evaluator(0)
        try:
            for e in evs + [one]:
                e.set_nodes(**c.node_columns())
            with LocalClique(evs) as clique:
                got = clique.summarize(c.req_cpu, c.req_mem, c.pod_sel, c.pod_tol, flags)
            single = one.summarize(c.req_cpu, c.req_mem, c.pod_sel, c.pod_tol, flags)
            want = ref.cluster_expected(c, flags)
            cases += 1
            if not np.array_equal(got, single):
                failures.append(f"n={n} P={P}: sharded != single ctx")
            if not np.array_equal(single, want):
                failures.append(f"n={n} P={P}: single ctx != restatement")
        finally:
            for e in evs + [one]:
                e.close()
    print(json.dumps({"cases": cases, "failures": failures}))


if __name__ == "__main__":
    main()
