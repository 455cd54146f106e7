"""Child process of tests/test_gpu_admit_sharded.py: KSCHED_APPLY_WHILE_FIT at the sharded entry points, n ranks on one GPU.

    python -m tests.admit_sharded_worker <case> '<json spec>'

Runs against the test build of the library with the RCCL stand-in, as tests/apply_sharded_worker.py does (whose clique of evaluators it
borrows).  Prints "ok <case>" as its last line when all its checks passed.
"""
from __future__ import annotations

import json
import sys

import numpy as np
import torch

from kube_scheduler_rs_reference_amd import KschedError, _lib, synth
from tests.apply_sharded_worker import DEV, Ranks, batch, restate, t


def case_refused(spec):
    """ksched_apply_bindings_sharded_local with the flag: KSCHED_E_UNSUPPORTED, every replica's columns and index as they were, no
    status written; the same clique then applies the same batch with flags = 0 and every replica equals the single-ctx apply"""
    n, N, P = spec["n"], 3000, 9000
    c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=0xAD)
    cols = c.node_columns()
    R = Ranks(n, cols)
    before = R.ref.index_checksum()
    assert before != (0, 0)
    b, ok, rc, rm = batch(77, N, P, False)
    bounds = [0] + [P * (r + 1) // n for r in range(n)]
    sl = [slice(bounds[r], bounds[r + 1]) for r in range(n)]
    for flags in (_lib.APPLY_WHILE_FIT,):
        st = [torch.full((s.stop - s.start,), -7, dtype=torch.int32, device=DEV) for s in sl]
        try:
            R.clique.apply_bindings([t(b[s], np.int32) for s in sl], [t(rc[s], np.int64) for s in sl], [t(rm[s], np.int64) for s in sl],
                                    [bounds[r] for r in range(n)], ok=[t(ok[s], np.uint8) for s in sl], flags=flags, status_out=st)
        except KschedError as e:
            assert e.code == _lib.E_UNSUPPORTED, e.code
        else:
            raise AssertionError("the sharded apply accepted KSCHED_APPLY_WHILE_FIT")
        torch.cuda.synchronize()
        for r, e in enumerate(R.evs):
            got = e.read_nodes()  # (KSCHED_E_STATE here would say the replica was invalidated)
            assert np.array_equal(got[0], c.avail_cpu) and np.array_equal(got[1], c.avail_mem), f"rank {r}: columns changed"
            assert e.index_checksum() == before, f"rank {r}: index changed"
            assert (st[r].cpu().numpy() == -7).all(), f"rank {r}: a status was written"
    # with another admission rule or RELEASE beside it the flag set is malformed: E_INVAL, as at the single-ctx call
    for flags in (_lib.APPLY_WHILE_FIT | _lib.APPLY_RELEASE, _lib.APPLY_WHILE_FIT | _lib.APPLY_FIRST_PER_NODE):
        try:
            R.clique.apply_bindings([t(b[s], np.int32) for s in sl], [t(rc[s], np.int64) for s in sl], [t(rm[s], np.int64) for s in sl],
                                    [bounds[r] for r in range(n)], flags=flags)
        except KschedError as e:
            assert e.code == _lib.E_INVAL, e.code
        else:
            raise AssertionError(f"the sharded apply accepted flags {flags:#x}")
    # the clique is usable as before
    st, want = R.apply(bounds, b, ok, rc, rm, 0)
    cpu, mem = R.check_equal("flags = 0 after the refusal")
    for r in range(n):
        assert np.array_equal(st[r], want[bounds[r]:bounds[r + 1]]), f"rank {r} status"
    exp = restate(c.avail_cpu, c.avail_mem, b, rc, rm, ok, 0)
    assert np.array_equal(exp[0], cpu) and np.array_equal(exp[1], mem) and np.array_equal(exp[2], want)
    assert not np.array_equal(cpu, c.avail_cpu) and (want == _lib.APPLY_APPLIED).sum() > 1000
    R.close()


if __name__ == "__main__":
    case, spec = sys.argv[1], json.loads(sys.argv[2])
    {"refused": case_refused}[case](spec)
    print(f"ok {case}")
