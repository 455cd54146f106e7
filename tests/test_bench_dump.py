"""bench.py --dump-outputs: what the last timed step computed, as .npy files two builds can compare output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_capture_samples_fixed_rows_and_stays_in_budget():
    import torch

    import bench
    from kube_scheduler_rs_reference_amd import pack_mask

    rng = np.random.default_rng(7)
    P, N = 5000, 300
    bits = rng.random((P, N)) < 0.3
    words = np.zeros((P, 8), dtype=np.uint64)  # a pitched buffer: the mask is its first W columns
    words[:, :5] = pack_mask(bits)
    mask = torch.from_numpy(words.view(np.int64))[:, :5]
    binding = torch.from_numpy(rng.integers(-1, N, P).astype(np.int32))
    a = bench.capture_outputs(torch, torch.device("cpu"), binding, mask, 100, N)
    b = bench.capture_outputs(torch, torch.device("cpu"), binding, mask, 100, N)
    assert set(a) == {"bindings", "feasible", "feasible_rows"}
    assert a["bindings"].dtype == np.float64 and np.array_equal(a["bindings"], binding.numpy())
    assert a["feasible"].dtype == np.float32 and a["feasible_rows"].dtype == np.float64
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    rows = a["feasible_rows"].astype(np.int64) - 100
    assert a["feasible"].shape == (rows.size, N) and rows.size == min(P, bench.DUMP_MAX_ROWS)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["feasible"], bits[rows].astype(np.float32))
    # a wide snapshot: fewer rows, still under 64 MB in all
    big = bench.capture_outputs(torch, torch.device("cpu"), binding, torch.zeros((P, 782), dtype=torch.int64), 0, 50_000)
    assert 0 < big["feasible"].shape[0] < bench.DUMP_MAX_ROWS and sum(x.nbytes for x in big.values()) < 64_000_000
    # bindings only (--no-mask)
    assert set(bench.capture_outputs(torch, torch.device("cpu"), binding, None, 0, N)) == {"bindings"}


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(built, tmp_path):
    quick = ["--steps", "7", "--warmup", "3", "--ramp-ms", "5", "--kernel-samples", "4", "--repeats", "1", "--no-cpu-baseline", "--no-others",
             "--no-end-to-end", "--live-traffic", "off"]
    dumps = []
    for i in range(2):
        d = tmp_path / str(i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *quick, "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 7 and line["parity_check"]["mismatches"] == 0
        assert line["dumped_outputs"]["input_batch"] == 6 % line["config"]["input_rotation"]["batches"]
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64_000_000
        dumps.append({f.stem: np.load(f) for f in d.iterdir()})
    a, b = dumps
    assert set(a) == {"bindings", "feasible", "feasible_rows"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a["bindings"].shape == (100_000,) and a["feasible"].shape == (a["feasible_rows"].size, 5_000)
    # a pod bound to a node is feasible on it
    rows = a["feasible_rows"].astype(np.int64)
    bound = a["bindings"][rows].astype(np.int64)
    hit = bound >= 0
    assert hit.any() and np.all(a["feasible"][np.nonzero(hit)[0], bound[hit]] == 1.0)
