"""What the GPU suites of the ranked picks (tests/test_gpu_uniform_pick.py, test_gpu_spread_pick.py, test_gpu_pack_pick.py) share: the
oracle's mask of a synthetic cluster, tensors of a cluster's pod columns on the evaluator's device, sentinel-filled outputs, and the draws
at the edges of a rank.  A plain module: no test, no fixture."""
import numpy as np

from oracle import capi


def oracle_mask(c, flags, cpu=None, mem=None):
    feas, _, _ = capi.eval_encoded(c.avail_cpu if cpu is None else cpu, c.avail_mem if mem is None else mem,
                                   c.node_labels if c.n_keys else None, c.node_taints if c.n_taints else None, c.req_cpu, c.req_mem,
                                   np.ascontiguousarray(c.pod_sel) if c.n_keys else None, c.pod_tol if c.n_taints else None, None, flags)
    return feas


def dev_of(ev):
    import torch
    return torch.device("cuda", ev.device)


def to_dev(ev, a, dt):
    import torch
    return torch.from_numpy(np.array(a, order="C").view(dt)).to(dev_of(ev))  # (a copy: the shared cases are read-only)


def pod_tensors(ev, c, lo=0, hi=None):
    hi = c.P if hi is None else hi
    return (to_dev(ev, c.req_cpu[lo:hi], np.int64), to_dev(ev, c.req_mem[lo:hi], np.int64),
            to_dev(ev, c.pod_sel[:, lo:hi], np.int32) if c.n_keys else None, to_dev(ev, c.pod_tol[lo:hi], np.int64) if c.n_taints else None)


def pitched_mask(ev, p, pitch, fill=0x5A):
    """a [p, W] view with rows `pitch` words apart over a buffer filled with a sentinel"""
    import torch
    buf = torch.empty((max(p, 1), max(pitch, 1)), dtype=torch.int64, device=dev_of(ev))
    buf.untyped_storage().fill_(fill)
    return buf[:p, :ev.W]


def mask_np(m):
    return m.contiguous().cpu().numpy().view(np.uint64)


def fresh(ev, p, extra=0):
    """p (+ extra guard) bindings holding a sentinel no pick writes"""
    import torch
    return torch.full((p + extra,), -7, dtype=torch.int32, device=dev_of(ev))


def u_lo(j, c):
    """the smallest draw whose k is j among c feasible nodes: ceil(j * 2^32 / c)"""
    return -((-j << 32) // c)


def u_hi(j, c):
    """the largest draw whose k is j"""
    return u_lo(j + 1, c) - 1
