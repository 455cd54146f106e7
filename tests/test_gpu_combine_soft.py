"""KSCHED_COMBINE_SOFT (extension E7) on the GPU, bit for bit: feasible(this call) is the oracle's mask of the same request, the expected mask
is tests/soft_ref.py (pinned by tests/test_soft_restatement.py) of the old mask and that one.
 1. both ops at the knife edges of k_mask_combine_soft: rows of one word, the valid-bits edge, odd and even W, one n at each side of every
    row-length switch of csrc/mask_combine_soft.hpp (the group sizes, registers against two reads) for both unit widths, packed and pitched
    rows, an unaligned base, more than one block and more than one grid pass; old masks whose neighbouring rows narrow, are dropped and are
    empty, with garbage at and beyond n, sentinels in the padding words and in two guard rows;
 2. the recipe of include/ksched.h as a chain -- the hard mask, two soft tiers, ksched_pick_device -- against a restatement written from the
    label columns, and the tiers in the other order, which give another mask;
 3. a pick in a soft combining call == ksched_pick_device on the combined mask with the pick flag alone, for all five picks and both ops,
    a pod whose tier was dropped included;
 4. the refusals: KSCHED_E_INVAL with mask and bindings untouched;
 5. a soft combining call and a scratch-mask pick on two streams, alternately.
Shapes are the smallest at which the kernel takes each path; the launch geometry is read from csrc/mask_combine_soft.hpp."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (COMBINE_AND, COMBINE_ANDNOT, COMBINE_OR, COMBINE_SOFT, FIT, PICK_BESTFIT, PICK_PACK, PICK_SAMPLED,
                                             PICK_SPREAD, PICK_UNIFORM, SEL, TAINT, WANT_FIT_MASK, _lib, pack_mask, synth)
from tests import combine_ref, soft_ref
from tests.pick_helpers import dev_of, fresh, mask_np, oracle_mask, pod_tensors, to_dev
from tests.uniform_ref import uniform_pick

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = [COMBINE_AND, COMBINE_ANDNOT]
OP_IDS = ["and", "andnot"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD_ROWS = 2
ALL = 0xFFFFFFFFFFFFFFFF


def plan_constants():
    """kSoftBlock, kSoftMaxGrid, kSoftWave, kSoftLaneUnits and kSoftKeepUnits as csrc/mask_combine_soft.hpp states them"""
    text = open(os.path.join(ROOT, "kube_scheduler_rs_reference_amd", "csrc", "mask_combine_soft.hpp")).read()
    names = ("kSoftBlock", "kSoftMaxGrid", "kSoftWave", "kSoftLaneUnits", "kSoftKeepUnits")
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1)) for name in names)


def switch_nodes():
    """one n at each side of every row-length switch of the plan, for one-word and for 16-byte units: the group doubles when a lane would get
    more than kSoftLaneUnits units (up to the wave), and past kSoftKeepUnits units per lane of a whole wave the row is read twice"""
    _, _, wave, lane_units, keep_units = plan_constants()
    units, g = [], 1
    while g < wave:
        units.append(lane_units * g)
        g *= 2
    units.append(keep_units * wave)
    out = set()
    for vec in (1, 2):
        for u in units:
            out.update((64 * u * vec, 64 * u * vec + 1))  # W = u * vec words (u units), and one word -- one unit -- more
    return sorted(out)


@pytest.fixture
def ev(evaluator):
    evaluator.set_kernel("auto")
    yield evaluator
    evaluator.set_kernel("auto")
    evaluator.set_option(_lib.OPT_PICK_FROM_MASK, 0)
    evaluator.set_option(_lib.OPT_FUSED_PICK, 1)


def set_cluster(ev, c):
    ev.set_nodes(c.avail_cpu, c.avail_mem, c.node_labels if c.n_keys else None, c.node_taints if c.n_taints else None)


def preds(c):
    return FIT | (SEL if c.n_keys else 0) | (TAINT if c.n_taints else 0)


# ---- 1. both ops at the knife edges ---------------------------------------------------------------------------------------------------
EDGE_NODES = sorted(set([1, 2, 63, 64, 65, 127, 129, 1024, 1025, 2049, 4097, 8193] + switch_nodes()))
EDGE_PODS = [1, 37, 257]
_EDGE = {}


def lowest_bit(w):
    return w & (~w + np.uint64(1))


def highest_bit(w):
    w = w.copy()
    for s in (1, 2, 4, 8, 16, 32):
        w |= w >> np.uint64(s)
    return w ^ (w >> np.uint64(1))


def one_bit_of(m, rng):
    """[P, W] with one set bit of every row of m that has one (in a randomly chosen non-zero word: its lowest or its highest bit), else zero"""
    P, W = m.shape
    w = (rng.random((P, W)) * (m != 0)).argmax(axis=1)
    word = m[np.arange(P), w]
    bit = np.where(rng.random(P) < 0.5, lowest_bit(word), highest_bit(word))
    out = np.zeros_like(m)
    out[np.arange(P), w] = bit
    return out


def old_mask_for(new, op, n, rng):
    """The old mask of a case, from the oracle's `new`, by row index mod 4: 0 -> random ORed with one bit that survives the op; 1 -> random
    restricted to the bits the op removes, ORed with one such bit; 2 -> zero; 3 -> random.  Then every row's last word gets all bits at and
    beyond n set."""
    P, W = new.shape
    valid = np.full((P, W), ALL, dtype=np.uint64)
    valid[:, -1] = combine_ref.valid_bits_word(n)
    survives, removed = (new & valid, ~new & valid) if op == COMBINE_AND else (~new & valid, new & valid)
    rnd = rng.integers(0, 1 << 64, size=(P, W), dtype=np.uint64)
    kind = (np.arange(P) % 4)[:, None]
    old = np.where(kind == 0, rnd | one_bit_of(survives, rng), np.where(kind == 1, (rnd & removed) | one_bit_of(removed, rng), np.where(kind == 3, rnd, np.uint64(0))))
    old[:, -1] |= ~valid[:, -1]
    return old


def edge_case(n, P):
    """the cluster, the oracle's mask of P pods x n nodes and, per op, the old mask, the expected mask and the rows' decisions: computed once,
    read-only.  Narrowed, dropped and empty rows are each at least a tenth of the rows."""
    if (n, P) not in _EDGE:
        c = synth.make_cluster(P, n, n_keys=4, n_taints=0, seed=0xE7000 + n)
        feas = oracle_mask(c, preds(c))
        feas.setflags(write=False)
        per_op = {}
        for op in OPS:
            old = old_mask_for(feas, op, n, np.random.default_rng([0xE7, n, op]))
            want = soft_ref.soft_combine(old, feas, op, n)
            what = soft_ref.decisions(old, feas, op, n)
            shares = [float((what == k).mean()) for k in (soft_ref.NARROWED, soft_ref.DROPPED, soft_ref.EMPTY)]
            print(f"n = {n}, P = {P}, {soft_ref.NAMES[op]}: narrowed {shares[0]:.2f}, dropped {shares[1]:.2f}, empty {shares[2]:.2f}")
            assert min(shares) >= 0.10, f"n = {n}, {soft_ref.NAMES[op]}: narrowed / dropped / empty rows are {shares} of the rows"
            for a in (old, want, what):
                a.setflags(write=False)
            per_op[op] = (old, want, what)
        _EDGE[(n, P)] = (c, feas, per_op)
    return _EDGE[(n, P)]


def first_pods(cols, p):
    """the first p pods of pod_tensors' columns ([P] or [n_keys, P], or None)"""
    return tuple(None if t is None else t[:p] if t.dim() == 1 else t[:, :p].contiguous() for t in cols)


def soft_once(ev, cols, flags, op, n, p, pitch, offset, old, want, what):
    """One soft combining call into a [p, W] view of rows `pitch` words apart that starts `offset` words into its buffer; behind the view's
    rows lie GUARD_ROWS more.  Words [0, W) are old's first p rows, every other word of the buffer the sentinel."""
    import torch
    W = (n + 63) // 64
    rows = p + GUARD_ROWS
    host = np.full(offset + rows * pitch + 1, SENTINEL, dtype=np.uint64)
    body = host[offset:offset + rows * pitch].reshape(rows, pitch)
    body[:p, :W] = old[:p]
    buf = torch.from_numpy(host.view(np.int64)).to(dev_of(ev))
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + rows * pitch].view(rows, pitch)[:p, :W]
    assert view.data_ptr() % 16 == 8 * (offset % 2) and (p == 1 or view.stride(0) == pitch)
    ev.eval_device(*first_pods(cols, p), None, flags | op | COMBINE_SOFT, out_feasible=view)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    got_body = got[offset:offset + rows * pitch].reshape(rows, pitch)
    assert np.array_equal(got_body[:p, :W], want[:p]), f"{what}: pods {np.nonzero((got_body[:p, :W] != want[:p]).any(axis=1))[0][:5]} differ from soft_ref"
    pad = got_body[:p, W:]
    assert ((pad == SENTINEL) | (pad == 0)).all(), f"{what}: a padding word is neither untouched nor zero"
    assert (got_body[p:] == SENTINEL).all(), f"{what}: wrote into the guard rows"
    assert (got[:offset] == SENTINEL).all() and got[-1] == SENTINEL, f"{what}: wrote outside the view"


@pytest.mark.parametrize("kernel", ["direct", "auto"])
@pytest.mark.parametrize("n", EDGE_NODES)
def test_both_ops_at_the_knife_edges(ev, n, kernel):
    c, feas, per_op = edge_case(n, max(EDGE_PODS))
    set_cluster(ev, c)
    W = ev.W
    assert W == (n + 63) // 64
    cols = pod_tensors(ev, c)
    flags = preds(c)
    # the mask kernel a plain call of this snapshot runs under `kernel`: a combining call names the same one
    ev.set_kernel(kernel)
    plain = ev.alloc_mask(max(EDGE_PODS), pitched=False)
    ev.eval_device(*cols, None, flags, out_feasible=plain)
    name = ev.last_kernel
    assert name == "direct" if kernel == "direct" else name in ("direct", "fused")
    assert np.array_equal(mask_np(plain), feas), "the plain call is the oracle's mask"
    std = int(_lib.load().ksched_mask_pitch(n))
    assert std % 16 == 0 and std >= W
    for p in EDGE_PODS:
        for pitch, offset in ((W, 0), (W + 1, 0), (std, 0), (std, 1), (W, 1)):
            for op, op_id in zip(OPS, OP_IDS):
                old, want, _ = per_op[op]
                soft_once(ev, cols, flags, op, n, p, pitch, offset, old, want, f"n = {n}, {kernel}, p = {p}, pitch {pitch}, offset {offset}, {op_id}")
                assert ev.last_kernel == name and ev.last_pick == "none"


def test_the_cases_cover_each_side_of_every_switch():
    """the n of the knife-edge test, against the plan's constants: rows of 4 * g and 4 * g + 1 units for every group g below the wave, and
    of 8 * 64 and 8 * 64 + 1 units, as one-word units (W = units) and as 16-byte units (W = 2 * units)"""
    block, max_grid, wave, lane_units, keep_units = plan_constants()
    assert (block, wave) == (256, 64) and lane_units < keep_units
    words = {(n + 63) // 64 for n in EDGE_NODES}
    g = 1
    while g < wave:
        for vec in (1, 2):
            assert {lane_units * g * vec, lane_units * g * vec + 1} <= words, (g, vec)
        g *= 2
    for vec in (1, 2):
        assert {keep_units * wave * vec, keep_units * wave * vec + 1} <= words, vec


@pytest.mark.parametrize("kernel", ["direct", "auto"])
def test_more_than_one_grid_pass(ev, kernel):
    """n = 63 (W = 1, a lane per row): one more row than a full grid covers in one pass; packed, one word into the buffer, and at pitch 2"""
    block, max_grid = plan_constants()[:2]
    n, p = 63, block * max_grid + 1
    c, feas, per_op = edge_case(n, p)
    set_cluster(ev, c)
    assert ev.W == 1
    cols = pod_tensors(ev, c)
    ev.set_kernel(kernel)
    for (pitch, offset), op in zip(((1, 0), (1, 1), (2, 0), (2, 1)), OPS + OPS[::-1]):
        old, want, _ = per_op[op]
        soft_once(ev, cols, preds(c), op, n, p, pitch, offset, old, want, f"n = {n}, {kernel}, p = {p}, pitch {pitch}, offset {offset}, op {op:#x}")


# ---- 2. the recipe ------------------------------------------------------------------------------------------------------------------------
ZONE, DISK, ZONE_A, DISK_HDD = 2, 1, 1, 2  # label keys (4 and 3 values; a tenth of the nodes carry none) and the values asked for


@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
@pytest.mark.parametrize("kernel", ["direct", "auto"])
def test_the_recipe_as_a_chain(ev, kernel, pitched):
    """the hard mask (fit), then two soft tiers -- prefer zone = a, prefer not disk = hdd --, then ksched_pick_device; and the tiers in the
    other order.  Pod 0 fits nowhere; pod 1 fits exactly two nodes, one in zone a with an hdd and one outside zone a without: whichever tier
    comes first decides, and the other one is dropped."""
    import torch
    P, N = 200, 300
    c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=0xE7C4A1)
    zone, disk = c.node_labels[ZONE], c.node_labels[DISK]
    x = int(np.nonzero((zone == ZONE_A) & (disk == DISK_HDD))[0][0])
    y = int(np.nonzero((zone != ZONE_A) & (disk != DISK_HDD))[0][0])
    c.avail_mem[[x, y]] = 1 << 50
    c.avail_cpu[[x, y]] = 1 << 40
    c.req_mem[0] = 1 << 60
    c.req_mem[1] = 1 << 49
    set_cluster(ev, c)
    ev.set_kernel(kernel)
    cpu, mem, _, _ = pod_tensors(ev, c)

    def sel_of(key, value):
        s = np.zeros((c.n_keys, P), dtype=np.uint32)
        s[key] = value
        return to_dev(ev, s, np.int32)

    # written from the label columns, not from masks
    fits = (c.req_cpu[:, None] <= c.avail_cpu[None, :]) & (c.req_mem[:, None] <= c.avail_mem[None, :])
    in_a, hdd = (zone == ZONE_A)[None, :], (disk == DISK_HDD)[None, :]

    def tier(cur, narrowed):
        return np.where(narrowed.any(axis=1)[:, None], narrowed, cur)
    zone_first = tier(tier(fits, fits & in_a), tier(fits, fits & in_a) & ~hdd)
    disk_first = tier(tier(fits, fits & ~hdd), tier(fits, fits & ~hdd) & in_a)
    assert not fits[0].any() and np.nonzero(fits[1])[0].tolist() == sorted((x, y))
    assert np.nonzero(zone_first[1])[0].tolist() == [x] and np.nonzero(disk_first[1])[0].tolist() == [y]
    assert (zone_first.any(axis=1) == fits.any(axis=1)).all() and (disk_first.any(axis=1) == fits.any(axis=1)).all()
    assert (zone_first != fits).any() and not np.array_equal(zone_first, disk_first)
    draws = np.random.default_rng(0xE7C4).integers(0, 1 << 32, size=(P, 3), dtype=np.uint64).astype(np.uint32)
    smp = to_dev(ev, draws, np.int32)
    tiers = {"zone": (sel_of(ZONE, ZONE_A), SEL | COMBINE_AND | COMBINE_SOFT), "disk": (sel_of(DISK, DISK_HDD), SEL | COMBINE_ANDNOT | COMBINE_SOFT)}
    for order, bits in ((("zone", "disk"), zone_first), (("disk", "zone"), disk_first)):
        want = pack_mask(bits)
        M = ev.alloc_mask(P, pitched=pitched)
        M.fill_(-1)  # whatever the mask held before the chain
        out = fresh(ev, P, 4)
        ev.eval_device(cpu, mem, None, None, None, FIT, out_feasible=M)
        for name in order:
            sel, flags = tiers[name]
            ev.eval_device(cpu, mem, sel, None, None, flags, out_feasible=M)
            assert ev.last_pick == "none"
        ev.pick_device(M, PICK_UNIFORM, out[:P], samples=smp)
        torch.cuda.synchronize()
        got = mask_np(M)
        assert np.array_equal(got, want), f"{order}: pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from the label columns' answer"
        b = out.cpu().numpy()
        assert np.array_equal(b[:P], uniform_pick(got, draws[:, 0], N)) and (b[P:] == -7).all()
        assert b[0] == -1 and b[1] == (x if order[0] == "zone" else y)


# ---- 3. a pick in a soft combining call -------------------------------------------------------------------------------------------------------
PICKS = [(PICK_SAMPLED, "from-mask"), (PICK_BESTFIT, "from-mask"), (PICK_UNIFORM, "uniform"), (PICK_SPREAD, "spread"), (PICK_PACK, "pack")]
_PICK_CASE = {}


def pick_case():
    if not _PICK_CASE:
        P, N = 300, 700
        c = synth.make_cluster(P, N, n_keys=8, n_taints=16, seed=0xE7B1C)
        feas = oracle_mask(c, preds(c))
        rng = np.random.default_rng(0xE7B1)
        old = pack_mask(rng.random((P, N)) < 0.3)
        old[0] = 0  # an empty row: stays empty
        old[1] &= ~feas[1]  # AND would empty it: the tier is dropped for pod 1
        old[2] = (old[2] & feas[2]) | one_bit_of(feas[2:3], rng)[0]  # AND-NOT would empty it: dropped for pod 2
        assert old[1].any() and old[2].any()
        draws = rng.integers(0, 1 << 32, size=(P, 5), dtype=np.uint64).astype(np.uint32)
        for a in (feas, old, draws):
            a.setflags(write=False)
        _PICK_CASE.update(c=c, feas=feas, old=old, draws=draws)
    return _PICK_CASE


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("pick,last_pick", PICKS, ids=["sampled", "bestfit", "uniform", "spread", "pack"])
def test_a_pick_in_a_soft_combining_call_is_the_pick_from_the_combined_mask(ev, pick, last_pick, op):
    """... with the pick flag alone and no predicate flag, under either setting of KSCHED_OPT_PICK_FROM_MASK and with the riding pick on or off;
    the pod whose tier was dropped is picked from the row it kept"""
    import torch
    k = pick_case()
    c, N = k["c"], k["c"].N
    P = c.P
    set_cluster(ev, c)
    cols = pod_tensors(ev, c)
    want = soft_ref.soft_combine(k["old"], k["feas"], op, N)
    what = soft_ref.decisions(k["old"], k["feas"], op, N)
    dropped = 1 if op == COMBINE_AND else 2
    assert what[0] == soft_ref.EMPTY and what[dropped] == soft_ref.DROPPED and (what == soft_ref.NARROWED).sum() > P // 2
    assert not np.array_equal(want, combine_ref.combine(k["old"], k["feas"], op, N))
    smp = to_dev(ev, c.samples if pick == PICK_SAMPLED else k["draws"], np.int32) if pick != PICK_BESTFIT else None
    combined = to_dev(ev, want, np.int64)
    alone = fresh(ev, P)
    ev.pick_device(combined, pick, alone, req_mem_bytes=cols[1], samples=smp)
    torch.cuda.synchronize()
    alone = alone.cpu().numpy()
    assert (alone >= 0).any() and ((alone >= 0) <= want.any(axis=1)).all()
    if pick != PICK_SAMPLED:  # (the sampled pick binds only if a drawn node is in the row)
        assert alone[0] == -1 and alone[dropped] >= 0
    for from_mask, fused_pick in ((0, 1), (1, 1), (0, 0)):
        ev.set_option(_lib.OPT_PICK_FROM_MASK, from_mask)
        ev.set_option(_lib.OPT_FUSED_PICK, fused_pick)
        M = to_dev(ev, k["old"], np.int64)
        out = fresh(ev, P, 4)
        ev.eval_device(*cols, smp, preds(c) | op | COMBINE_SOFT | pick, out_feasible=M, out_binding=out[:P])
        assert ev.last_pick == last_pick
        torch.cuda.synchronize()
        assert np.array_equal(mask_np(M), want)
        b = out.cpu().numpy()
        assert np.array_equal(b[:P], alone), f"pods {np.nonzero(b[:P] != alone)[0][:5]} differ from ksched_pick_device on the combined mask"
        assert (b[P:] == -7).all()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_refusals_leave_mask_and_bindings_untouched(ev, op):
    import torch
    c = synth.make_cluster(40, 130, n_keys=4, n_taints=0, seed=0xE7E44)
    set_cluster(ev, c)
    P, W = c.P, ev.W
    lib, h = _lib.load(), ev._h
    cpu, mem, sel, _ = pod_tensors(ev, c)
    smp = to_dev(ev, c.samples, np.int32)
    dM, dF = (torch.full((P, W), 0x5A5A5A5A, dtype=torch.int64, device=dev_of(ev)) for _ in range(2))
    dB = fresh(ev, P)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    other = COMBINE_ANDNOT if op == COMBINE_AND else COMBINE_AND
    f = FIT | SEL | op | COMBINE_SOFT
    st = C.c_void_p(torch.cuda.current_stream(ev.device).cuda_stream)

    def device(flags, feas, fit, bind, attempts=0, samples=None, p=P):
        return lib.ksched_eval_device_pitched(h, p, vp(cpu), vp(mem), vp(sel), None, vp(samples), attempts, flags, vp(feas), vp(fit), vp(bind), W, st)
    # the accepting entry points: no op, OR, two ops, no mask, a fit mask, an unknown bit
    assert device(FIT | SEL | COMBINE_SOFT, dM, None, None) == _lib.E_INVAL, "the modifier needs an op"
    assert device(FIT | SEL | COMBINE_SOFT | PICK_UNIFORM, dM, None, dB, 5, smp) == _lib.E_INVAL
    assert device(FIT | SEL | COMBINE_OR | COMBINE_SOFT, dM, None, None) == _lib.E_INVAL, "OR cannot empty a row"
    assert device(f | other, dM, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_OR, dM, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_AND | COMBINE_OR | COMBINE_ANDNOT, dM, None, None) == _lib.E_INVAL
    assert device(f, None, None, None) == _lib.E_INVAL
    assert device(f | PICK_UNIFORM, None, None, dB, 5, smp) == _lib.E_INVAL, "a pick does not stand in for the mask"
    assert device(f | WANT_FIT_MASK, dM, dF, None) == _lib.E_INVAL
    assert device(f | WANT_FIT_MASK, dM, None, None) == _lib.E_INVAL
    assert device(f, dM, dF, None) == _lib.E_INVAL
    assert device(f | 0x1000, dM, None, None) == _lib.E_INVAL, "0x1000 stays unknown"
    assert device(FIT | SEL | 0x1000, dM, None, None) == _lib.E_INVAL
    assert device(f | 0x4000, dM, None, None) == _lib.E_INVAL
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, FIT | SEL | COMBINE_SOFT, vp(dM), None, None, st) == _lib.E_INVAL
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, f | other, vp(dM), None, None, st) == _lib.E_INVAL
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, f, None, None, None, st) == _lib.E_INVAL
    # p == 0: a no-op
    assert device(f | PICK_UNIFORM, dM, None, dB, 5, smp, p=0) == _lib.OK
    # the entry points that do not take the flag, with an op beside it and without
    hM, hB = np.full((P, W), SENTINEL, np.uint64), np.full(P, -7, np.int32)
    table = torch.full((P, _lib.SUMMARY_WORDS), -7, dtype=torch.int32, device=dev_of(ev))
    pipe = ev.pipe(2)
    try:
        for soft in (op | COMBINE_SOFT, COMBINE_SOFT):
            assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), None, None, None, 0, FIT | soft, hp(hM), None, None) == _lib.E_INVAL
            assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), None, None, hp(c.samples), 5, FIT | soft | PICK_UNIFORM, hp(hM), None, hp(hB)) == _lib.E_INVAL
            dev_b, stream = C.c_void_p(), C.c_void_p()
            assert lib.ksched_eval_begin(h, P, hp(c.req_cpu), hp(c.req_mem), None, P, None, None, 0, FIT | soft, hp(hM), None, P, C.byref(dev_b), C.byref(stream)) == _lib.E_INVAL
            assert not dev_b.value
            assert lib.ksched_pick(h, P, hp(hM), None, hp(c.samples), 5, PICK_UNIFORM | soft, hp(hB)) == _lib.E_INVAL
            assert lib.ksched_pick_device(h, P, vp(dM), W, None, vp(smp), 5, PICK_UNIFORM | soft, vp(dB), st) == _lib.E_INVAL
            assert lib.ksched_summarize_device(h, P, vp(cpu), vp(mem), vp(sel), None, FIT | SEL | soft, vp(table), st) == _lib.E_INVAL
            assert lib.ksched_pipe_submit(pipe._h, 0, P, vp(cpu), vp(mem), vp(sel), None, vp(smp), 5, FIT | SEL | soft | PICK_UNIFORM, vp(dM), W, vp(dB)) == _lib.E_INVAL
    finally:
        pipe.close()
    torch.cuda.synchronize()
    assert (dM == 0x5A5A5A5A).all() and (dF == 0x5A5A5A5A).all() and (dB == -7).all() and (table == -7).all()
    assert (hM == SENTINEL).all() and (hB == -7).all()


# ---- 5. two users of the scratch mask ---------------------------------------------------------------------------------------------------------
def test_a_soft_combining_call_and_a_scratch_mask_pick_on_two_streams(ev):
    """stream A: soft combining calls (they evaluate into the ctx's scratch mask); stream B: uniform picks without out_feasible (they do too),
    with other predicates; enqueued alternately, each gives its single-stream answer"""
    import torch
    k = pick_case()
    c, N, P = k["c"], k["c"].N, k["c"].P
    set_cluster(ev, c)
    cols = pod_tensors(ev, c)
    smp = to_dev(ev, k["draws"], np.int32)
    want_masks = [soft_ref.soft_combine(k["old"], k["feas"], op, N) for op in OPS]
    fit_only = oracle_mask(c, FIT)
    want_pick = uniform_pick(fit_only, k["draws"][:, 0], N)
    rounds = 3 * len(OPS)
    masks = [to_dev(ev, k["old"], np.int64) for _ in range(rounds)]
    outs = [fresh(ev, P) for _ in range(rounds)]
    a, b = torch.cuda.Stream(ev.device), torch.cuda.Stream(ev.device)
    torch.cuda.synchronize()
    try:
        for i in range(rounds):
            ev.eval_device(*cols, None, preds(c) | OPS[i % 2] | COMBINE_SOFT, out_feasible=masks[i], stream=a)
            ev.eval_device(cols[0], cols[1], None, None, smp, FIT | PICK_UNIFORM, out_binding=outs[i], stream=b)
        torch.cuda.synchronize()
        for i in range(rounds):
            assert np.array_equal(mask_np(masks[i]), want_masks[i % 2]), f"round {i}: the combined mask"
            assert np.array_equal(outs[i].cpu().numpy(), want_pick), f"round {i}: the pick from the scratch mask"
    finally:
        ev.forget_stream(a)
        ev.forget_stream(b)
