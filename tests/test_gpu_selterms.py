"""KSCHED_SEL_TERMS (extension E10: ORed selector terms in one tagged call) on the GPU, bit for bit against tests/selterms_ref.py (pinned by
tests/test_selterms_restatement.py), with tests/combine_ref.py / tests/soft_ref.py, the calls that exist already and ksched_pick_device on
top of it.
 1. mask parity at the word, wave and block edges of the kernels' mapping (n, read off the launch geometry), the tile edges of the pod
    walk (p), each side of the eight-key boundary between the two kernels (keys) and term counts 1, 2, 3 and 15, into packed rows, rows at
    ksched_mask_pitch(n) and views that start one word into their buffer; node ids on both sides of 2^29, all six tags, tags 6 / 7 and
    NEVER; what the cases tell apart is asserted on the EXPECTED values first;
 2. agreement with what exists: one term == the tagged call; T terms == a tagged call and T - 1 tagged calls under KSCHED_COMBINE_OR; a
    pod padded with NEVER terms == the same pod at its own term count; a leading all-zero term gives the valid-bits row;
 3. the call under AND, OR, AND-NOT and the soft modifier into a caller's mask with garbage beyond n; each of the five picks in the call,
    plain and combining == ksched_pick_device on the resulting mask; the header's recipe end to end with node_affinity_rows' rows;
 4. the host forms ksched_eval and ksched_eval_begin / _end (sel_stride > p) give the device form's bits;
 5. a label update before the call, and two streams around a label update;
 6. the refusals at every entry point with outputs untouched, field 0 beside what is legal today, and the edge sizes.
Every output goes into sentinel-filled buffers with guard rows.  Shapes are the smallest at which the kernels take each path.  What the three selector
files share -- the guarded evaluation, the bodies that are the same for every call -- is tests/selector_calls.py's."""
import ctypes as C

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import (COMBINE_AND, COMBINE_ANDNOT, COMBINE_OR, COMBINE_SOFT, FIT, MAX_TERMS, PICK_BESTFIT, PICK_SAMPLED, PICK_SPREAD, PICK_UNIFORM,
                                             SEL, SEL_NEVER, SEL_TERMS_MASK, SEL_TERMS_SHIFT, SELOP_EXISTS, SELOP_GT, SELOP_LT, SELOP_TAGGED, TAINT, WANT_FIT_MASK,
                                             Evaluator, _lib, node_affinity_rows, pack_mask, sel_terms, synth)
from tests import combine_ref, selector_calls, selterms_ref, seltag_ref
from tests.pick_helpers import dev_of, fresh, mask_np, oracle_mask, pod_tensors, to_dev
from tests.selector_calls import COMBINES, PICKS, SENTINEL, SelectorCall, ev, eval_into_view, row_kinds, zeros_dev  # noqa: F401 (ev: the fixture)

pytestmark = pytest.mark.gpu

TG = SEL | SELOP_TAGGED
EQ, NE, EX, AB, GT, LT = seltag_ref.TAGS
E = seltag_ref.entry


def F(t):
    return TG | sel_terms(t)


def call(t):
    return SelectorCall(F(t), "selterms", selterms_ref.selterms_mask, (t,))


# the launch geometry (csrc/sel_ops.hpp, which csrc/sel_terms.hpp's plan takes over): a wave owns 4 word columns of 64 nodes, a block is 4
# waves, a pass is 8 keys -- more than 8 keys take the wide kernel
CW, WAVES, PASS_KEYS = 4, 4, 8
WAVE_NODES, BLOCK_NODES = 64 * CW, 64 * CW * WAVES
NODES = [1, 63, 64, 65, WAVE_NODES - 1, WAVE_NODES, WAVE_NODES + 1, BLOCK_NODES - 1, BLOCK_NODES, BLOCK_NODES + 1, 4 * BLOCK_NODES + 1]
PODS = [1, 63, 64, 65, 129]
KEYS = [1, PASS_KEYS, PASS_KEYS + 1, 32]
TERMS = [1, 2, 3, MAX_TERMS]
P_MAX, T_MAX = max(PODS), max(TERMS)
# what a node carries: 0 = not the key; small ids; ids on both sides of 2^29 and of the sign bit
IDS = np.array([0, 1, 2, 3, 4, 5, 1, 2, 3, 0x1FFFFFFF, 0x20000000, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)
ENTRY_IDS = np.array([1, 2, 3, 4, 5, 0x1FFFFFFF], dtype=np.uint32)
TAG_WEIGHTS = [0.5, 0.1, 0.05, 0.1, 0.1, 0.15]  # EQ-heavy: a term stays selective, so that an OR of fifteen is not every node


def test_the_constants_are_the_restatements():
    assert (SEL_TERMS_SHIFT, SEL_TERMS_MASK, MAX_TERMS) == (selterms_ref.SHIFT, selterms_ref.MASK, selterms_ref.MAX_TERMS)
    assert [sel_terms(t) for t in TERMS] == [selterms_ref.field(t) for t in TERMS]
    assert (CW, WAVES, PASS_KEYS) == (4, 4, 8) and NODES[-4:] == [1023, 1024, 1025, 4097]


# ---- 1. mask parity -----------------------------------------------------------------------------------------------------------------------
_CASES = {}


def entries_for(rng, keys, p):
    """[T_MAX][keys][p] tagged entries.  A term constrains two keys (one where there is one) by tags drawn with TAG_WEIGHTS; 1 entry in 24 is
    tag 6, tag 7 or NEVER.  By pod % 8: 1 -- term 0 all zeros (the valid-bits row); 2 -- a pod with its own term count c in 1 .. 3 and
    NEVER terms behind them; 3 -- every term NEVER (no node); 5 -- term 1 all zeros behind a real term 0; 4 -- with more than eight keys:
    every term constrains one key on each side of a pass boundary by equality, so that ORing pass by pass is wrong."""
    sel = np.zeros((T_MAX, keys, p), dtype=np.uint32)
    for pod in range(p):
        for t in range(T_MAX):
            ks = rng.choice(keys, size=min(2, keys), replace=False)
            for k in ks:
                tag = rng.choice(6, p=TAG_WEIGHTS)
                e = E(tag, ENTRY_IDS[rng.integers(0, ENTRY_IDS.size)])
                odd = rng.integers(0, 24)
                e = E(6, 3) if odd == 0 else E(7, 1) if odd == 1 else np.uint32(SEL_NEVER) if odd == 2 else e
                sel[t, k, pod] = e
        kind = pod % 8
        if kind == 1:
            sel[0, :, pod] = 0
        elif kind == 2:
            c = 1 + (pod // 8) % 3
            sel[c:, :, pod] = 0
            sel[c:, rng.integers(0, keys), pod] = SEL_NEVER
        elif kind == 3:
            sel[:, rng.integers(0, keys), pod] = SEL_NEVER
        elif kind == 5:
            sel[1, :, pod] = 0
        elif kind == 4 and keys > PASS_KEYS:
            sel[:, :, pod] = 0
            for t in range(T_MAX):
                lo, hi = rng.integers(0, PASS_KEYS), rng.integers(PASS_KEYS, keys)
                sel[t, lo, pod] = E(EQ, 1 + (t % 3))
                sel[t, hi, pod] = E(EQ, 1 + ((t + pod // 8) % 5))
    return sel


def case(n, keys, p=P_MAX):
    """labels [keys][n] drawn from IDS, entries [T_MAX][keys][p], and per term count T the expected mask of the first T terms; computed
    once, read-only"""
    if (n, keys, p) not in _CASES:
        rng = np.random.default_rng([0xE10, n, keys, p])
        lab = IDS[rng.integers(0, IDS.size, size=(keys, n))]
        sel = entries_for(rng, keys, p)
        bits = [seltag_ref.pass_bits(lab, sel[t]) for t in range(T_MAX)]
        want, acc = {}, np.zeros((p, n), dtype=bool)
        for t in range(T_MAX):
            acc = acc | bits[t]
            if t + 1 in TERMS:
                want[t + 1] = seltag_ref.pack(acc)
        single = [seltag_ref.pack(b) for b in bits[:3]]
        for a in [lab, sel] + list(want.values()) + single:
            a.setflags(write=False)
        _CASES[(n, keys, p)] = dict(lab=lab, sel=sel, want=want, single=single)
    return _CASES[(n, keys, p)]


_FACTS = {}


def matrix_facts():
    """What the matrix contains, from the expected values alone -- asserted before any device call, so that no case can pass vacuously."""
    if _FACTS:
        return _FACTS
    full = empty = or_shows = wrong_per_pass = 0
    mixed = {}
    tags = set()
    for n in NODES:
        for keys in KEYS:
            k = case(n, keys)
            assert np.array_equal(k["want"][1], k["single"][0]), "one term IS the tagged row"
            for T in TERMS:
                f, e, m = row_kinds(k["want"][T], n)
                full, empty = full + f, empty + e
                mixed[(n, keys, T)] = m / P_MAX
            # rows of the three-term call that differ from every single term's row: the OR shows
            or_shows += int((np.stack([(k["want"][3] != s).any(axis=1) for s in k["single"]]).all(axis=0)).sum())
            if keys > PASS_KEYS and n >= 63:
                for T in (2, 3, MAX_TERMS):
                    wrong = selterms_ref.and_of_ors_mask(k["lab"], k["sel"][:T], PASS_KEYS)
                    assert (wrong != k["want"][T]).any(), f"n = {n}, keys = {keys}, T = {T}: ORing pass by pass gives the same bits"
                    wrong_per_pass += 1
            count = np.unpackbits(k["want"][3].view(np.uint8), axis=1).sum(axis=1)
            for pod in np.nonzero((count > 0) & (count < n))[0]:
                tags.update(int(e_) >> 29 for e_ in k["sel"][:3, :, pod].ravel() if e_)
    _FACTS.update(full=full, empty=empty, or_shows=or_shows, wrong_per_pass=wrong_per_pass, mixed=mixed, tags=tags)
    return _FACTS


def check_matrix_facts():
    f = matrix_facts()
    assert f["full"] >= 100 and f["empty"] >= 100, "rows with every node and rows with none"
    assert f["or_shows"] >= 200, "rows that differ from every single term's row"
    assert f["wrong_per_pass"] == 3 * 2 * len([n for n in NODES if n >= 63])
    for (n, keys, T), m in f["mixed"].items():
        if n >= 63 and T <= 3:
            assert m >= 0.3, f"n = {n}, keys = {keys}, T = {T}: only {m:.0%} of the rows are neither empty nor full"
        elif n >= 63:
            assert m >= 0.1, f"n = {n}, keys = {keys}, T = {T}: only {m:.0%} of the rows are neither empty nor full"
    assert set(range(8)) <= f["tags"], "every tag, 6 and 7 included, occurs in a row that is neither empty nor full"


def test_the_matrix_tells_the_kernels_from_wrong_ones():
    check_matrix_facts()


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("n", NODES)
def test_mask_parity(ev, n, keys):
    check_matrix_facts()
    k = case(n, keys)
    W = (n + 63) // 64
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    assert ev.W == W
    std = int(_lib.load().ksched_mask_pitch(n))
    assert std % 16 == 0 and std >= W
    layouts = ((W, 0), (std, 0), (W, 1), (std, 1))
    i = 0
    for T in TERMS:
        want = k["want"][T]
        assert want.shape == (P_MAX, W) and not (want[:, -1] & ~np.uint64(combine_ref.valid_bits_word(n))).any()
        for p in PODS:
            for pitch, offset in (layouts if p == P_MAX else (layouts[i % 4],)):  # every layout at the largest p, one in turn at the others
                got = eval_into_view(ev, k["sel"][:T], F(T), n, p, pitch, offset)
                assert np.array_equal(got, want[:p]), \
                    f"T = {T}, p = {p}, pitch {pitch}, offset {offset}: pods {np.nonzero((got != want[:p]).any(axis=1))[0][:5]} differ from selterms_ref"
                assert ev.last_kernel == "selterms" and ev.last_pick == "none"
            i += 1


@pytest.mark.parametrize("keys", [2, PASS_KEYS + 1], ids=["narrow", "wide"])
def test_a_block_that_walks_more_than_one_pod_tile(ev, keys):
    """1024 column blocks leave two block rows for three pod tiles: the first block row walks two tiles, the second one"""
    n, p, T = 16 * 64 * 1024 - 37, 130, 2
    W = (n + 63) // 64
    gx = (W + CW * WAVES - 1) // (CW * WAVES)
    assert gx == 1024 and (2048 + gx - 1) // gx == 2 < (p + 63) // 64 == 3, "pod_tiles_per_block == 2"
    rng = np.random.default_rng([0xE10B, keys])
    lab = IDS[rng.integers(0, IDS.size, size=(keys, n))]
    sel = np.zeros((T, keys, p), dtype=np.uint32)
    sel[0, 0] = E(rng.choice([EQ, LT, AB], size=p), rng.integers(1, 6, size=p))
    sel[1, keys - 1] = E(rng.choice([EQ, GT, NE], size=p), rng.integers(1, 6, size=p))
    sel[1, 0, ::3] = E(EQ, 2)
    want = selterms_ref.selterms_mask(lab, sel)
    assert row_kinds(want, n)[2] >= p // 2
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), lab)
    got = eval_into_view(ev, sel, F(T), n, p, W, 1)
    assert np.array_equal(got, want), f"pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from selterms_ref"


def test_no_selectors_and_no_keys_pass_every_node(ev):
    full = selector_calls.no_selectors_and_no_keys_pass_every_node(ev, [call(3)], [call(15)], 0xE100, IDS)
    got = eval_into_view(ev, np.zeros((4, 0, 3), np.uint32), F(4), 65, 3, 2, 0)
    assert np.array_equal(got, full)


# ---- 2. agreement with what exists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,keys", [(1025, PASS_KEYS), (257, PASS_KEYS + 1), (65, 32)])
def test_one_term_is_the_tagged_call(ev, n, keys):
    k = case(n, keys)
    W = (n + 63) // 64
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    got = eval_into_view(ev, k["sel"][:1], F(1), n, P_MAX, W, 0)
    assert ev.last_kernel == "selterms"
    flat = eval_into_view(ev, k["sel"][0], F(1), n, P_MAX, W, 0)  # [1 * keys][p] is the same array
    tagged = eval_into_view(ev, k["sel"][0], TG, n, P_MAX, W, 0)
    assert ev.last_kernel == "seltag"
    assert row_kinds(tagged, n)[2] > P_MAX // 4
    assert np.array_equal(got, tagged) and np.array_equal(flat, tagged) and np.array_equal(got, k["want"][1])


@pytest.mark.parametrize("n,keys", [(1025, PASS_KEYS), (257, PASS_KEYS + 1), (65, 32)])
@pytest.mark.parametrize("T", [2, 3, MAX_TERMS])
def test_t_terms_are_a_tagged_call_and_t_minus_one_under_combine_or(ev, n, keys, T):
    import torch
    k = case(n, keys)
    W = (n + 63) // 64
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    got = eval_into_view(ev, k["sel"][:T], F(T), n, P_MAX, W, 0)
    M = torch.full((P_MAX, W), 0x5A, dtype=torch.int64, device=dev_of(ev))
    z = zeros_dev(ev, P_MAX)
    for t in range(T):
        ev.eval_device(z, z, to_dev(ev, k["sel"][t], np.int32), None, None, TG | (COMBINE_OR if t else 0), out_feasible=M)
        assert ev.last_kernel == "seltag"
    torch.cuda.synchronize()
    assert np.array_equal(got, k["want"][T]) and np.array_equal(got, mask_np(M))


@pytest.mark.parametrize("keys", [PASS_KEYS, PASS_KEYS + 1])
def test_never_padding_is_the_pods_own_term_count_and_a_zero_term_is_every_node(ev, keys):
    n, p = 1025, 129
    k = case(n, keys)
    W = (n + 63) // 64
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    rng = np.random.default_rng([0xE102, keys])
    own = rng.integers(1, 4, size=p)  # the pod's own term count, 1 .. 3
    real = np.array(k["sel"][:3])
    real[:, :, 1::8] = k["sel"][1:4, :, 1::8]  # (no all-zero terms here: they are the second half of this test)
    real[:, :, 5::8] = k["sel"][2:5, :, 5::8]
    padded = np.zeros((7, keys, p), dtype=np.uint32)
    padded[:3] = real
    for pod in range(p):
        padded[own[pod]:, :, pod] = 0
        padded[own[pod]:, rng.integers(0, keys), pod] = E(rng.choice([6, 7]), rng.integers(0, 1 << 29))  # any tag-6 / tag-7 entry, in any one key
    got = eval_into_view(ev, padded, F(7), n, p, W, 0)
    assert np.array_equal(got, selterms_ref.selterms_mask(k["lab"], padded))
    seen = 0
    for c in (1, 2, 3):
        at_c = eval_into_view(ev, real[:c], F(c), n, p, W, 0)
        mine = own == c
        assert np.array_equal(got[mine], at_c[mine]), f"pods of {c} terms, padded to 7, differ from the same pods in a call of {c} terms"
        seen += int(row_kinds(got[mine], n)[2])
    assert seen > p // 2
    # a leading all-zero term: the valid-bits row, whatever follows; and a zero term further back
    valid = selterms_ref.selterms_mask(k["lab"], None, p=p)
    for where in (0, 1, 6):
        z = padded.copy()
        z[where] = 0
        got = eval_into_view(ev, z, F(7), n, p, W + 1, 1)
        assert np.array_equal(got, valid), f"an all-zero term {where}"
    assert int(valid[0, -1]) == 1 and (valid[:, :-1] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


def test_timing_brackets_the_kernel(ev):
    n, keys = 1025, PASS_KEYS
    k = case(n, keys)
    ev.set_nodes(np.zeros(n, np.int64), np.zeros(n, np.int64), k["lab"])
    ev.set_timing(True)
    try:
        ev.kernel_time_ms()  # (reading the samples resets them)
        eval_into_view(ev, k["sel"][:3], F(3), n, P_MAX, ev.W, 0)
        ms, count = ev.kernel_time_ms()
        assert count == 1 and ms > 0, "one pair of stream events around the one launch"
    finally:
        ev.set_timing(False)


# ---- 3. combining and picks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comb,comb_id", COMBINES, ids=[c[1] for c in COMBINES])
def test_the_call_under_every_combine(ev, comb, comb_id):
    k = case(1025, PASS_KEYS + 1)
    selector_calls.the_call_under_every_combine(ev, call(3), k["lab"], k["sel"][:3], k["want"][3], comb, np.random.default_rng([0xE103, comb]))


_PICK_CASE = {}


def pick_case():
    if not _PICK_CASE:
        P, N, T = 300, 700, 3
        c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=0xE10B1C)
        rng = np.random.default_rng(0xE10B1)
        base = np.ascontiguousarray(c.pod_sel)
        assert base.max() < 1 << 29 or (base[base >= 1 << 29] == SEL_NEVER).all()
        sel = np.zeros((T,) + base.shape, dtype=np.uint32)
        for t in range(T):
            rolled = np.roll(base, 7 * t, axis=1)  # another pod's selectors: another term
            tags = rng.choice(6, size=base.shape, p=TAG_WEIGHTS)
            sel[t] = np.where((rolled != 0) & (rolled != SEL_NEVER), E(tags, rolled & 0x1FFFFFFF), rolled)
            sel[t, 0, np.nonzero(~(sel[t] != 0).any(axis=0))[0]] = E(EQ, 1)  # no all-zero term: every node would pass
        sel[:, 3, 1::9] = SEL_NEVER  # pods without a node
        old = pack_mask(rng.random((P, N)) < 0.4)
        draws = rng.integers(0, 1 << 32, size=(P, 5), dtype=np.uint64).astype(np.uint32)
        new = selterms_ref.selterms_mask(c.node_labels, sel)
        for a in (sel, old, draws, new):
            a.setflags(write=False)
        _PICK_CASE.update(c=c, sel=sel, old=old, draws=draws, new=new, T=T)
    return _PICK_CASE


@pytest.mark.parametrize("pick,last_pick", PICKS, ids=["sampled", "bestfit", "uniform", "spread", "pack"])
def test_a_pick_in_the_call_is_the_pick_from_the_resulting_mask(ev, pick, last_pick):
    k = pick_case()
    selector_calls.a_pick_in_the_call_is_the_pick_from_the_resulting_mask(ev, call(k["T"]), k, k["new"], pick, last_pick, options=((0, 1), (1, 1)))


@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
def test_the_recipe_end_to_end(ev, pitched):
    """(zone In {a, b} AND gpu Exists) OR (cores Gt 16), then KSCHED_FIT | KSCHED_COMBINE_AND | the spread pick: two calls, with
    node_affinity_rows producing the rows; a third of the pods have no affinity, some a single term"""
    import torch
    P, N = 200, 300
    c = synth.make_cluster(P, N, n_keys=8, n_taints=0, seed=0xE10C4A)
    c.req_mem[0] = 1 << 60  # pod 0 fits nowhere
    rng = np.random.default_rng(0xE10C4)
    keys = ["zone", "gpu", "cores"] + [f"k{i}" for i in range(3, c.n_keys)]
    zones = {"a": 1, "b": 2, "c": 3}
    lab = c.node_labels.copy()
    lab[0] = np.where(rng.random(N) < 0.1, 0, rng.integers(1, 4, N))
    lab[1] = np.where(rng.random(N) < 0.6, 1, 0)
    cores = np.array([4, 8, 16, 32, 64])[rng.integers(0, 5, N)]
    lab[2] = np.where(rng.random(N) < 0.1, 0, cores + 1)
    lab = lab.astype(np.uint32)
    recipe = [[("zone", "In", ["a", "b"]), ("gpu", "Exists", [])], [("cores", "Gt", ["16"])]]
    pods = [None if i % 3 == 0 else [recipe[1]] if i % 7 == 1 else recipe for i in range(P)]
    sel, T, overflow = node_affinity_rows(pods, keys, {"zone": zones, "gpu": {"true": 1}}, ["cores"])
    assert T == 3 and overflow == [] and sel.shape == (3, c.n_keys, P)
    # the label columns' answer, written out here
    zone_ab, gpu, more = (lab[0] == 1) | (lab[0] == 2), lab[1] != 0, (lab[2] != 0) & (lab[2].astype(np.int64) - 1 > 16)
    whole, second = (zone_ab & gpu) | more, more
    assert 0 < second.sum() < whole.sum() < N and ((lab[2] == 17) & ~(zone_ab & gpu)).any(), "a node with exactly 16 cores fails Gt 16"
    affinity = np.stack([np.ones(N, bool) if t is None else second if len(t) == 1 else whole for t in pods])
    fits = (c.req_cpu[:, None] <= c.avail_cpu[None, :]) & (c.req_mem[:, None] <= c.avail_mem[None, :])
    bits = fits & affinity
    assert P // 4 < bits.any(axis=1).sum() < P, "pods with a node and pods without one"
    want = pack_mask(bits)
    ev.set_nodes(c.avail_cpu, c.avail_mem, lab)
    cpu, mem = to_dev(ev, c.req_cpu, np.int64), to_dev(ev, c.req_mem, np.int64)
    draws = rng.integers(0, 1 << 32, size=(P, 3), dtype=np.uint64).astype(np.uint32)
    smp = to_dev(ev, draws, np.int32)
    M = ev.alloc_mask(P, pitched=pitched)
    M.fill_(-1)  # whatever the mask held before the chain
    out = fresh(ev, P, 4)
    ev.eval_device(cpu, mem, to_dev(ev, sel, np.int32), None, None, F(T), out_feasible=M)
    assert ev.last_kernel == "selterms"
    ev.eval_device(cpu, mem, None, None, smp, FIT | COMBINE_AND | PICK_SPREAD, out_feasible=M, out_binding=out[:P])
    alone = fresh(ev, P)
    ev.pick_device(to_dev(ev, want, np.int64), PICK_SPREAD, alone, samples=smp)
    torch.cuda.synchronize()
    got = mask_np(M)
    assert np.array_equal(got, want), f"pods {np.nonzero((got != want).any(axis=1))[0][:5]} differ from the label columns' answer"
    b = out.cpu().numpy()
    assert np.array_equal(b[:P], alone.cpu().numpy()) and (b[P:] == -7).all()
    assert ((b[:P] >= 0) == bits.any(axis=1)).all() and bits[np.nonzero(b[:P] >= 0)[0], b[:P][b[:P] >= 0]].all()


# ---- 4. the host forms --------------------------------------------------------------------------------------------------------------------------
def test_the_host_forms_give_the_device_forms_bits(ev):
    k = pick_case()
    selector_calls.the_host_forms_give_the_device_forms_bits(ev, call(k["T"]), k, k["new"], lo=37, p=150)


# ---- 5. snapshot changes ------------------------------------------------------------------------------------------------------------------------
def snapshot_case(seed, T=2):
    c = synth.make_cluster(129, 1100, n_keys=8, n_taints=0, seed=seed)
    rng = np.random.default_rng(seed)
    base = np.ascontiguousarray(c.pod_sel)
    sel = np.zeros((T,) + base.shape, dtype=np.uint32)
    for t in range(T):
        rolled = np.roll(base, 5 * t, axis=1)
        sel[t] = np.where((rolled != 0) & (rolled != SEL_NEVER), E(rng.choice(6, size=base.shape, p=TAG_WEIGHTS), rolled & 0x1FFFFFFF), rolled)
        sel[t, 0, np.nonzero(~(sel[t] != 0).any(axis=0))[0]] = E(EQ, 1)
    return c, sel, rng


def test_a_label_update_before_the_call(built):
    c, sel, rng = snapshot_case(0xE106)
    lab = c.node_labels.copy()
    n, p, T = c.N, c.P, sel.shape[0]
    W = (n + 63) // 64
    e = Evaluator(0)
    try:
        e.set_nodes(c.avail_cpu, c.avail_mem, lab)
        before = selterms_ref.selterms_mask(lab, sel)
        assert np.array_equal(eval_into_view(e, sel, F(T), n, p, W, 0), before)
        idx = rng.choice(n, size=200, replace=False).astype(np.uint32)
        rows = rng.integers(0, lab.max(axis=1)[:, None] + 1, size=(8, idx.size)).astype(np.uint32)
        lab[:, idx] = rows
        after = selterms_ref.selterms_mask(lab, sel)
        assert not np.array_equal(before, after), "the update shows in the mask"
        e.update_node_labels(idx, rows)
        assert np.array_equal(eval_into_view(e, sel, F(T), n, p, W, 0), after), "after the update"
        # another key count: eleven keys (the wide kernel) over other nodes
        k = case(1025, PASS_KEYS + 1)
        lab2 = np.concatenate([k["lab"], k["lab"][:2][:, ::-1]])
        sel2 = np.concatenate([k["sel"][:3], k["sel"][:3, :2]], axis=1)
        e.set_nodes(np.zeros(1025, np.int64), np.zeros(1025, np.int64), lab2)
        assert e.n_keys == 11
        want = selterms_ref.selterms_mask(lab2, sel2)
        got = eval_into_view(e, sel2, F(3), 1025, P_MAX, 17, 0)
        assert np.array_equal(got, want) and not np.array_equal(want, k["want"][3]), "after ksched_set_nodes with eleven keys"
    finally:
        e.close()


def test_two_streams_around_a_label_update(ev):
    c, sel, rng = snapshot_case(0xE107)
    selector_calls.two_streams_around_a_label_update(ev, call(sel.shape[0]), c, sel, rng)


# ---- 6. refusals and edge sizes -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_mask_and_bindings_untouched(ev):
    import torch
    c = synth.make_cluster(40, 130, n_keys=4, n_taints=4, seed=0xE10E44)
    ev.set_nodes(c.avail_cpu, c.avail_mem, c.node_labels, c.node_taints)
    P, W, T = c.P, ev.W, 2
    lib, h = _lib.load(), ev._h
    cpu, mem, sel1, tol = pod_tensors(ev, c)
    hsel = np.stack([np.ascontiguousarray(c.pod_sel), np.roll(np.ascontiguousarray(c.pod_sel), 3, axis=1)])
    sel = to_dev(ev, hsel, np.int32)
    smp = to_dev(ev, c.samples, np.int32)
    dM, dF = (torch.full((P, W), 0x5A5A5A5A, dtype=torch.int64, device=dev_of(ev)) for _ in range(2))
    dB = fresh(ev, P)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    K = sel_terms(T)
    f = TG | K
    st = C.c_void_p(torch.cuda.current_stream(ev.device).cuda_stream)

    def device(flags, feas, fit, bind, attempts=0, samples=None, p=P):
        return lib.ksched_eval_device_pitched(h, p, vp(cpu), vp(mem), vp(sel), vp(tol), vp(samples), attempts, flags, vp(feas), vp(fit), vp(bind), W, st)
    # the field without KSCHED_SELOP_TAGGED: no selector term, a plain call, an operator call -- hence without KSCHED_SEL, or beside an operator
    for rest in (0, FIT, SEL, FIT | SEL, FIT | SEL | TAINT, SEL | SELOP_EXISTS, SEL | SELOP_GT, SEL | SELOP_LT, SELOP_TAGGED):
        assert device(rest | K, dM, None, None) == _lib.E_INVAL, hex(rest)
        assert device(rest | K | PICK_UNIFORM, dM, None, dB, 5, smp) == _lib.E_INVAL, hex(rest)
    for op in (SELOP_EXISTS, SELOP_GT, SELOP_LT):
        assert device(f | op, dM, None, None) == _lib.E_INVAL
    for t in (1, MAX_TERMS):
        assert device(SEL | sel_terms(t), dM, None, None) == _lib.E_INVAL
    # fit, taints and a fit mask beside the field
    assert device(f | FIT, dM, None, None) == _lib.E_INVAL
    assert device(f | TAINT, dM, None, None) == _lib.E_INVAL
    assert device(f | FIT | TAINT | PICK_BESTFIT, dM, None, dB) == _lib.E_INVAL
    assert device(f | WANT_FIT_MASK, dM, dF, None) == _lib.E_INVAL
    assert device(f | WANT_FIT_MASK, dM, None, None) == _lib.E_INVAL
    assert device(f, dM, dF, None) == _lib.E_INVAL
    assert device(f | COMBINE_AND | FIT, dM, None, None) == _lib.E_INVAL
    # every refusal of a tagged, a plain or a combining call stays
    assert device(f, None, None, None) == _lib.E_INVAL, "nothing to write"
    assert device(f | COMBINE_OR, None, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_AND | COMBINE_OR, dM, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_SOFT, dM, None, None) == _lib.E_INVAL
    assert device(f | COMBINE_OR | COMBINE_SOFT, dM, None, None) == _lib.E_INVAL
    assert device(f | PICK_UNIFORM | PICK_SPREAD, dM, None, dB, 5, smp) == _lib.E_INVAL
    assert device(f | PICK_UNIFORM, dM, None, None, 5, smp) == _lib.E_INVAL, "a pick needs out_binding"
    for probe in (0x1000, 0x20000, 0x80000, 0x1000000):
        assert device(f | probe, dM, None, None) == _lib.E_INVAL and device(SEL | probe, dM, None, None) == _lib.E_INVAL, hex(probe) + " stays unknown"
    assert lib.ksched_eval_device(h, P, None, vp(mem), vp(sel), None, None, 0, f, vp(dM), None, None, st) == _lib.E_INVAL, "the requests stay required"
    assert lib.ksched_eval_device(h, P, vp(cpu), vp(mem), vp(sel), None, None, 0, SEL | K, vp(dM), None, None, st) == _lib.E_INVAL
    hM, hB = np.full((P, W), SENTINEL, np.uint64), np.full(P, -7, np.int32)
    for bad in (SEL | K, SELOP_TAGGED | K, f | SELOP_EXISTS, f | FIT, f | COMBINE_OR):
        assert lib.ksched_eval(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, None, 0, bad, hp(hM), None, None) == _lib.E_INVAL, hex(bad)
    dev_b, stream = C.c_void_p(), C.c_void_p()
    for bad in (SEL | K, f | SELOP_LT, f | TAINT, f | COMBINE_OR):
        assert lib.ksched_eval_begin(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), P, None, None, 0, bad, hp(hM), None, P, C.byref(dev_b), C.byref(stream)) == _lib.E_INVAL
        assert not dev_b.value
    assert lib.ksched_eval_begin(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), P - 1, None, None, 0, f, hp(hM), None, P, C.byref(dev_b), C.byref(stream)) == _lib.E_INVAL
    # the entry points that do not take the field
    table = torch.full((P, _lib.SUMMARY_WORDS), -7, dtype=torch.int32, device=dev_of(ev))
    htable = np.full((P, _lib.SUMMARY_WORDS), 7, np.uint32)
    pairs = np.zeros(1, np.uint32)
    reason = np.full(1, -7, np.int32)
    pipe = ev.pipe(2)
    try:
        for flags in (f | PICK_UNIFORM, FIT | SEL | K | PICK_UNIFORM, FIT | K | PICK_SAMPLED):
            assert lib.ksched_pipe_submit(pipe._h, 0, P, vp(cpu), vp(mem), vp(sel), None, vp(smp), 5, flags, vp(dM), W, vp(dB)) == _lib.E_INVAL
        assert pipe.slot_stream_handle(0) == 0, "nothing was enqueued on the slot"
    finally:
        pipe.close()
    for flags in (PICK_UNIFORM | K, PICK_UNIFORM | f):
        assert lib.ksched_pick(h, P, hp(hM), None, hp(c.samples), 5, flags, hp(hB)) == _lib.E_INVAL
        assert lib.ksched_pick_device(h, P, vp(dM), W, None, vp(smp), 5, flags, vp(dB), st) == _lib.E_INVAL
    for flags in (f, SEL | K, FIT | K):
        assert lib.ksched_summarize_device(h, P, vp(cpu), vp(mem), vp(sel), None, flags, vp(table), st) == _lib.E_INVAL
        assert lib.ksched_summarize(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, flags, hp(htable)) == _lib.E_INVAL
        assert lib.ksched_explain(h, P, hp(c.req_cpu), hp(c.req_mem), hp(hsel), None, 1, hp(pairs), hp(pairs), flags, hp(reason)) == _lib.E_INVAL
    # the Python face: ValueError before the library
    for call in (lambda: ev.eval_device(cpu, mem, sel, None, None, SEL | K, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, f | FIT, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, f | SELOP_GT, out_feasible=dM),
                 lambda: ev.eval_device(cpu, mem, sel, None, None, f, out_feasible=dM, out_fit=dF),
                 lambda: ev.eval_device(cpu, mem, sel1, None, None, f, out_feasible=dM),          # [n_keys, p] rows under T = 2: an out-of-bounds read
                 lambda: ev.eval_device(cpu, mem, sel, None, None, TG | sel_terms(3), out_feasible=dM),
                 lambda: ev.pick_device(dM, PICK_UNIFORM | K, dB, samples=smp),
                 lambda: ev.pick(hM, PICK_UNIFORM | K, samples=c.samples),
                 lambda: ev.summarize_device(cpu, mem, sel, None, SEL | K, out=table),
                 lambda: ev.summarize(c.req_cpu, c.req_mem, hsel, None, SEL | K),
                 lambda: ev.explain(c.req_cpu, c.req_mem, hsel, None, [0], [1], SEL | K),
                 lambda: ev.eval(c.req_cpu, c.req_mem, hsel, None, None, f | TAINT),
                 lambda: ev.eval(c.req_cpu, c.req_mem, hsel[0], None, None, f)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert (dM == 0x5A5A5A5A).all() and (dF == 0x5A5A5A5A).all() and (dB == -7).all() and (table == -7).all()
    assert (hM == SENTINEL).all() and (hB == -7).all() and (htable == 7).all() and (reason == -7).all()
    # p == 0: a no-op; field 0 beside what is legal today behaves as today; and the call itself works
    assert device(f | PICK_UNIFORM, dM, None, dB, 5, smp, p=0) == _lib.OK
    torch.cuda.synchronize()
    assert (dM == 0x5A5A5A5A).all() and (dB == -7).all()
    ev.eval_device(cpu, mem, sel1, tol, None, FIT | SEL | TAINT | sel_terms_zero(), out_feasible=dM)
    assert ev.last_kernel in ("direct", "fused")
    ev.eval_device(cpu, mem, sel1, None, None, TG, out_feasible=dF)
    assert ev.last_kernel == "seltag"
    torch.cuda.synchronize()
    assert np.array_equal(mask_np(dM), oracle_mask(c, FIT | SEL | TAINT))
    assert np.array_equal(mask_np(dF), seltag_ref.seltag_mask(c.node_labels, hsel[0]))
    ev.eval_device(cpu, mem, sel1, None, None, SEL | SELOP_EXISTS | COMBINE_ANDNOT, out_feasible=dF)
    assert ev.last_kernel == "selop"
    ev.eval_device(cpu, mem, sel, None, None, f, out_feasible=dF)
    torch.cuda.synchronize()
    assert ev.last_kernel == "selterms" and np.array_equal(mask_np(dF), selterms_ref.selterms_mask(c.node_labels, hsel))


def sel_terms_zero():
    """field 0: no term field"""
    return 0 << SEL_TERMS_SHIFT


def test_edge_sizes(built):
    def smallest(e):
        """the smallest call that does something: one pod, three terms of EQ 1 on nodes that all carry id 1"""
        r = e.eval(np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones((3, 2, 1), np.uint32), None, None, F(3))
        assert r.feasible.tolist() == [[0xFFFFFFFFFFFFFFFF, 0x3F]] and e.last_kernel == "selterms"
    selector_calls.edge_sizes(call(3), COMBINE_OR, smallest)
