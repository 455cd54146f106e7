"""Constructed inputs that put the decisions of the mask, best-fit and summary kernels on their edges, and a plain reference.

Random inputs test a compare well where ties are heavy; they test it badly where a bug needs a coincidence with the STRUCTURE of a search:
a request exactly equal to the one element a search level holds, a winner inside the one window of cpu ranks that is tested individually,
a label id at the end of a tile's sorted list.  Every builder here returns a `Case`: node columns, pod columns and `cond`, a dict of INPUT
CONDITIONS it guarantees -- computed from the data, not asserted from intent (tests/test_knife_edges_host.py asserts them, and pins the
reference below against the oracle's scalar loops).

Pure numpy and Python integers: nothing here touches the library under test, the GPU or the oracle.

The reference
  fit[p, n]  = (req_cpu[p] <= cpu[n]) & (req_mem[p] <= mem[n]), broadcast on int64: a compare cannot overflow.
  sel[p, n]  = every key k the pod constrains (sel[k, p] != 0) carries exactly that id on the node (include/ksched.h: ids are exact; SEL_NEVER
               is carried by no node).
  taint[p,n] = (taints[n] & ~tol[p]) == 0.
  best fit   = the first feasible node in np.lexsort((node, cpu, mem)) order.  include/ksched.h defines the pick as the lexicographic minimum of
               (mem residual, cpu residual, node) over the feasible nodes; for a FIXED pod the residuals are avail - req with the same req for
               every node, so minimising them is minimising (mem, cpu, node) itself -- without forming a difference, which is why no
               128-bit arithmetic is needed here.  (The oracle forms the differences in __int128; the host test pins one against the other.)
  summary    = tests/summary_ref.counts_from_masks over the three term masks.
  sampled    = the first draw < N whose feasible bit is set, else -1.
  reasons    = check_node_validity's order: resources, then the selector, then the taint extension.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

FIT, SEL, TAINT = 0x01, 0x02, 0x04
SEL_NEVER = 0xFFFFFFFF
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TILE = 1024


@dataclass
class Case:
    name: str
    cpu: np.ndarray                      # [N] int64
    mem: np.ndarray                      # [N] int64
    req_cpu: np.ndarray                  # [P] int64
    req_mem: np.ndarray                  # [P] int64
    labels: Optional[np.ndarray] = None  # [K, N] uint32
    taints: Optional[np.ndarray] = None  # [N] uint64
    sel: Optional[np.ndarray] = None     # [K, P] uint32
    tol: Optional[np.ndarray] = None     # [P] uint64
    samples: Optional[np.ndarray] = None  # [P, 5] uint32 node indices
    pairs: Optional[np.ndarray] = None   # [M, 2] uint32 (pod, node) pairs for ksched_explain
    flags: int = FIT                     # the predicates this case is about
    cond: dict = field(default_factory=dict)
    extra: dict = field(default_factory=dict)

    @property
    def N(self) -> int:
        return int(self.cpu.shape[0])

    @property
    def P(self) -> int:
        return int(self.req_cpu.shape[0])

    def with_nodes(self, cpu=None, mem=None, labels=None, taints=None) -> "Case":
        """The same pods against changed node columns (what a snapshot update leaves behind)."""
        return Case(self.name, self.cpu if cpu is None else cpu, self.mem if mem is None else mem, self.req_cpu, self.req_mem,
                    self.labels if labels is None else labels, self.taints if taints is None else taints, self.sel, self.tol, self.samples,
                    self.pairs, self.flags, {}, self.extra)


# ---- the plain reference -----------------------------------------------------------------------------------------------------------------
def term_masks(c: Case, flags: int):
    """(F, S, T) as [P, N] bool; a predicate not in `flags` is all true."""
    P, N = c.P, c.N
    one = np.ones((P, N), dtype=bool)
    F = S = T = one
    if flags & FIT:
        F = (c.req_cpu[:, None] <= c.cpu[None, :]) & (c.req_mem[:, None] <= c.mem[None, :])
    if flags & SEL and c.sel is not None and c.labels is not None:
        S = one.copy()
        for k in range(c.labels.shape[0]):
            s = c.sel[k]
            rows = np.nonzero(s != 0)[0]
            if rows.size:
                S[rows] &= s[rows, None] == c.labels[k][None, :]
    if flags & TAINT and c.taints is not None:
        tol = c.tol if c.tol is not None else np.zeros(P, dtype=np.uint64)
        T = (c.taints[None, :] & ~tol[:, None]) == 0
    return F, S, T


def feasible(c: Case, flags: int) -> np.ndarray:
    F, S, T = term_masks(c, flags)
    return F & S & T


def pack(bits: np.ndarray) -> np.ndarray:
    """[P, N] bool -> [P, ceil(N / 64)] uint64, bit (node % 64) of word (node / 64), padding bits zero."""
    p, n = bits.shape
    W = (n + 63) // 64
    padded = np.zeros((p, W * 64), dtype=np.uint8)
    padded[:, :n] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(p, W)


def bestfit_order(c: Case) -> np.ndarray:
    return np.lexsort((np.arange(c.N), c.cpu, c.mem))  # ascending (mem, cpu, node)


def bestfit(c: Case, feas: np.ndarray) -> np.ndarray:
    order = bestfit_order(c)
    f = feas[:, order]
    first = f.argmax(axis=1)
    return np.where(f.any(axis=1), order[first], -1).astype(np.int32)


def sampled(feas: np.ndarray, samples: np.ndarray) -> np.ndarray:
    P, N = feas.shape
    out = np.full(P, -1, dtype=np.int32)
    rows = np.arange(P)
    for a in range(samples.shape[1] - 1, -1, -1):  # last draw first: an earlier feasible draw overwrites a later one
        d = samples[:, a].astype(np.int64)
        ok = d < N
        ok[ok] = feas[rows[ok], d[ok]]
        out[ok] = d[ok].astype(np.int32)
    return out


def counts(c: Case, flags: int) -> np.ndarray:
    from tests.summary_ref import counts_from_masks  # (its module imports the oracle's bridge; the function itself is plain popcounts)
    F, S, T = term_masks(c, flags)
    return counts_from_masks(pack(F), pack(S), pack(T), c.N)


def reasons(c: Case, flags: int, pairs: np.ndarray) -> np.ndarray:
    F, S, T = term_masks(c, flags)
    p, n = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    return np.where(~F[p, n], 1, np.where(~S[p, n], 2, np.where(~T[p, n], 3, 0))).astype(np.int32)


# ---- helpers of the builders -------------------------------------------------------------------------------------------------------------
def clip64(v: int) -> int:
    return min(max(int(v), I64_MIN), I64_MAX)


def triple(v: int):
    return [clip64(int(v) - 1), int(v), clip64(int(v) + 1)]


def i64(values) -> np.ndarray:
    return np.array([int(v) for v in values], dtype=np.int64)


def rank_below(values: np.ndarray, req: np.ndarray) -> np.ndarray:
    """index_tile_fit's rank, restated: #values < req"""
    return np.searchsorted(np.sort(values), req, side="left")


def eytzinger(sorted_vals: np.ndarray) -> np.ndarray:
    """csrc/tile_index.hpp, restated: slot k at level L = floor(log2 k), j = k - 2^L, holds sorted[(2j + 1) * 2^(9 - L) - 1]; slot 0 holds sorted[1023]."""
    tree = np.empty(TILE, dtype=np.int64)
    tree[0] = sorted_vals[TILE - 1]
    for level in range(10):
        j = np.arange(1 << level)
        tree[(1 << level) + j] = sorted_vals[((2 * j + 1) << (9 - level)) - 1]
    return tree


def descent(tree: np.ndarray, req: np.ndarray):
    """The ten-level descent for every request: (lc = #values among sorted[0..1022] below req, levels at which the request EQUALS the path's element)."""
    k = np.ones(req.shape[0], dtype=np.int64)
    hit = np.zeros((req.shape[0], 10), dtype=bool)
    for level in range(10):
        v = tree[k]
        hit[:, level] = v == req
        k = 2 * k + (v < req)
    return k - TILE, hit


# ---- fit_ranks -----------------------------------------------------------------------------------------------------------------------------
def _distinct_values(rng, salt: int):
    """1024 distinct int64 values over both signs: the two ends of the domain that a request can still step beyond by one, a run of small
    values two apart (v + 1 of one is v - 1 of the next), the rest wide."""
    small = [2 * i + 1 + salt for i in range(-11, 11)]
    vals = {I64_MIN, I64_MAX - 1, *small}
    while len(vals) < TILE:
        vals.add(int(rng.integers(-(1 << 62), 1 << 62)))
    return sorted(vals)


def fit_ranks() -> Case:
    rng = np.random.default_rng(20251)
    N = 2 * TILE + 1
    cpu, mem = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    # tile 0: 1024 distinct values per column, shuffled so that a value's position in the sorted order is not its node index
    vc, vm = _distinct_values(rng, 0), _distinct_values(rng, 100)
    cpu[:TILE] = i64(vc)[rng.permutation(TILE)]
    mem[:TILE] = i64(vm)[rng.permutation(TILE)]
    # tile 1: heavy ties.  cpu: sub-tile 3 all equal and below every other node, a unique maximum.  memory, the mirror: sub-tile 5 all equal and
    # above every other node, a unique minimum.
    t1 = np.arange(TILE, 2 * TILE)
    cpu[t1] = rng.choice(np.array([100, 200, 300, 400, 500, 600, 700, 800, 900, 1000], dtype=np.int64), TILE)
    mem[t1] = rng.choice(np.array([-40, -30, -20, -10, 0, 10, 20, 30, 40, 50], dtype=np.int64) << 20, TILE)
    cpu[TILE + 3 * 128:TILE + 4 * 128] = -50
    mem[TILE + 5 * 128:TILE + 6 * 128] = 1 << 40
    cpu[TILE + 77] = 10_000          # unique maximum (sub-tile 0)
    mem[TILE + 900] = -(1 << 40)     # unique minimum (sub-tile 7)
    # tile 2: one node, the largest value there is in both columns
    cpu[2 * TILE] = mem[2 * TILE] = I64_MAX

    node_of_c = {int(v): i for i, v in enumerate(cpu[:TILE])}
    node_of_m = {int(v): i for i, v in enumerate(mem[:TILE])}
    rc, rm, edge, below = [], [], [], []

    def add(c, m, e, b):
        rc.append(int(c)), rm.append(int(m)), edge.append(int(e)), below.append(int(b))

    for res, vals, node_of in ((0, vc, node_of_c), (1, vm, node_of_m)):
        for r, v in enumerate(vals):
            e, b = node_of[v], node_of[vals[max(r - 1, 0)]]
            for x in triple(v):
                add(x, I64_MIN, e, b) if res == 0 else add(I64_MIN, x, e, b)
    for res, col in ((0, cpu), (1, mem)):  # tile 1's distinct values
        vals = sorted({int(v) for v in col[t1]})
        for r, v in enumerate(vals):
            e = TILE + int(np.nonzero(col[t1] == v)[0][0])
            b = TILE + int(np.nonzero(col[t1] == vals[max(r - 1, 0)])[0][0])
            for x in triple(v):
                add(x, I64_MIN, e, b) if res == 0 else add(I64_MIN, x, e, b)
    for i in range(256):  # on an edge in both resources at once, at one node of tile 0
        n = int(rng.integers(0, TILE))
        add(clip64(int(cpu[n]) + (i % 3) - 1), clip64(int(mem[n]) + ((i // 3) % 3) - 1), n, (n + 1) % TILE)
    for x in (I64_MIN, I64_MAX):
        add(x, I64_MIN, 2 * TILE, 0)
        add(I64_MIN, x, 2 * TILE, 0)
    req_cpu, req_mem = i64(rc), i64(rm)
    P = req_cpu.shape[0]
    edge, below = np.array(edge, dtype=np.uint32), np.array(below, dtype=np.uint32)
    # draws: the node on the edge, the one just below it, one at random, one beyond the snapshot, and tile 2's node or a second random one -- in two orders
    smp = np.empty((P, 5), dtype=np.uint32)
    rnd = rng.integers(0, N, P).astype(np.uint32)
    even = (np.arange(P) % 2) == 0
    cols_a = np.stack([below, edge, np.full(P, 2 * TILE, dtype=np.uint32), rnd, np.full(P, N + 5, dtype=np.uint32)], axis=1)
    cols_b = np.stack([np.full(P, N, dtype=np.uint32), edge, rnd, below, rng.integers(0, 2 * TILE, P).astype(np.uint32)], axis=1)  # (no draw at tile 2: some find no node)
    smp[even], smp[~even] = cols_a[even], cols_b[~even]
    pods = np.arange(P, dtype=np.uint32)
    pairs = np.concatenate([np.stack([pods, edge], axis=1), np.stack([pods, below], axis=1)])
    c = Case("fit_ranks", cpu, mem, req_cpu, req_mem, samples=smp, pairs=pairs, flags=FIT)
    c.cond = fit_rank_conditions(c)
    return c


def fit_rank_conditions(c: Case) -> dict:
    out = {"pods": c.P, "nodes": c.N}
    for name, col, req, other in (("cpu", c.cpu, c.req_cpu, c.req_mem), ("mem", c.mem, c.req_mem, c.req_cpu)):
        t0 = col[:TILE]
        srt = np.sort(t0)
        out[f"{name}_tile0_distinct"] = int(np.unique(t0).size)
        out[f"{name}_position_is_not_index"] = int((np.argsort(t0, kind="stable") != np.arange(TILE)).sum())
        rank = rank_below(t0, req)
        out[f"{name}_ranks_answered"] = int(np.unique(rank).size)  # 1025 = every rank 0 .. 1024
        lc, hit = descent(eytzinger(srt), req)
        top = lc == TILE - 1
        out[f"{name}_lc1023_req_eq_max"] = int((top & (req == srt[-1])).sum())
        out[f"{name}_lc1023_req_above_max"] = int((top & (req > srt[-1])).sum())
        out[f"{name}_lc1023_req_below_max"] = int((top & (req < srt[-1])).sum())
        out[f"{name}_levels_with_req_on_path"] = int(hit.any(axis=0).sum())  # 10 = every level
        out[f"{name}_level_elements_hit"] = int(np.unique(req[hit.any(axis=1)]).size)
        # tile 1's cnt bytes: nodes of each sub-tile below the largest / smallest request that separates them
        t1 = col[TILE:2 * TILE].reshape(8, 128)
        out[f"{name}_tile1_unique_max"] = int((t1 == t1.max()).sum() == 1)
        out[f"{name}_tile1_unique_min"] = int((t1 == t1.min()).sum() == 1)
        lo = [s for s in range(8) if (t1[s] == t1[s][0]).all() and t1[s][0] < np.delete(t1, s, axis=0).min()]
        hi = [s for s in range(8) if (t1[s] == t1[s][0]).all() and t1[s][0] > np.delete(t1, s, axis=0).max()]
        out[f"{name}_tile1_subtile_all_below"] = lo
        out[f"{name}_tile1_subtile_all_above"] = hi
        for s in lo:  # a request just above the sub-tile's value: cnt byte of that sub-tile 128, every other 0
            out[f"{name}_pods_at_cnt_128_others_0"] = int((req == int(t1[s][0]) + 1).sum())
        for s in hi:  # a request equal to it: every other sub-tile's byte 128, this one 0
            out[f"{name}_pods_at_cnt_0_others_128"] = int((req == int(t1[s][0])).sum())
    out["pods_on_an_edge_in_both"] = int(((np.isin(c.req_cpu, c.cpu[:TILE]) | np.isin(c.req_cpu - 1, c.cpu[:TILE]) | np.isin(c.req_cpu + 1, c.cpu[:TILE]))
                                          & (np.isin(c.req_mem, c.mem[:TILE]) | np.isin(c.req_mem - 1, c.mem[:TILE]) | np.isin(c.req_mem + 1, c.mem[:TILE]))
                                          & (c.req_cpu != I64_MIN) & (c.req_mem != I64_MIN)).sum())
    out["tile2_node"] = (int(c.cpu[2 * TILE]), int(c.mem[2 * TILE]))
    return out


def rotate_tile0(c: Case):
    """One ksched_update_nodes that moves every value of tile 0 to the next node: the sorted values stay, every position changes.
    -> (node indices, new cpu, new mem, the case after the update)"""
    idx = np.arange(TILE, dtype=np.uint32)
    cpu, mem = c.cpu.copy(), c.mem.copy()
    cpu[:TILE], mem[:TILE] = np.roll(c.cpu[:TILE], 1), np.roll(c.mem[:TILE], 1)
    return idx, cpu[:TILE].copy(), mem[:TILE].copy(), c.with_nodes(cpu=cpu, mem=mem)


# ---- bestfit_window ------------------------------------------------------------------------------------------------------------------------
BF_SHAPES = ("mem_equal", "cpu_reversed", "quantised")


def bf_q(n: int) -> int:
    return (n + 255) // 256  # csrc/bestfit_layout.hpp bf_row_layout: q = ceil(n / levels), levels = 256


def bf_two_4096_blocks_n() -> int:
    """The smallest n whose sample arrays hold two blocks of 4096 (csrc/bestfit_layout.hpp bf_order_layout: n2 = ceil(n / 4096), and the sampled
    searches apply up to 64^3 nodes), restated; tests/test_knife_edges_host.py reads the same from the header's own arithmetic."""
    n = 1
    while (n + 4095) // 4096 < 2 or n > 64 ** 3:
        n += 1
    return n


def bestfit_window(n: int, shape: str) -> Case:
    rng = np.random.default_rng(n * 7 + BF_SHAPES.index(shape))
    q = bf_q(n)
    rc, rm = [], []
    if shape == "mem_equal":
        # all memory equal, cpu distinct: best-fit order = cpu order, the winner is the first node with cpu >= req -- at cpu rank r, inside the
        # window whenever r % q != 0
        cpu = (10 * rng.permutation(n) + 3).astype(np.int64)
        mem = np.full(n, 1000, dtype=np.int64)
        for j, v in enumerate(sorted(int(x) for x in cpu)):
            for x in triple(v):
                rc.append(x), rm.append(1000)
            rc.append(v), rm.append(999)
            if j % 8 == 0:  # one more than every node's memory: the memory search runs off the end
                rc.append(v), rm.append(1001)
        for x in triple(1000):
            rc.append(I64_MIN), rm.append(x)
            rc.append(int(cpu[0])), rm.append(x)
    elif shape == "cpu_reversed":
        # memory distinct, cpu in the reverse order: the feasible positions of (cpu of position j, mem of position s) are [s, j] -- `start` and the
        # cpu window meet at the winner when s == j
        pos = rng.permutation(n)  # best-fit position of node i
        mem = (7 * pos).astype(np.int64) - 7 * (n // 2)
        cpu = (11 * (n - 1 - pos) + 5).astype(np.int64) - 11 * (n // 3)
        for i in np.argsort(pos):
            for x in triple(int(cpu[i])):
                rc.append(x), rm.append(int(mem[i]))
            for x in triple(int(mem[i])):
                rc.append(int(cpu[i])), rm.append(x)
    elif shape == "quantised":
        # both columns take 7 values: the node index decides among equals.  cpu classes sized so that #cpu < c_k is 1 mod q for k >= 1: the window of
        # a request c_k then holds the q - 1 lowest-indexed nodes of the class, and those carry the lowest memory values, one each
        cv = [-3000, -7, 0, 9, 500, 501, 1 << 40]
        mv = [-(1 << 35), -1, 0, 1, 1 << 20, (1 << 20) + 2, 1 << 41]
        base = (n // 7) // q * q
        sizes = [base + 1] + [base] * 5
        sizes.append(n - sum(sizes))
        cls = np.repeat(np.arange(7), sizes)[rng.permutation(n)]
        cpu = i64(cv)[cls]
        mem = i64(mv)[rng.integers(0, 7, n)]
        for k in range(1, 7):
            first = np.nonzero(cls == k)[0][:min(q - 1, 7)]
            mem[first] = i64(mv)[:first.size]
        for v in cv:
            for x in triple(v):
                for m in mv:
                    rc.append(x), rm.append(m)
        for m in mv:
            for x in triple(m):
                for v in cv:
                    rc.append(v), rm.append(x)
    else:
        raise ValueError(shape)
    c = Case(f"bestfit_window-{n}-{shape}", cpu, mem, i64(rc), i64(rm), flags=FIT)
    c.cond = bestfit_window_conditions(c)
    return c


BF_ORDER_NODES = (1024, 2048, 2049, 4097)  # one run of the orders' merge sort, exactly two, two and a record, four and a record (three passes)


def bestfit_orders(n: int) -> Case:
    """A snapshot on which all three levels of the best-fit order and every merge of its sort decide something: avail_mem descends in node
    index, every value shared by the three nodes of a triple (the sorted runs of 1024 nodes come out in reverse, so each merge moves every
    record); avail_cpu descends inside a triple, (c + 1, c, c): the second and third node tie in both and the node index decides.  Two label
    keys, so that the snapshot has a bitmap index.  200 pods ask for exactly a triple's memory and for its c (-> the tied pair's first node),
    c + 1 (-> the triple's first node) or c + 2 (-> on to a triple further down the order)."""
    rng = np.random.default_rng(n)
    T = (n + 2) // 3
    t = np.arange(n) // 3
    c = 2 * rng.integers(0, 40, T)
    c[0] = 1000  # (the last triple of the order takes whatever fits nowhere else)
    mem = (5000 + (T - 1 - t)).astype(np.int64)
    cpu = (c[t] + (np.arange(n) % 3 == 0)).astype(np.int64)
    labels = np.stack([1 + np.arange(n) % 3, 1 + np.arange(n) % 5]).astype(np.uint32)
    P = 200
    tj = np.round(np.arange(P) * (T - 1) / (P - 1)).astype(np.int64)
    rc = c[tj] + np.array([0, 1, 0, 2])[np.arange(P) % 4]
    rm = 5000 + (T - 1 - tj)
    k = Case(f"bestfit_orders-{n}", cpu, mem, i64(rc), i64(rm), labels=labels, flags=FIT)
    k.cond = bestfit_orders_conditions(k)
    return k


def bestfit_orders_conditions(c: Case) -> dict:
    n = c.N
    win = bestfit(c, feasible(c, FIT))
    bound = win[win >= 0]
    order = bestfit_order(c)
    h = np.arange(0, n - 2, 3)  # the first node of every full triple
    sharers = np.unique(c.mem, return_counts=True, return_inverse=True)
    return {
        "distinct_nodes_bound": int(np.unique(bound).size),
        "unbound": int((win < 0).sum()),
        "bound_below_1024": int((bound < 1024).sum()),
        "bound_in_last_1024": int((bound >= n - 1024).sum()),
        "mem_descends_in_index": bool((np.diff(c.mem) <= 0).all()),
        "nodes_sharing_their_mem_with_two_others": int((sharers[2][sharers[1]] == 3).sum()),
        "full_triples": int(h.size),
        "triples_cpu_descending_with_a_tied_pair": int(((c.cpu[h] > c.cpu[h + 1]) & (c.cpu[h + 1] == c.cpu[h + 2])).sum()),
        "label_keys": int(c.labels.shape[0]),
        "order_is_not_index_order": int((order != np.arange(n)).sum()),
        "winners_by_place_in_triple": np.bincount(bound % 3, minlength=3).tolist(),
    }


def bestfit_window_conditions(c: Case) -> dict:
    n, q = c.N, bf_q(c.N)
    win = bestfit(c, feasible(c, FIT))
    bound = win >= 0
    by_cpu = np.lexsort((np.arange(n), c.cpu))  # ascending (cpu, node): csrc/ksched_api.hip build_bestfit, order 1
    cpurank = np.empty(n, dtype=np.int64)
    cpurank[by_cpu] = np.arange(n)
    r = np.searchsorted(c.cpu[by_cpu], c.req_cpu, side="left")  # #nodes with cpu below the request
    w = np.maximum(win, 0)
    in_window = bound & (cpurank[w] >= (r // q) * q) & (cpurank[w] < ((r + q - 1) // q) * q)
    exact = in_window & (c.cpu[w] == c.req_cpu)
    out = {"n": n, "q": q, "pods": c.P, "bound": int(bound.sum()), "unbound_share": float((~bound).mean()),
           "winner_in_window_cpu_eq_req_share_of_bound": float(exact.sum() / max(int(bound.sum()), 1)),
           "winner_in_window_share_of_bound": float(in_window.sum() / max(int(bound.sum()), 1))}
    # block ends of the searched arrays: bf_mem (memory in best-fit order) and cpu_sorted; blocks of 8^k and of 64 / 4096
    reqs = {"mem": set(int(x) for x in c.req_mem), "cpu": set(int(x) for x in c.req_cpu)}
    arrays = {"mem": np.sort(c.mem), "cpu": np.sort(c.cpu)}
    for b in (8, 64, 512, 4096):
        if n <= b:
            continue
        for name in ("mem", "cpu"):
            ends = arrays[name][b - 1::b]  # the last element of every whole block
            missing = [int(e) for e in ends if not {clip64(int(e) - 1), int(e), clip64(int(e) + 1)} <= reqs[name]]
            out[f"block{b}_{name}_ends"] = int(ends.size)
            out[f"block{b}_{name}_ends_without_a_triple"] = len(missing)
    return out


def swap_window_cpu(c: Case):
    """An update that exchanges the cpu of neighbouring cpu ranks inside windows (ranks 1 and 2 of every q ranks): the best-fit order, the window's
    members and the winners move.  -> (node indices, new cpu, new mem, the case after the update)"""
    n, q = c.N, bf_q(c.N)
    by_cpu = np.lexsort((np.arange(n), c.cpu))
    a = by_cpu[1:n - 1:q][: (n - 2) // q]
    b = by_cpu[2:n:q][: a.size]
    cpu = c.cpu.copy()
    cpu[a], cpu[b] = c.cpu[b], c.cpu[a]
    idx = np.concatenate([a, b]).astype(np.uint32)
    return idx, cpu[idx].copy(), c.mem[idx].copy(), c.with_nodes(cpu=cpu)


# ---- selector_ids --------------------------------------------------------------------------------------------------------------------------
def selector_ids() -> Case:
    rng = np.random.default_rng(77)
    N = TILE + 1
    lab = np.zeros((3, N), dtype=np.uint32)
    lab[0] = rng.integers(0, 6, N)                 # a row key: ids 1 .. 5, 0 = absent
    lab[0, :6] = np.arange(6)
    ids1 = (0x80000000 + 3 * rng.permutation(N)).astype(np.uint32)  # a list key, every id with bit 31 set, one node each
    lab[1] = ids1
    absent = np.array([5, 300, 1000], dtype=np.int64)  # ... but for three nodes of tile 0 that do not carry the key
    lab[1, absent] = 0
    card = 40
    ids2 = (1000 * (1 + np.arange(card))).astype(np.uint32)  # a list key of cardinality 40, ids spread: ~25 nodes per id and tile
    lab[2] = ids2[rng.integers(0, card, N)]
    lab[2, TILE] = ids2[7]

    cls, s0, s1, s2 = [], [], [], []

    def add(name, a=0, b=0, c=0):
        cls.append(name), s0.append(a), s1.append(b), s2.append(c)

    for v in (5, 6, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, SEL_NEVER):
        add(f"row:{v:#x}", a=v)
    for t in range(2):
        present = np.sort(lab[1, t * TILE:min(N, (t + 1) * TILE)])
        present = present[present != 0]
        add(f"list:first-of-tile{t}", b=int(present[0]))
        add(f"list:last-of-tile{t}", b=int(present[-1]))
    allp = np.sort(lab[1][lab[1] != 0])
    add("list:absent-between", b=int(allp[10]) + 1)
    add("list:absent-between", b=int(allp[-2]) + 2)
    for i in absent:  # the ids the three keyless nodes would have carried: absent, between two present ones
        add("list:absent-between", b=int(ids1[i]))
    add("list:below-smallest", b=int(allp[0]) - 1)
    add("list:above-largest", b=int(allp[-1]) + 1)
    add("list:above-largest", b=int(allp[-1]) + 3)
    add("list:0x7fffffff", b=0x7FFFFFFF)
    add("list:0xfffffffe", b=0xFFFFFFFE)
    add("list:never", b=SEL_NEVER)
    for i in rng.choice(N, 40, replace=False):
        add("list:present", b=int(ids1[i])) if lab[1, i] else add("list:absent-between", b=int(ids1[i]))
    for v in ids2:
        add("list2:present", c=int(v))
    for v in (999, 1001, 40_001, int(ids2[-1]) + 1, 0x80000000, 0xFFFFFFFE, SEL_NEVER):
        add("list2:absent", c=v)
    for i in rng.choice(N, 40, replace=False):  # combinations over the three keys, taken from a node: feasible by construction
        add("combined:feasible", a=int(lab[0, i]), b=int(lab[1, i]), c=int(lab[2, i]))
    for i in rng.choice(N, 20, replace=False):
        add("combined:one-key-off", a=int(lab[0, i]), b=int(lab[1, i]), c=int(ids2[(np.nonzero(ids2 == lab[2, i])[0][0] + 1) % card]))
    P = len(cls)
    sel = np.array([s0, s1, s2], dtype=np.uint64).astype(np.uint32)
    # resources: every node holds every pod but for a band, so that best fit has a choice and the fit term is live
    cpu = rng.integers(0, 64, N).astype(np.int64) * 250
    mem = rng.integers(1, 64, N).astype(np.int64) << 28
    req_cpu = np.where(np.arange(P) % 4 == 0, 4000, 0).astype(np.int64)
    req_mem = np.full(P, 1 << 28, dtype=np.int64)
    pods = np.arange(P, dtype=np.uint32)
    pairs = np.concatenate([np.stack([pods, rng.integers(0, N, P).astype(np.uint32)], axis=1),
                            np.stack([pods, np.full(P, TILE, dtype=np.uint32)], axis=1)])
    c = Case("selector_ids", cpu, mem, req_cpu, req_mem, labels=lab, sel=sel, pairs=pairs, flags=FIT | SEL, extra={"classes": cls})
    # ... and a pair per pod with a node the selector accepts, where there is one
    S = term_masks(c, SEL)[1]
    has = S.any(axis=1)
    c.pairs = np.concatenate([pairs, np.stack([pods[has], S[has].argmax(axis=1).astype(np.uint32)], axis=1)])
    c.cond = selector_conditions(c)
    return c


def selector_conditions(c: Case) -> dict:
    S = term_masks(c, SEL)[1]
    any_node = S.any(axis=1)
    out = {"pods": c.P, "ids_with_bit31_on_nodes": int((c.labels[1] >> 31).sum()), "key1_absent_nodes": int((c.labels[1] == 0).sum())}
    per = {}
    for name, ok in zip(c.extra["classes"], any_node):
        f = per.setdefault(name, [0, 0])
        f[0 if ok else 1] += 1
    out["classes"] = per  # class -> [pods with a node the selector accepts, pods without]
    # key 2's ranges per tile: entries of the tile's sorted list carrying one id
    runs = [int((c.labels[2, :TILE] == v).sum()) for v in np.unique(c.labels[2])]
    out["key2_cardinality"], out["key2_shortest_run_tile0"], out["key2_longest_run_tile0"] = len(runs), min(runs), max(runs)
    return out


def relabel(c: Case):
    """A ksched_update_node_labels that moves one node's key-1 id to the largest present id plus 3 and sets another node's key-1 id to 0.
    -> (node indices, [3][2] new label ids, the case after the update)"""
    lab = c.labels.copy()
    a, b = 17, 600
    lab[1, a] = np.uint32(int(c.labels[1].max()) + 3)
    lab[1, b] = 0
    idx = np.array([a, b], dtype=np.uint32)
    return idx, np.ascontiguousarray(lab[:, idx]), c.with_nodes(labels=lab)


# ---- taint_bits ----------------------------------------------------------------------------------------------------------------------------
TAINT_BITS = (0, 3, 4, 59, 60, 63)


def taint_bits() -> Case:
    rng = np.random.default_rng(99)
    N = TILE + 1
    bits = np.array([1 << b for b in TAINT_BITS], dtype=np.uint64)
    pick = rng.random((N, len(bits))) < 0.3
    pick[:len(bits) + 2] = False
    for i in range(len(bits)):
        pick[i, i] = True                 # one node per single bit
    pick[len(bits)] = True                # one node with all six
    pick[TILE] = [True, False, False, False, False, True]  # the lone node of the second tile: bits 0 and 63
    taints = (pick * bits[None, :]).sum(axis=1, dtype=np.uint64)
    tol = [0, 0xFFFFFFFFFFFFFFFF]
    for i in rng.choice(N, 60, replace=False).tolist() + list(range(len(bits) + 1)) + [TILE]:
        t = int(taints[i])
        tol.append(t)                     # exactly a node's set
        for b in TAINT_BITS:
            if t >> b & 1:
                tol.append(t & ~(1 << b))  # ... less one bit
    tol = np.array(tol, dtype=np.uint64)
    P = tol.shape[0]
    cpu = rng.integers(1, 64, N).astype(np.int64) * 250
    mem = rng.integers(1, 64, N).astype(np.int64) << 28
    req_cpu = np.where(np.arange(P) % 3 == 0, 8000, 250).astype(np.int64)
    req_mem = np.full(P, 1 << 28, dtype=np.int64)
    smp = rng.integers(0, N + 3, (P, 5)).astype(np.uint32)
    smp[:, 1] = TILE
    c = Case("taint_bits", cpu, mem, req_cpu, req_mem, taints=taints, tol=tol, samples=smp, flags=FIT | TAINT)
    T = term_masks(c, TAINT)[2]
    used = int(np.bitwise_or.reduce(taints))
    c.cond = {"pods": P, "taint_bits_in_use": [b for b in range(64) if used >> b & 1], "groups": (used.bit_length() + 3) // 4,
              "pods_tolerating_every_node": int(T.all(axis=1).sum()), "pods_tolerating_no_tainted_node": int((T == (taints == 0)[None, :]).all(axis=1).sum()),
              "pods_one_bit_short_of_a_node": int(((~T) & (np.bitwise_count(taints[None, :] & ~tol[:, None]) == 1)).any(axis=1).sum())
              if hasattr(np, "bitwise_count") else -1}
    return c


# ---- exact_fill ----------------------------------------------------------------------------------------------------------------------------
def exact_fill():
    """avail = k_n * r per resource with k_n in 0 .. 3; pod i < N requests exactly (r, r') and draws node i five times, so a sampled pick binds it
    there while the node still holds one more request; 16 further pods request zero and draw node 0, which holds exactly zero from the start.
    One round = evaluate, apply the bindings with FIRST_PER_NODE: every node with something left loses exactly one request.
    -> (case, k [N], r, r')"""
    rng = np.random.default_rng(5)
    N = TILE + 1
    r, r2 = 1_000_003, (1 << 33) + 7
    k = rng.integers(0, 4, N)
    k[:4], k[TILE] = [0, 1, 2, 3], 3
    cpu, mem = i64([int(x) * r for x in k]), i64([int(x) * r2 for x in k])
    P = N + 16
    req_cpu, req_mem = np.full(P, r, dtype=np.int64), np.full(P, r2, dtype=np.int64)
    req_cpu[N:] = 0
    req_mem[N:] = 0
    smp = np.repeat(np.arange(P, dtype=np.uint32)[:, None], 5, axis=1)
    smp[N:] = np.array([N + 1, 0, 0, 0, 0], dtype=np.uint32)
    c = Case("exact_fill", cpu, mem, req_cpu, req_mem, samples=smp, flags=FIT)
    c.cond = {"pods": P, "zero_request_pods": int(((req_cpu == 0) & (req_mem == 0)).sum()), "nodes_by_k": [int((k == j).sum()) for j in range(4)],
              "node0": (int(cpu[0]), int(mem[0]))}
    return c, k, r, r2


def exact_fill_after(k, r: int, r2: int, rounds: int):
    """The columns after `rounds` rounds, by Python integers."""
    left = [max(int(x) - rounds, 0) for x in k]
    return i64([x * r for x in left]), i64([x * r2 for x in left])
