"""The constructed inputs of tests/knife_edges.py really sit on the edges they aim at (every builder's input conditions, computed from its
data), and the plain numpy reference they are checked against on the GPU equals the oracle's scalar loops on every one of them: mask, fit
mask, best-fit bindings (the oracle minimises __int128 residuals; the reference takes the first feasible node in (mem, cpu, node) order),
sampled bindings, summary counts.  No GPU, and the library under test is not called: the rank conditions use index_tile_fit's definition,
#values < req, restated in numpy."""
import os
import re

import numpy as np
import pytest

from oracle import capi
from tests import knife_edges as ke
from tests import summary_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICK_SAMPLED, PICK_BESTFIT, WANT_FIT_MASK = 0x08, 0x10, 0x20
BF_NODES = (1025, ke.bf_two_4096_blocks_n())


def pin_against_the_oracle(c, flag_sets):
    """mask, fit mask, best-fit and sampled bindings and the summary counts of the plain reference == the oracle's"""
    for flags in flag_sets:
        F, S, T = ke.term_masks(c, flags)
        feas = F & S & T
        m, fit, bf = capi.eval_encoded(c.cpu, c.mem, c.labels, c.taints, c.req_cpu, c.req_mem, c.sel, c.tol, None, flags | PICK_BESTFIT | WANT_FIT_MASK)
        assert np.array_equal(ke.pack(feas), m), (c.name, flags, "mask")
        assert np.array_equal(ke.pack(F), fit), (c.name, flags, "fit mask")
        got = ke.bestfit(c, feas)
        assert np.array_equal(got, bf), (c.name, flags, "best fit", int((got != bf).sum()))
        if c.samples is not None:
            sb = capi.eval_encoded(c.cpu, c.mem, c.labels, c.taints, c.req_cpu, c.req_mem, c.sel, c.tol, c.samples, flags | PICK_SAMPLED, want_mask=False)[2]
            assert np.array_equal(ke.sampled(feas, c.samples), sb), (c.name, flags, "sampled")
        want = summary_ref.expected_counts(c.cpu, c.mem, c.labels, c.taints, c.req_cpu, c.req_mem, c.sel, c.tol, flags)
        assert np.array_equal(ke.counts(c, flags), want), (c.name, flags, "summary")


def test_fit_ranks_conditions_and_reference():
    c = ke.fit_ranks()
    k = c.cond
    print(k)
    assert c.N == 2049 and 6000 <= c.P <= 7000
    for res in ("cpu", "mem"):
        assert k[f"{res}_tile0_distinct"] == 1024 and k[f"{res}_position_is_not_index"] >= 1000
        assert k[f"{res}_ranks_answered"] == 1025, "every rank 0 .. 1024 of tile 0 is some pod's answer"
        assert k[f"{res}_lc1023_req_eq_max"] >= 1 and k[f"{res}_lc1023_req_above_max"] >= 1 and k[f"{res}_lc1023_req_below_max"] >= 1
        assert k[f"{res}_levels_with_req_on_path"] == 10 and k[f"{res}_level_elements_hit"] >= 1023
    assert k["cpu_tile1_unique_max"] == 1 and k["mem_tile1_unique_min"] == 1
    assert k["cpu_tile1_subtile_all_below"] == [3] and k["mem_tile1_subtile_all_above"] == [5]
    assert k["cpu_pods_at_cnt_128_others_0"] >= 1 and k["mem_pods_at_cnt_0_others_128"] >= 1
    assert k["pods_on_an_edge_in_both"] >= 256
    assert k["tile2_node"] == (ke.I64_MAX, ke.I64_MAX)
    assert int(c.cpu[:1024].min()) == ke.I64_MIN and int(c.cpu[:1024].max()) == ke.I64_MAX - 1
    assert int(c.mem[:1024].min()) == ke.I64_MIN and int(c.mem[:1024].max()) == ke.I64_MAX - 1
    assert not np.array_equal(np.argsort(c.cpu[:1024]), np.argsort(c.mem[:1024]))  # two permutations
    pin_against_the_oracle(c, [ke.FIT])
    # the rotation keeps the sorted values and moves every one of them
    idx, ncpu, nmem, c2 = ke.rotate_tile0(c)
    assert np.array_equal(np.sort(c2.cpu[:1024]), np.sort(c.cpu[:1024])) and (c2.cpu[:1024] != c.cpu[:1024]).all() and (c2.mem[:1024] != c.mem[:1024]).all()
    assert ke.fit_rank_conditions(c2)["cpu_ranks_answered"] == 1025
    pin_against_the_oracle(c2, [ke.FIT])
    # the explain pairs name both outcomes, the draws reach all three tiles
    r = ke.reasons(c, ke.FIT, c.pairs)
    assert (r == 0).sum() > 2000 and (r == 1).sum() > 2000
    assert all(((c.samples // 1024) == t).any() for t in (0, 1, 2)) and (c.samples >= c.N).any()


def test_the_two_block_node_count_is_the_layout_headers():
    """bf_order_layout's n2 and `sampled` rule, read from the header, give the node count the best-fit cases use (expected: 4097)."""
    src = open(os.path.join(ROOT, "kube_scheduler_rs_reference_amd", "csrc", "bestfit_layout.hpp")).read()
    n2 = re.search(r"l\.n2 = \(n \+ (\d+)u\) / (\d+)u;", src)
    sampled = re.search(r"l\.sampled = n <= (\d+)u \* (\d+)u \* (\d+)u;", src)
    levels = re.search(r"uint32_t levels = (\d+), q = 1;", src)
    assert n2 and sampled and levels
    block = int(n2.group(2))
    assert int(n2.group(1)) == block - 1
    limit = int(sampled.group(1)) * int(sampled.group(2)) * int(sampled.group(3))
    n = next(n for n in range(1, limit + 1) if (n + block - 1) // block >= 2)
    assert n == ke.bf_two_4096_blocks_n() == 4097 and n <= limit
    assert int(levels.group(1)) == 256 and ke.bf_q(1025) == 5 and ke.bf_q(4097) == 17


@pytest.mark.parametrize("shape", ke.BF_SHAPES)
@pytest.mark.parametrize("n", BF_NODES)
def test_bestfit_window_conditions_and_reference(n, shape):
    c = ke.bestfit_window(n, shape)
    k = c.cond
    print(c.name, k)
    assert k["winner_in_window_cpu_eq_req_share_of_bound"] >= 0.25, k
    assert k["unbound_share"] >= 0.01, k
    for b in (8, 64, 512, 4096):
        if n > b:
            for res in ("mem", "cpu"):
                assert k[f"block{b}_{res}_ends"] >= 1 and k[f"block{b}_{res}_ends_without_a_triple"] == 0, (b, res, k)
    assert ("block4096_mem_ends" in k) == (n > 4096)
    pin_against_the_oracle(c, [ke.FIT])
    idx, ncpu, nmem, c2 = ke.swap_window_cpu(c)
    assert idx.size >= 2 * (n // ke.bf_q(n)) - 4 and np.unique(idx).size == idx.size
    k2 = ke.bestfit_window_conditions(c2)
    if shape != "quantised":  # (equal values swap into themselves there)
        assert (c2.cpu != c.cpu).sum() == idx.size
        assert (ke.bestfit(c2, ke.feasible(c2, ke.FIT)) != ke.bestfit(c, ke.feasible(c, ke.FIT))).sum() > 0
    assert k2["winner_in_window_share_of_bound"] > 0
    pin_against_the_oracle(c2, [ke.FIT])


@pytest.mark.parametrize("n", ke.BF_ORDER_NODES)
def test_bestfit_orders_conditions_and_reference(n):
    c = ke.bestfit_orders(n)
    k = c.cond
    print(c.name, k)
    assert c.N == n and c.P == 200 and k["label_keys"] == 2
    assert k["distinct_nodes_bound"] >= 150 and k["unbound"] == 0
    assert k["bound_below_1024"] >= 1 and k["bound_in_last_1024"] >= 1
    # memory descends in node index, every value shared by three nodes (the last one by n % 3 when that is not 0) ...
    assert k["mem_descends_in_index"] and k["nodes_sharing_their_mem_with_two_others"] == n - n % 3 and k["full_triples"] == n // 3
    # ... cpu descends inside every triple, whose last two nodes tie in both columns
    assert k["triples_cpu_descending_with_a_tied_pair"] == n // 3
    assert k["order_is_not_index_order"] >= n - 3
    # winners are first nodes of a triple (cpu decided) and first nodes of a tied pair (the index decided), never the pair's second node
    w = k["winners_by_place_in_triple"]
    assert w[0] >= 40 and w[1] >= 40 and w[2] == 0, w
    pin_against_the_oracle(c, [ke.FIT])


def test_selector_ids_conditions_and_reference():
    c = ke.selector_ids()
    k = c.cond
    print(k)
    assert c.N == 1025 and c.labels.shape[0] == 3
    assert k["ids_with_bit31_on_nodes"] == 1025 - 3 and k["key1_absent_nodes"] == 3
    assert int(c.labels[0].max()) == 5 and 38 <= k["key2_cardinality"] <= 41 and k["key2_shortest_run_tile0"] > 8
    cl = k["classes"]
    for name in ("row:0x5", "list:first-of-tile0", "list:last-of-tile0", "list:first-of-tile1", "list:last-of-tile1", "list:present", "list2:present",
                 "combined:feasible"):
        assert cl[name][0] >= 1, (name, cl[name])  # a node the selector accepts
    for name in ("row:0x6", "row:0x7fffffff", "row:0x80000000", "row:0xfffffffe", "row:0xffffffff", "list:absent-between", "list:below-smallest",
                 "list:above-largest", "list:0x7fffffff", "list:0xfffffffe", "list:never", "list2:absent"):
        assert cl[name][0] == 0 and cl[name][1] >= 1, (name, cl[name])  # none: that is what the id means
    assert cl["combined:one-key-off"][1] >= 10
    assert cl["list:absent-between"][1] >= 5
    pin_against_the_oracle(c, [ke.SEL, ke.FIT | ke.SEL])
    r = ke.reasons(c, ke.FIT | ke.SEL, c.pairs)
    assert all((r == x).sum() >= 5 for x in (0, 1, 2))
    idx, lab, c2 = ke.relabel(c)
    assert int(c2.labels[1].max()) == int(c.labels[1].max()) + 3 and (c2.labels[1] == 0).sum() == 4 and lab.shape == (3, 2)
    assert (ke.term_masks(c2, ke.SEL)[1] != ke.term_masks(c, ke.SEL)[1]).any()
    pin_against_the_oracle(c2, [ke.FIT | ke.SEL])


def test_taint_bits_conditions_and_reference():
    c = ke.taint_bits()
    k = c.cond
    print(k)
    assert c.N == 1025 and k["taint_bits_in_use"] == [0, 3, 4, 59, 60, 63] and k["groups"] == 16
    assert int(c.taints.max()) >> 63 == 1
    assert k["pods_tolerating_every_node"] >= 1 and k["pods_tolerating_no_tainted_node"] >= 1 and k["pods_one_bit_short_of_a_node"] >= 50
    assert (c.tol == 0).any() and (c.tol == np.uint64(0xFFFFFFFFFFFFFFFF)).any() and np.isin(c.tol, c.taints).sum() >= 60
    pin_against_the_oracle(c, [ke.TAINT, ke.FIT | ke.TAINT])


def test_exact_fill_rounds_by_python_integers():
    c, kk, r, r2 = ke.exact_fill()
    print(c.cond)
    assert c.N == 1025 and c.cond["zero_request_pods"] == 16 and min(c.cond["nodes_by_k"]) >= 100 and c.cond["node0"] == (0, 0)
    cpu, mem = c.cpu, c.mem
    for j in range(1, 4):
        cj = c.with_nodes(cpu=cpu, mem=mem)
        pin_against_the_oracle(cj, [ke.FIT])
        feas = ke.feasible(cj, ke.FIT)
        b = ke.sampled(feas, c.samples)
        live = np.array([int(x) >= j for x in kk])
        assert np.array_equal(b[:c.N] >= 0, live) and (b[:c.N][live] == np.arange(c.N)[live]).all()  # every node with something left gets its pod
        assert (b[c.N:] == 0).all()  # the zero requests land on node 0, which holds exactly zero
        # FIRST_PER_NODE: per node the lowest pod index; pods beyond the first add nothing here (zero requests), so the subtraction is one request per live node
        cpu, mem = ke.exact_fill_after(kk, r, r2, j)
        assert np.array_equal(cpu, np.where(live, cj.cpu - r, cj.cpu)) and np.array_equal(mem, np.where(live, cj.mem - r2, cj.mem))
        after = ke.feasible(c.with_nodes(cpu=cpu, mem=mem), ke.FIT)
        gone = np.array([int(x) <= j for x in kk])
        assert not after[:c.N][:, gone].any(), "a node with k_n <= j has left every requesting pod's mask"
        assert after[c.N:].all(), "a zero request still fits every node, the ones at exactly zero included"
    assert not cpu.any() and not mem.any()
