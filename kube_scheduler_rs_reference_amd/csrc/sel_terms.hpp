// sel_terms.hpp -- the rules of a tagged call with a TERM COUNT (extension E10, include/ksched.h: KSCHED_SEL_TERMS), said once: the count a
// flag word names, which calls may carry one and with which other flags, where entry (term, key, pod) lies, one pod's row restated on the
// CPU, and the geometry of the kernel's one launch.
//
// A tagged call (E9, sel_tags.hpp) answers ONE conjunctive matchExpressions term per pod.  With a term count T in bits 20 .. 23 of the flag
// word the selector entries are [T][nkeys][p], and the pod's row is the OR over the T terms of the AND over the keys of seltag_pass: a
// required nodeAffinity (a list of ORed nodeSelectorTerms, `In` with several values expanded into terms) in one call and one mask.  A term
// of zeros passes everywhere; a term with one tag-6 / tag-7 entry (KSCHED_SEL_NEVER) passes nowhere -- the padding of a pod with fewer terms.
//
// Host-only on purpose, like sel_tags.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/selterms_plan_tests.cpp pins every rule at its boundary without a GPU.  check_eval_args (ksched_api.hip) asks
// check_selterms_args for every evaluation entry point; plan_eval (eval_plan.hpp) carries `terms` from EvalFacts to EvalPlan; launch_mask
// launches k_eval_selterms / k_eval_selterms_wide (kernels_selterms.hpp) through run_selector_mask (kernels_sel_walk.hpp) with what
// plan_selterms_launch says and takes no decision of its own.
#pragma once

#include <cstdint>

#include "../../include/ksched.h"
#include "sel_ops.hpp"
#include "sel_tags.hpp"

namespace ksched {

// the term count of a flag word: 0 = no term field (the call means what it means without E10), else 1 .. KSCHED_MAX_TERMS
constexpr uint32_t sel_terms(uint32_t flags) { return (flags & KSCHED_SEL_TERMS_MASK) >> KSCHED_SEL_TERMS_SHIFT; }
static_assert(sel_terms(KSCHED_SEL_TERMS(KSCHED_MAX_TERMS)) == KSCHED_MAX_TERMS && KSCHED_SEL_TERMS(KSCHED_MAX_TERMS) == KSCHED_SEL_TERMS_MASK,
              "the field holds exactly the counts 1 .. KSCHED_MAX_TERMS");

// The argument rules of a flag word that may carry a term count.  `accepted`: the entry point takes tagged calls (ksched_eval,
// ksched_eval_begin, ksched_eval_device, ksched_eval_device_pitched); ksched_pipe_submit passes false.  KSCHED_E_INVAL, with nothing
// enqueued:
//  * the field where it is not accepted;
//  * no KSCHED_SELOP_TAGGED: the field says how many tagged rows a pod has (so also: without KSCHED_SEL, or beside an operator flag of E8
//    -- check_seltag_args refuses those of a tagged call, and is asked here so that the answer does not depend on who is asked first);
//  * KSCHED_FIT, KSCHED_TAINT, KSCHED_WANT_FIT_MASK or out_fit: a tagged call's rule.
// A word without the field is KSCHED_OK here whatever the rest says.
constexpr int check_selterms_args(uint32_t flags, bool accepted, bool have_fit) {
    if (sel_terms(flags) == 0u) return KSCHED_OK;
    if (!accepted || !sel_tagged(flags)) return KSCHED_E_INVAL;
    return check_seltag_args(flags, accepted, have_fit);
}

// entry (term, k, pod) of [terms][nkeys][p] selector entries; `stride`: entries between consecutive columns (p, or ksched_eval_begin's sel_stride)
constexpr uint64_t selterms_index(uint32_t term, uint32_t k, uint32_t pod, uint32_t nkeys, uint64_t stride) {
    return ((uint64_t)term * nkeys + k) * stride + pod;
}
// how many columns of `stride` entries the host forms copy
constexpr uint32_t selterms_columns(uint32_t terms, uint32_t nkeys) { return (terms == 0u ? 1u : terms) * nkeys; }

// One pod's row: what the kernels compute, and what tests restate them against.  `lab` holds the label columns [nkeys][n], `sel` the
// entries [terms][nkeys][p]; `row` gets W = ceil(n / 64) words: bit (node % 64) of word (node / 64) is the OR over the terms of the AND over
// all keys of seltag_pass, the bits at or beyond n are zero.  sel == nullptr or nkeys == 0: every node passes.  terms == 1 IS seltag_row.
inline void selterms_row(const uint32_t *lab, const uint32_t *sel, uint32_t nkeys, uint32_t terms, uint32_t n, uint32_t p, uint32_t pod, uint64_t *row) {
    const uint32_t W = (uint32_t)(((uint64_t)n + 63u) / 64u);
    for (uint32_t w = 0; w < W; ++w) row[w] = 0;
    for (uint32_t node = 0; node < n; ++node) {
        bool any = !sel || nkeys == 0u;
        for (uint32_t t = 0; t < terms && !any; ++t) {
            bool ok = true;
            for (uint32_t k = 0; k < nkeys && ok; ++k) ok = seltag_pass(sel[selterms_index(t, k, pod, nkeys, p)], lab[(uint64_t)k * n + node]);
            any = ok;
        }
        if (any) row[node >> 6] |= 1ull << (node & 63u);
    }
}

// ---- the launch -----------------------------------------------------------------------------------------------------------------
// k_eval_seltag's geometry over the word columns and the pod tiles (plan_selop_launch: a wave on kSelopCW word columns, kSelopWaves waves
// a block, the pod tiles spread over about kSelopTargetBlocks blocks) -- but ONE launch whatever the key count.  The tagged kernel's key
// passes AND into the mask across launches; under an OR that is wrong ((A0 & A1) | (B0 & B1) is not (A0 | B0) & (A1 | B1)): a term's AND
// must be complete over all keys before it is ORed.  So a snapshot of more than kSelopKeys keys takes the WIDE kernel, which walks the
// `key_passes` inside the launch (kernels_selterms.hpp says how); up to kSelopKeys keys take the kernel that never leaves its registers.
struct SeltermsLaunch {
    uint32_t block = 64u * kSelopWaves;
    uint32_t gx = 0, gy = 0;  // gx == 0: nothing to launch
    uint32_t pod_tiles = 0, pod_tiles_per_block = 0;
    uint32_t key_passes = 0;  // max(1, ceil(nkeys / kSelopKeys)), walked INSIDE the one launch
    bool wide = false;        // key_passes > 1: k_eval_selterms_wide
    uint32_t terms = 0;
};

// p rows of W words, `terms` (>= 1) terms over `nkeys` keys that selectors constrain (0: none given, or a snapshot without keys)
constexpr SeltermsLaunch plan_selterms_launch(uint32_t p, uint32_t W, uint32_t nkeys, uint32_t terms) {
    SeltermsLaunch l;
    const SelopLaunch s = plan_selop_launch(p, W, nkeys);
    l.gx = s.gx, l.gy = s.gy, l.pod_tiles = s.pod_tiles, l.pod_tiles_per_block = s.pod_tiles_per_block;
    l.key_passes = s.passes;
    l.wide = s.passes > 1u;
    l.terms = nkeys == 0u ? 1u : terms;  // (without keys there is nothing to OR: one term of no key, the all-valid rows)
    return l;
}

}  // namespace ksched
