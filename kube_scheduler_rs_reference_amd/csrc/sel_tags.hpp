// sel_tags.hpp -- the rules of a TAGGED call (extension E9, include/ksched.h: KSCHED_SELOP_TAGGED), said once: which calls may carry the flag
// and with which other flags, how a selector entry splits into a tag and an id, the rule for one (entry, node id) pair, the one compare form
// the kernel reduces every tag to, one pod's row restated on the CPU, and the geometry of the kernel's launches.
//
// Under an operator flag of E8 (sel_ops.hpp) the operator belongs to the CALL: every constrained entry of every pod is read under it, so a
// batch whose pods use different operators takes one evaluation per operator over the whole pods x nodes rectangle, and a negated expression
// (NotIn, DoesNotExist) a call of its own.  Under KSCHED_SELOP_TAGGED the operator belongs to the ENTRY: its top three bits are a tag (EQ, NE,
// EXISTS, ABSENT, GT, LT), the low 29 its id, and one call answers a whole conjunctive matchExpressions term per pod.  The node's id is
// compared WHOLE, as an unsigned 32-bit number: a snapshot may hold ids at or above 2^29, an entry cannot name them.
//
// Host-only on purpose, like sel_ops.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and tests/cpp/seltag_plan_tests.cpp
// pins every rule at its boundary without a GPU.  check_eval_args (ksched_api.hip) asks check_seltag_args for every evaluation entry point;
// plan_eval (eval_plan.hpp) carries `seltag` from EvalFacts to EvalPlan; launch_mask launches k_eval_seltag (kernels_seltag.hpp) through
// run_selector_mask (kernels_sel_walk.hpp) with what plan_seltag_launch says and takes no decision of its own.
#pragma once

#include <cstdint>

#include "../../include/ksched.h"
#include "sel_ops.hpp"

namespace ksched {

// does the flag word ask for the tagged reading of the selector entries?
constexpr bool sel_tagged(uint32_t flags) { return (flags & KSCHED_SELOP_TAGGED) != 0; }

// The argument rules of a flag word that may carry KSCHED_SELOP_TAGGED.  `accepted`: the entry point takes tagged calls (ksched_eval,
// ksched_eval_begin, ksched_eval_device, ksched_eval_device_pitched); ksched_pipe_submit passes false.  KSCHED_E_INVAL, with nothing
// enqueued:
//  * the flag where it is not accepted;
//  * an operator flag of E8 beside it: the operator is the entry's or the call's, not both;
//  * no KSCHED_SEL: the flag says how the selector entries are read;
//  * KSCHED_FIT, KSCHED_TAINT, KSCHED_WANT_FIT_MASK or out_fit: the call answers the selector term alone; fit and taints come from another
//    call and are combined in (KSCHED_COMBINE_*).
// A word without the flag is KSCHED_OK here whatever the rest says: the plain rules, the operators', the combine's and the picks' are
// check_eval_args' own, and hold for a tagged call unchanged.
constexpr int check_seltag_args(uint32_t flags, bool accepted, bool have_fit) {
    if (!sel_tagged(flags)) return KSCHED_OK;
    if (!accepted || (flags & KSCHED_SELOP_ANY)) return KSCHED_E_INVAL;
    if (!(flags & KSCHED_SEL)) return KSCHED_E_INVAL;
    if ((flags & (KSCHED_FIT | KSCHED_TAINT | KSCHED_WANT_FIT_MASK)) || have_fit) return KSCHED_E_INVAL;
    return KSCHED_OK;
}

// ---- the entry ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t seltag_tag(uint32_t e) { return e >> KSCHED_SELTAG_SHIFT; }
constexpr uint32_t seltag_id(uint32_t e) { return e & KSCHED_SELTAG_ID_MASK; }
constexpr uint32_t seltag_entry(uint32_t tag, uint32_t id) { return (tag << KSCHED_SELTAG_SHIFT) | (id & KSCHED_SELTAG_ID_MASK); }

// One (selector entry, node id) pair: e = sel_val_ids[k * p + pod], v = label_val_ids[k][node], the node's WHOLE id (0: the node does not
// carry the key).  e == 0: the pod does not constrain the key.  Tags 6 and 7 pass nowhere whatever the id field holds -- KSCHED_SEL_NEVER is
// tag 7 and keeps its meaning without a case of its own.  An absent node PASSES NE (Kubernetes' NotIn) and ABSENT, and fails the rest.
constexpr bool seltag_pass(uint32_t e, uint32_t v) {
    if (e == 0u) return true;
    const uint32_t id = seltag_id(e);
    switch (seltag_tag(e)) {
        case KSCHED_SELTAG_EQ: return v == id;
        case KSCHED_SELTAG_NE: return v != id;
        case KSCHED_SELTAG_EXISTS: return v != 0u;
        case KSCHED_SELTAG_ABSENT: return v == 0u;
        case KSCHED_SELTAG_GT: return v != 0u && v > id;
        case KSCHED_SELTAG_LT: return v != 0u && v < id;
        default: return false;
    }
}

// The ONE form the kernel reduces every constrained entry to, decoded on the scalar side (the entry is wave-uniform):
//     pass(v) = (v - lo < len) != neg        -- v - lo in unsigned 32-bit arithmetic, wrapping: v lies in the range [lo, lo + len)
// so that a constrained (key, column) costs a subtraction and one compare on the vector side whatever its tag, and no branch on the tag:
//     EQ      [id, id + 1)        NE      not [id, id + 1)
//     EXISTS  [1, 2^32)           ABSENT  not [1, 2^32)
//     GT      [id + 1, 2^32)      LT      [1, id)       (id 0 and 1: the empty range)
//     tags 6 and 7: the empty range (len == 0 passes no v; neg is false for them).
// `neg` is applied before the valid-bits word: a padding lane holds id 0 and PASSES a negated range.  The kernel computes the same three
// numbers from the tag's three bits in integer arithmetic (kernels_sel_walk.hpp: sel_and_entry); tests/cpp/seltag_plan_tests.cpp pins both against
// seltag_pass.
struct SeltagForm {
    uint32_t lo = 0, len = 0;
    bool neg = false;
};
constexpr SeltagForm seltag_form(uint32_t e) {
    const uint32_t tag = seltag_tag(e), id = seltag_id(e);
    SeltagForm f;
    switch (tag) {
        case KSCHED_SELTAG_EQ:
        case KSCHED_SELTAG_NE: f.lo = id, f.len = 1u; break;
        case KSCHED_SELTAG_EXISTS:
        case KSCHED_SELTAG_ABSENT: f.lo = 1u, f.len = 0xFFFFFFFFu; break;
        case KSCHED_SELTAG_GT: f.lo = id + 1u, f.len = ~id; break;
        case KSCHED_SELTAG_LT: f.lo = 1u, f.len = id > 1u ? id - 1u : 0u; break;
        default: break;
    }
    f.neg = tag == KSCHED_SELTAG_NE || tag == KSCHED_SELTAG_ABSENT;
    return f;
}
// the same, from the tag's bits without a compare: the kernel's arithmetic, restated here so that the host test pins it
constexpr SeltagForm seltag_form_bits(uint32_t e) {
    const uint32_t tag = seltag_tag(e), id = seltag_id(e);
    const uint32_t t0 = tag & 1u, t1 = (tag >> 1) & 1u, t2 = tag >> 2;
    const uint32_t by_id = 0u - ((t1 ^ 1u) & ((t0 & t2) ^ 1u));
    const uint32_t len45 = (((id > 1u ? id : 1u) - 1u) & (0u - t0)) | (~id & (t0 - 1u));
    const uint32_t len03 = 1u | (0u - t1);
    SeltagForm f;
    f.lo = (id & by_id) + (t1 | t2);
    f.len = ((len45 & (0u - t2)) | (len03 & (t2 - 1u))) & (0u - ((t1 & t2) ^ 1u));
    f.neg = (t0 & (t2 ^ 1u)) != 0u;
    return f;
}
constexpr bool seltag_form_pass(const SeltagForm &f, uint32_t v) { return ((uint32_t)(v - f.lo) < f.len) != f.neg; }

// One pod's row: what the kernel computes, and what tests restate it against.  `lab` holds the label columns [nkeys][n], `sel` the selector
// entries [nkeys][p]; `row` gets W = ceil(n / 64) words: bit (node % 64) of word (node / 64) is the AND over all keys of seltag_pass, the
// bits at or beyond n are zero -- under NE and ABSENT too.  sel == nullptr or nkeys == 0: no pod constrains anything, every node passes.
inline void seltag_row(const uint32_t *lab, const uint32_t *sel, uint32_t nkeys, uint32_t n, uint32_t p, uint32_t pod, uint64_t *row) {
    const uint32_t W = (uint32_t)(((uint64_t)n + 63u) / 64u);
    for (uint32_t w = 0; w < W; ++w) row[w] = 0;
    for (uint32_t node = 0; node < n; ++node) {
        bool ok = true;
        if (sel)
            for (uint32_t k = 0; k < nkeys && ok; ++k) ok = seltag_pass(sel[(uint64_t)k * p + pod], lab[(uint64_t)k * n + node]);
        if (ok) row[node >> 6] |= 1ull << (node & 63u);
    }
}

// ---- the launch -----------------------------------------------------------------------------------------------------------------
// k_eval_selop's geometry, unchanged (sel_ops.hpp: a wave on kSelopCW word columns, kSelopWaves waves a block, kSelopKeys keys a pass, the
// pod tiles spread over about kSelopTargetBlocks blocks): the tagged kernel keeps that mapping, only what a constrained entry means differs.
using SeltagLaunch = SelopLaunch;
constexpr SeltagLaunch plan_seltag_launch(uint32_t p, uint32_t W, uint32_t nkeys) { return plan_selop_launch(p, W, nkeys); }

}  // namespace ksched
