// sel_ops.hpp -- the rules of an OPERATOR call (extension E8, include/ksched.h: KSCHED_SELOP_EXISTS / _GT / _LT), said once: which operator a
// flag word names, which calls may carry one and with which other flags, the rule for one (selector entry, node id) pair, one pod's row
// restated on the CPU, and the geometry of the operator kernel's launches.
//
// An operator call answers ONE selector term per (pod, key) where a plain KSCHED_SEL call answers "the node's id equals this id": the node
// carries the key at all (EXISTS), carries it with an id above the pod's entry (GT), or below it (LT).  The ids are compared as unsigned
// 32-bit numbers, exactly; which id a value of a numeric label gets (say id = value + 1) is the caller's interning.  A node WITHOUT the key
// (id 0) fails every constrained key under every operator -- Kubernetes' rule for Gt / Lt on a missing label; it is what keeps LT from
// letting absent nodes through.
//
// Host-only on purpose, like mask_combine.hpp and mask_combine_soft.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/selop_plan_tests.cpp pins every rule at its boundary without a GPU.  check_eval_args (ksched_api.hip) asks check_selop_args for
// every evaluation entry point; plan_eval (eval_plan.hpp) carries the operator from EvalFacts to EvalPlan; launch_mask launches k_eval_selop
// (kernels_selop.hpp) through run_selector_mask (kernels_sel_walk.hpp) with what plan_selop_launch says and takes no decision of its own.
#pragma once

#include <cstdint>

#include "../../include/ksched.h"

namespace ksched {

enum class SelOp : uint8_t { kNone, kExists, kGt, kLt };

// at most one operator flag per call (two at once are the caller's KSCHED_E_INVAL: check_selop_args)
constexpr bool at_most_one_selop(uint32_t flags) {
    const uint32_t o = flags & KSCHED_SELOP_ANY;
    return (o & (o - 1u)) == 0;
}

// the operator of a flag word that carries at most one operator flag; kNone for none (and for more than one: such a word names no operator)
constexpr SelOp sel_op(uint32_t flags) {
    switch (flags & KSCHED_SELOP_ANY) {
        case KSCHED_SELOP_EXISTS: return SelOp::kExists;
        case KSCHED_SELOP_GT: return SelOp::kGt;
        case KSCHED_SELOP_LT: return SelOp::kLt;
        default: return SelOp::kNone;
    }
}

// The argument rules of a flag word that may carry an operator flag.  `accepted`: the entry point takes operator calls (ksched_eval,
// ksched_eval_begin, ksched_eval_device, ksched_eval_device_pitched); ksched_pipe_submit passes false.  KSCHED_E_INVAL, with nothing
// enqueued:
//  * an operator flag where none is accepted;
//  * two operator flags at once;
//  * no KSCHED_SEL: the operator is a reading of the selector entries;
//  * KSCHED_FIT, KSCHED_TAINT, KSCHED_WANT_FIT_MASK or out_fit: the call answers the selector term alone; fit and taints come from another
//    call and are combined in (KSCHED_COMBINE_*).
// A word without an operator flag is KSCHED_OK here whatever the rest says: the plain rules, the combine's and the picks' are
// check_eval_args' own, and hold for an operator call unchanged.
constexpr int check_selop_args(uint32_t flags, bool accepted, bool have_fit) {
    if (!(flags & KSCHED_SELOP_ANY)) return KSCHED_OK;
    if (!accepted || !at_most_one_selop(flags)) return KSCHED_E_INVAL;
    if (!(flags & KSCHED_SEL)) return KSCHED_E_INVAL;
    if ((flags & (KSCHED_FIT | KSCHED_TAINT | KSCHED_WANT_FIT_MASK)) || have_fit) return KSCHED_E_INVAL;
    return KSCHED_OK;
}

// One (selector entry, node id) pair: e = sel_val_ids[k * p + pod], v = label_val_ids[k][node].  e == 0: the pod does not constrain the
// key.  e == KSCHED_SEL_NEVER: "this expression can match nothing", under every operator.  Otherwise the node must carry the key (v != 0)
// and, for GT / LT, its id must lie above / below the entry as an unsigned 32-bit number.  (kNone: the plain call's equality.)
constexpr bool selop_pass(SelOp op, uint32_t e, uint32_t v) {
    if (e == 0u) return true;
    if (e == KSCHED_SEL_NEVER) return false;
    switch (op) {
        case SelOp::kExists: return v != 0u;
        case SelOp::kGt: return v != 0u && v > e;
        case SelOp::kLt: return v != 0u && v < e;
        default: return v == e;
    }
}

// One pod's row: what the kernel computes, and what tests restate it against.  `lab` holds the label columns [nkeys][n], `sel` the selector
// entries [nkeys][p]; `row` gets W = ceil(n / 64) words: bit (node % 64) of word (node / 64) is the AND over all keys of selop_pass, the
// bits at or beyond n are zero.  sel == nullptr or nkeys == 0: no pod constrains anything, every node passes.
inline void selop_row(SelOp op, const uint32_t *lab, const uint32_t *sel, uint32_t nkeys, uint32_t n, uint32_t p, uint32_t pod, uint64_t *row) {
    const uint32_t W = (uint32_t)(((uint64_t)n + 63u) / 64u);
    for (uint32_t w = 0; w < W; ++w) row[w] = 0;
    for (uint32_t node = 0; node < n; ++node) {
        bool ok = true;
        if (sel)
            for (uint32_t k = 0; k < nkeys && ok; ++k) ok = selop_pass(op, sel[(uint64_t)k * p + pod], lab[(uint64_t)k * n + node]);
        if (ok) row[node >> 6] |= 1ull << (node & 63u);
    }
}

// ---- the launch ---------------------------------------------------------------------------------------------------------------
// k_eval_direct's mapping (kernels_direct.hpp): a wave owns kSelopCW consecutive 64-node word columns, whose label ids of up to kSelopKeys
// keys stay in registers; a block is kSelopWaves waves on adjacent columns and walks `pod_tiles_per_block` tiles of 64 pods.  grid.x covers
// the word columns, grid.y the pod tiles: as many as bring the grid to about kSelopTargetBlocks blocks (all 256 compute units busy), but no
// more, so that a block stays on its node columns for as many pods as possible.  A snapshot with more than kSelopKeys keys takes one PASS
// per kSelopKeys keys; the passes after the first AND their words into the mask.  No keys (or no selectors): one pass without keys, which
// writes the all-valid rows.
constexpr uint32_t kSelopCW = 4;       // word columns per wave
constexpr uint32_t kSelopWaves = 4;    // waves per block: 16 words = 1024 nodes per block
constexpr uint32_t kSelopKeys = 8;     // label keys per pass
constexpr uint32_t kSelopTargetBlocks = 2048;

struct SelopLaunch {
    uint32_t block = 64u * kSelopWaves;
    uint32_t gx = 0, gy = 0;  // gx == 0: nothing to launch
    uint32_t pod_tiles = 0;            // ceil(p / 64)
    uint32_t pod_tiles_per_block = 0;  // ceil(pod_tiles / gy): the tiles [y * pod_tiles_per_block, ...) are block row y's
    uint32_t passes = 0;               // max(1, ceil(nkeys / kSelopKeys)); pass i handles the keys [i * kSelopKeys, ...)
};

// p rows of W words over `nkeys` keys that selectors constrain (0: none given, or a snapshot without keys)
constexpr SelopLaunch plan_selop_launch(uint32_t p, uint32_t W, uint32_t nkeys) {
    SelopLaunch l;
    if (p == 0 || W == 0) return l;
    const uint32_t words_per_block = kSelopCW * kSelopWaves;
    l.gx = (uint32_t)(((uint64_t)W + words_per_block - 1u) / words_per_block);
    l.pod_tiles = (uint32_t)(((uint64_t)p + 63u) / 64u);
    const uint32_t want = (kSelopTargetBlocks + l.gx - 1u) / l.gx;  // >= 1
    l.gy = l.pod_tiles < want ? l.pod_tiles : want;
    l.pod_tiles_per_block = (l.pod_tiles + l.gy - 1u) / l.gy;
    l.gy = (l.pod_tiles + l.pod_tiles_per_block - 1u) / l.pod_tiles_per_block;
    l.passes = nkeys == 0 ? 1u : (nkeys + kSelopKeys - 1u) / kSelopKeys;
    return l;
}

// the keys of pass i
constexpr uint32_t selop_pass_key0(uint32_t pass) { return pass * kSelopKeys; }
constexpr uint32_t selop_pass_keys(uint32_t nkeys, uint32_t pass) {
    return nkeys <= pass * kSelopKeys ? 0u : (nkeys - pass * kSelopKeys < kSelopKeys ? nkeys - pass * kSelopKeys : kSelopKeys);
}

}  // namespace ksched
