// mask_combine_soft.hpp -- the rules of a SOFT combining evaluation (extension E7, include/ksched.h: KSCHED_COMBINE_SOFT), said once: which
// flag words carry the modifier and which calls may, the row rule restated on the CPU, and the geometry of the soft combine's launch.
//
// The modifier turns "narrow the pod's row by this evaluation" into "... unless that would leave the row empty": per pod row
// r = old' OP new (OP one of AND, AND-NOT; old' = the caller's row with the bits at or beyond n cleared), and the row becomes r when r has a
// set bit, else old'.  The decision needs the whole row, so the kernel (kernels_combine_soft.hpp) gives every row to one GROUP of lanes of
// one wave, where k_mask_combine hands out units with no regard to rows.
//
// Host-only on purpose, like mask_combine.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/soft_plan_tests.cpp pins every rule at its boundary without a GPU.  check_eval_args (ksched_api.hip) asks check_soft_args for
// every evaluation entry point; plan_eval carries the bit from EvalFacts to EvalPlan; launch_mask launches k_mask_combine_soft with what
// plan_soft_launch says and takes no decision of its own.
#pragma once

#include <cstdint>

#include "mask_combine.hpp"

namespace ksched {

// does the flag word carry the modifier?
constexpr bool combine_soft(uint32_t flags) { return (flags & KSCHED_COMBINE_SOFT) != 0; }

// The argument rules of a flag word that may carry a combine flag, the modifier, or both: check_combine_args' rules (mask_combine.hpp) and,
// for a word with KSCHED_COMBINE_SOFT, KSCHED_E_INVAL with nothing enqueued for
//  * an entry point that takes no combining call (`accepted` false), whatever else the word says;
//  * no combine op: the modifier modifies one;
//  * KSCHED_COMBINE_OR: OR cannot empty a row, so the modifier would mean nothing;
//  * two ops at once, no out_feasible, KSCHED_WANT_FIT_MASK or out_fit: every refusal of a plain combining call.
// A word with neither is KSCHED_OK here whatever the rest says: the plain rules are check_eval_args' own.
constexpr int check_soft_args(uint32_t flags, bool accepted, bool have_feas, bool have_fit) {
    if (combine_soft(flags)) {
        if (!accepted || !at_most_one_combine(flags)) return KSCHED_E_INVAL;
        const CombineOp op = combine_op(flags);
        if (op != CombineOp::kAnd && op != CombineOp::kAndNot) return KSCHED_E_INVAL;
    }
    return check_combine_args(flags, accepted, have_feas, have_fit);
}

// One row of the soft combine, in place: what the kernel computes, and what tests restate it against.  old_row and new_row hold W =
// ceil(n / 64) words (n >= 1), op is kAnd or kAndNot.  Returns whether the row NARROWED (r had a set bit and was stored); a row that did not
// comes out as old': the caller's row with the bits at or beyond n cleared -- all zero if it held nothing below n.
inline bool soft_row(CombineOp op, uint64_t *old_row, const uint64_t *new_row, uint32_t W, uint32_t n) {
    old_row[W - 1u] &= valid_bits_word(n);
    uint64_t any = 0;
    for (uint32_t w = 0; w < W; ++w) any |= combine_word(op, old_row[w], new_row[w]);
    if (!any) return false;
    for (uint32_t w = 0; w < W; ++w) old_row[w] = combine_word(op, old_row[w], new_row[w]);
    return true;
}

// ---- the launch ---------------------------------------------------------------------------------------------------------------
// A UNIT is mask_combine.hpp's: two neighbouring words (16 bytes) of one row where both buffers allow it (combine_vec_words), else one word;
// a row of odd W ends in a one-word unit, so no unit reaches into the padding words [W, pitch).
// A row belongs to one GROUP of lanes: a power of two from 1 to 64 neighbouring lanes of one wave, 64 / group rows per wave.  Lane j of the
// group takes the units j, j + group, j + 2 * group, ... of its row -- neighbouring lanes, neighbouring units -- which are `units_per_lane`
// at most.  The group is the smallest that leaves a lane at most kSoftLaneUnits units, so that short rows fill the wave with several
// rows instead of idling most of its lanes, and a lane has several loads in flight; rows too long for that take a whole wave.
// Up to kSoftKeepUnits units per lane the group KEEPS the row in registers between the decision and the stores (one read of each buffer, at
// most one write: what k_mask_combine moves); a longer row (more than 64 * kSoftKeepUnits units: 65 536 nodes in 16-byte units) is
// read TWICE, once to decide and once to store.
// The grid is bounded and strides over the rows by `rows_per_pass`.  Rows are counted in 64 bits by the kernel: row + rows_per_pass may
// pass 2^32, and p * pitch words is a supported size beyond 2^32.
constexpr uint32_t kSoftBlock = 256;     // threads per block: four waves
constexpr uint32_t kSoftMaxGrid = 2048;  // blocks (as kCombineMaxGrid)
constexpr uint32_t kSoftWave = 64;       // lanes per wave: the largest group
constexpr uint32_t kSoftLaneUnits = 4;   // the group doubles until a lane has at most this many units, or the group is the wave
constexpr uint32_t kSoftKeepUnits = 8;   // the most units a lane keeps in registers (16 bytes each and twice: the row's words and the evaluation's)

struct SoftLaunch {
    uint32_t vec = 1;             // words per unit: 1 or 2
    uint32_t units_per_row = 0;   // ceil(W / vec)
    uint32_t group = 1, group_shift = 0;  // lanes per row, and its log2
    uint32_t units_per_lane = 0;  // ceil(units_per_row / group)
    bool keep = true;             // units_per_lane <= kSoftKeepUnits: the row stays in registers; else it is read twice
    uint32_t rows_per_block = 0;  // kSoftBlock / group
    uint32_t block = kSoftBlock, grid = 0;  // grid == 0: nothing to launch
    uint32_t rows_per_pass = 0;   // grid * rows_per_block (<= 2^19): the grid stride, in rows
    uint64_t passes = 0;          // ceil(p / rows_per_pass): the most rows any group takes
};

// p rows of W >= 1 words
constexpr SoftLaunch plan_soft_launch(uint32_t p, uint32_t W, uint32_t vec) {
    SoftLaunch l;
    l.vec = vec;
    l.units_per_row = (W + vec - 1u) / vec;
    while (l.group < kSoftWave && (l.units_per_row + l.group - 1u) / l.group > kSoftLaneUnits) l.group *= 2u, ++l.group_shift;
    l.units_per_lane = (l.units_per_row + l.group - 1u) / l.group;
    l.keep = l.units_per_lane <= kSoftKeepUnits;
    l.rows_per_block = kSoftBlock / l.group;
    if (p == 0) return l;
    const uint64_t blocks = ((uint64_t)p + l.rows_per_block - 1u) / l.rows_per_block;
    l.grid = blocks < kSoftMaxGrid ? (uint32_t)blocks : kSoftMaxGrid;
    l.rows_per_pass = l.grid * l.rows_per_block;
    l.passes = ((uint64_t)p + l.rows_per_pass - 1u) / l.rows_per_pass;
    return l;
}

}  // namespace ksched
