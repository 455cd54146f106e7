// mask_combine.hpp -- the rules of a combining evaluation (extension E6, include/ksched.h: KSCHED_COMBINE_AND / _OR / _ANDNOT), said once:
// which op a flag word names, which calls may carry one and with which outputs, the valid-bits word of a row's last word, how wide the
// combine kernel's accesses may be for a given pair of buffers, and the geometry of its launch.
//
// Host-only on purpose, like eval_plan.hpp, apply_plan.hpp and merge_sort_plan.hpp: no HIP include, no ksched_ctx, so that plain g++
// compiles it and tests/cpp/combine_plan_tests.cpp pins every rule at its boundary without a GPU.  check_eval_args (ksched_api.hip) asks
// check_combine_args (through mask_combine_soft.hpp's check_soft_args) for every evaluation entry point, the accepting and the refusing ones alike; plan_eval (eval_plan.hpp) carries the op
// from EvalFacts to EvalPlan; launch_mask launches k_mask_combine (kernels_combine.hpp) with what plan_combine_launch says and takes no
// decision of its own.
#pragma once

#include <cstdint>

#include "../../include/ksched.h"

namespace ksched {

// out_feasible = out_feasible OP feasible(this call)
enum class CombineOp : uint8_t { kNone, kAnd, kOr, kAndNot };

// at most one combine flag per call (two at once are the caller's KSCHED_E_INVAL: check_combine_args)
constexpr bool at_most_one_combine(uint32_t flags) {
    const uint32_t c = flags & KSCHED_COMBINE_ANY;
    return (c & (c - 1u)) == 0;
}

// the op of a flag word that carries at most one combine flag; kNone for none (and for more than one: such a word names no op)
constexpr CombineOp combine_op(uint32_t flags) {
    switch (flags & KSCHED_COMBINE_ANY) {
        case KSCHED_COMBINE_AND: return CombineOp::kAnd;
        case KSCHED_COMBINE_OR: return CombineOp::kOr;
        case KSCHED_COMBINE_ANDNOT: return CombineOp::kAndNot;
        default: return CombineOp::kNone;
    }
}

// one word of the combine: what the kernel computes, and what tests restate it against
constexpr uint64_t combine_word(CombineOp op, uint64_t old_word, uint64_t new_word) {
    return op == CombineOp::kAnd ? (old_word & new_word) : op == CombineOp::kOr ? (old_word | new_word) : op == CombineOp::kAndNot ? (old_word & ~new_word) : old_word;
}

// The argument rules of a flag word that may carry a combine flag.  `accepted`: the entry point takes combining calls
// (ksched_eval_device, ksched_eval_device_pitched); every other evaluation entry point passes false and refuses the flags -- a host
// mask would first have to travel to the device, a pipe slot's mask belongs to the slot.  KSCHED_E_INVAL, with nothing enqueued:
//  * a combine flag where none is accepted;
//  * two combine flags at once;
//  * no out_feasible: the mask is the call's left operand;
//  * KSCHED_WANT_FIT_MASK or out_fit: a combining call writes one mask.
// A word without a combine flag is KSCHED_OK here whatever the rest says: the plain rules are check_eval_args' own.
constexpr int check_combine_args(uint32_t flags, bool accepted, bool have_feas, bool have_fit) {
    if (!(flags & KSCHED_COMBINE_ANY)) return KSCHED_OK;
    if (!accepted || !at_most_one_combine(flags)) return KSCHED_E_INVAL;
    if (!have_feas) return KSCHED_E_INVAL;
    if ((flags & KSCHED_WANT_FIT_MASK) || have_fit) return KSCHED_E_INVAL;
    return KSCHED_OK;
}

// the bits of a row's last word that stand for nodes below n (n >= 1): the combine ANDs the last word with it, so that bits at or
// beyond n come out zero whatever the old mask held there
constexpr uint64_t valid_bits_word(uint32_t n) { return (n & 63u) ? ((1ull << (n & 63u)) - 1ull) : ~0ull; }

// ---- the launch ---------------------------------------------------------------------------------------------------------------
// A UNIT is two neighbouring words (16 bytes) of one row where both buffers allow it, else one word.  Units never straddle rows and never
// reach into the padding words [W, pitch): a row of odd W ends in a one-word unit.  A lane takes TWO units per iteration, one grid
// stride apart, and has the loads of both in flight before it stores either (kernels_combine.hpp; what it buys: DESIGN.md section 4).
constexpr uint32_t kCombineBlock = 256;     // threads per block: four waves
constexpr uint32_t kCombineMaxGrid = 2048;  // blocks: 256 compute units x 4 SIMDs x 8 waves, the chip's resident waves at the kernel's register count

// Words per unit for a pair of buffers with one row pitch: 2 when every row of both starts on a 16-byte boundary -- both bases 16-byte
// aligned and the pitch even --, else 1.  (A packed mask with odd W has rows that are only 8-byte aligned; so has a view that starts
// one word into a buffer.)
constexpr uint32_t combine_vec_words(uint64_t dst_addr, uint64_t src_addr, uint32_t pitch) {
    return (((dst_addr | src_addr) & 15u) == 0 && (pitch & 1u) == 0) ? 2u : 1u;
}

struct CombineLaunch {
    uint32_t vec = 1;            // words per unit: 1 or 2
    uint32_t units_per_row = 0;  // ceil(W / vec)
    uint64_t units = 0;          // p * units_per_row
    uint32_t block = kCombineBlock, grid = 0;  // grid == 0: nothing to launch
    // Grid stride: thread t starts at unit t = (row t / units_per_row, column t % units_per_row) and advances by grid * block units per
    // pass, i.e. by (drow, dcol) with a carry; it stops at the first row >= p.  Rows are counted in 64 bits: p * pitch words is a
    // supported size beyond 2^32.
    uint32_t drow = 0, dcol = 0;
    uint32_t drow2 = 0, dcol2 = 0;  // two strides as rows and columns: a lane's step from one iteration to the next
    uint64_t passes = 0;  // ceil(units / (grid * block)): the most units any thread takes; it runs ceil(passes / 2) iterations
};

// p >= 1 rows of W >= 1 words
constexpr CombineLaunch plan_combine_launch(uint32_t p, uint32_t W, uint32_t vec) {
    CombineLaunch l;
    l.vec = vec;
    l.units_per_row = (W + vec - 1u) / vec;
    l.units = (uint64_t)p * l.units_per_row;
    if (l.units == 0) return l;
    const uint64_t blocks = (l.units + kCombineBlock - 1u) / kCombineBlock;
    l.grid = blocks < kCombineMaxGrid ? (uint32_t)blocks : kCombineMaxGrid;
    const uint32_t stride = l.grid * kCombineBlock;
    l.drow = stride / l.units_per_row;
    l.dcol = stride % l.units_per_row;
    l.drow2 = 2u * l.drow + (2u * l.dcol) / l.units_per_row;
    l.dcol2 = (2u * l.dcol) % l.units_per_row;
    l.passes = (l.units + stride - 1u) / stride;
    return l;
}

}  // namespace ksched
