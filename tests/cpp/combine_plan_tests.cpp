// combine_plan_tests.cpp -- host-side check of the rules of a combining evaluation (extension E6: csrc/mask_combine.hpp, csrc/eval_plan.hpp),
// no GPU and no HIP: the op of a flag word, the argument rules for accepting and refusing entry points, the valid-bits word, the access
// width for aligned and unaligned buffers, the launch geometry at one word, one wave, one grid pass and one unit more, executed on the CPU
// (every unit visited exactly once, padding never); the plan of a combining request under every option; and, over a sweep of today's
// requests, that a plan without an op is the plan as it was computed before the field existed (plan_eval_as_it_was below).
// The expectations are written out here, not computed by the header.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/eval_plan.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/mask_combine.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static bool is(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

static const uint32_t kAnd = 0x200u, kOr = 0x400u, kAndNot = 0x800u;

// ---- the constants and the op of a flag word ---------------------------------------------------------------------------------------
static void the_flags_and_their_ops() {
    CHECK(KSCHED_COMBINE_AND == kAnd && KSCHED_COMBINE_OR == kOr && KSCHED_COMBINE_ANDNOT == kAndNot && KSCHED_COMBINE_ANY == 0xE00u);
    const uint32_t others = KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_ANY | KSCHED_WANT_FIT_MASK;
    CHECK(others == 0x1FFu && !(others & KSCHED_COMBINE_ANY) && !(0x1000u & KSCHED_COMBINE_ANY));
    CHECK(combine_op(0) == CombineOp::kNone && combine_op(others) == CombineOp::kNone && combine_op(0x1000u) == CombineOp::kNone);
    for (uint32_t rest : {0u, others, (uint32_t)KSCHED_FIT, (uint32_t)(KSCHED_SEL | KSCHED_PICK_SPREAD)}) {
        CHECK(combine_op(rest | kAnd) == CombineOp::kAnd);
        CHECK(combine_op(rest | kOr) == CombineOp::kOr);
        CHECK(combine_op(rest | kAndNot) == CombineOp::kAndNot);
        // two or three at once name no op, and are not "at most one"
        CHECK(combine_op(rest | kAnd | kOr) == CombineOp::kNone && combine_op(rest | kOr | kAndNot) == CombineOp::kNone &&
              combine_op(rest | kAnd | kAndNot) == CombineOp::kNone && combine_op(rest | 0xE00u) == CombineOp::kNone);
        CHECK(at_most_one_combine(rest) && at_most_one_combine(rest | kAnd) && at_most_one_combine(rest | kOr) && at_most_one_combine(rest | kAndNot));
        CHECK(!at_most_one_combine(rest | kAnd | kOr) && !at_most_one_combine(rest | kOr | kAndNot) && !at_most_one_combine(rest | kAnd | kAndNot) &&
              !at_most_one_combine(rest | 0xE00u));
    }
    CHECK(combine_word(CombineOp::kAnd, 0xCull, 0xAull) == 0x8ull && combine_word(CombineOp::kOr, 0xCull, 0xAull) == 0xEull &&
          combine_word(CombineOp::kAndNot, 0xCull, 0xAull) == 0x4ull && combine_word(CombineOp::kNone, 0xCull, 0xAull) == 0xCull);
    CHECK(combine_word(CombineOp::kAndNot, ~0ull, 0ull) == ~0ull && combine_word(CombineOp::kAndNot, ~0ull, ~0ull) == 0ull);
}

// ---- the argument rules ---------------------------------------------------------------------------------------------------------------
static void the_argument_rules() {
    for (uint32_t op : {kAnd, kOr, kAndNot})
        for (uint32_t rest : {0u, (uint32_t)KSCHED_FIT, (uint32_t)(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT), (uint32_t)(KSCHED_FIT | KSCHED_PICK_BESTFIT),
                              (uint32_t)(KSCHED_SEL | KSCHED_PICK_SPREAD)}) {
            const uint32_t f = rest | op;
            CHECK(check_combine_args(f, true, true, false) == KSCHED_OK);           // accepted, the mask given, no fit mask
            CHECK(check_combine_args(f, false, true, false) == KSCHED_E_INVAL);     // an entry point that refuses the flags, whatever it was given
            CHECK(check_combine_args(f, false, false, false) == KSCHED_E_INVAL);
            CHECK(check_combine_args(f, true, false, false) == KSCHED_E_INVAL);     // out_feasible == NULL
            CHECK(check_combine_args(f, true, true, true) == KSCHED_E_INVAL);       // out_fit
            CHECK(check_combine_args(f | KSCHED_WANT_FIT_MASK, true, true, false) == KSCHED_E_INVAL);  // the flag without the pointer
            CHECK(check_combine_args(f | KSCHED_WANT_FIT_MASK, true, true, true) == KSCHED_E_INVAL);   // both
            for (uint32_t second : {kAnd, kOr, kAndNot})
                if (second != op) CHECK(check_combine_args(f | second, true, true, false) == KSCHED_E_INVAL);  // two at once
            CHECK(check_combine_args(rest | 0xE00u, true, true, false) == KSCHED_E_INVAL);
            // a word without a combine flag: the rule says nothing (the plain rules are check_eval_args' own), accepted or not
            for (int accepted = 0; accepted < 2; ++accepted)
                for (int feas = 0; feas < 2; ++feas)
                    for (int fit = 0; fit < 2; ++fit) {
                        CHECK(check_combine_args(rest, accepted, feas, fit) == KSCHED_OK);
                        CHECK(check_combine_args(rest | KSCHED_WANT_FIT_MASK, accepted, feas, fit) == KSCHED_OK);
                        CHECK(check_combine_args(rest | 0x1000u, accepted, feas, fit) == KSCHED_OK);  // (unknown, not a combine flag: refused by the caller's `known` set)
                    }
        }
}

// ---- the valid-bits word ----------------------------------------------------------------------------------------------------------------
static void the_valid_bits_word() {
    CHECK(valid_bits_word(1) == 0x1ull && valid_bits_word(2) == 0x3ull);
    CHECK(valid_bits_word(63) == 0x7FFFFFFFFFFFFFFFull && valid_bits_word(64) == ~0ull && valid_bits_word(65) == 0x1ull);
    CHECK(valid_bits_word(127) == 0x7FFFFFFFFFFFFFFFull && valid_bits_word(128) == ~0ull && valid_bits_word(129) == 0x1ull);
    CHECK(valid_bits_word(5000) == 0xFFull);  // 5000 = 78 * 64 + 8
    CHECK(valid_bits_word(0xFFFFFFFFu) == 0x7FFFFFFFFFFFFFFFull && valid_bits_word(0xFFFFFFC0u) == ~0ull && valid_bits_word(0xFFFFFFC1u) == 0x1ull);
}

// ---- the access width -----------------------------------------------------------------------------------------------------------------
static void the_width_rule() {
    const uint64_t base = 0x7f0000001000ull;  // 4 KiB aligned
    CHECK(combine_vec_words(base, base + 0x100000, 2) == 2u && combine_vec_words(base, base + 0x100000, 16) == 2u && combine_vec_words(base, base + 0x100000, 80) == 2u);
    CHECK(combine_vec_words(base + 16, base + 32, 2) == 2u);  // 16-byte aligned is enough
    // an odd pitch: every other row is only 8-byte aligned (a packed mask with odd W: 79 words at 5 000 nodes)
    CHECK(combine_vec_words(base, base + 0x100000, 1) == 1u && combine_vec_words(base, base + 0x100000, 3) == 1u && combine_vec_words(base, base + 0x100000, 79) == 1u);
    // a base one word into a buffer, either buffer
    CHECK(combine_vec_words(base + 8, base + 0x100000, 2) == 1u && combine_vec_words(base, base + 0x100000 + 8, 2) == 1u && combine_vec_words(base + 8, base + 8, 16) == 1u);
    CHECK(combine_vec_words(base + 24, base, 16) == 1u);
    CHECK(combine_vec_words(base + 8, base, 3) == 1u);
}

// ---- the geometry, executed --------------------------------------------------------------------------------------------------------------
// Every thread of the launch walks as k_mask_combine does (two units per iteration, one stride apart; the same start, steps and carries);
// `seen` counts the visits of every word of a [p][pitch] buffer.  Every word below W is visited exactly once, no padding word ever, nobody
// takes more than `passes` units or runs more than ceil(passes / 2) iterations.
static void advance(uint64_t &row, uint32_t &col, uint32_t drow, uint32_t dcol, uint32_t upr) {
    row += drow;
    col += dcol;
    if (col >= upr) col -= upr, ++row;
}
static void walk(uint32_t p, uint32_t W, uint32_t pitch, uint32_t vec) {
    const CombineLaunch l = plan_combine_launch(p, W, vec);
    CHECK(l.vec == vec && l.block == 256u && l.units_per_row == (W + vec - 1) / vec && l.units == (uint64_t)p * l.units_per_row);
    CHECK(l.grid >= 1u && l.grid <= 2048u && (uint64_t)l.grid * l.block >= (l.units < 2048u * 256u ? l.units : 2048u * 256u));
    const uint32_t stride = l.grid * l.block;
    CHECK(l.drow == stride / l.units_per_row && l.dcol == stride % l.units_per_row && l.passes == (l.units + stride - 1) / stride);
    CHECK((uint64_t)l.drow2 * l.units_per_row + l.dcol2 == 2ull * stride && l.dcol2 < l.units_per_row);  // two strides, as rows and columns
    std::vector<uint8_t> seen((size_t)p * pitch, 0);
    uint64_t most = 0, most_iters = 0;
    auto visit = [&](uint64_t row, uint32_t col) {
        const uint32_t w0 = vec == 2 ? 2u * col : col;
        const bool both = vec == 2 && w0 + 1u < W;
        if (w0 >= W) { CHECK(!"a unit starts in the padding"); return; }
        ++seen[(size_t)row * pitch + w0];
        if (both) ++seen[(size_t)row * pitch + w0 + 1u];
    };
    for (uint32_t t = 0; t < stride; ++t) {
        uint64_t row0 = t / l.units_per_row, row1 = row0, units = 0, iters = 0;
        uint32_t col0 = t - (uint32_t)row0 * l.units_per_row, col1 = col0;
        advance(row1, col1, l.drow, l.dcol, l.units_per_row);
        while (row0 < p) {
            ++iters;
            visit(row0, col0), ++units;
            if (row1 < p) visit(row1, col1), ++units;
            advance(row0, col0, l.drow2, l.dcol2, l.units_per_row);
            advance(row1, col1, l.drow2, l.dcol2, l.units_per_row);
        }
        if (units > most) most = units;
        if (iters > most_iters) most_iters = iters;
    }
    CHECK(most == l.passes);
    CHECK(most_iters == (l.passes + 1) / 2);
    bool once = true, padding_alone = true;
    for (uint32_t r = 0; r < p; ++r)
        for (uint32_t w = 0; w < pitch; ++w) {
            const uint8_t s = seen[(size_t)r * pitch + w];
            if (w < W ? s != 1 : s != 0) (w < W ? once : padding_alone) = false;
        }
    CHECK(once);
    CHECK(padding_alone);
}

static void the_geometry() {
    // one word
    CombineLaunch l = plan_combine_launch(1, 1, 1);
    CHECK(l.units == 1 && l.grid == 1 && l.block == 256 && l.passes == 1 && l.units_per_row == 1 && l.drow == 256 && l.dcol == 0 && l.drow2 == 512 && l.dcol2 == 0);
    l = plan_combine_launch(1, 1, 2);  // the wide form of a one-word row: one one-word unit
    CHECK(l.units == 1 && l.grid == 1 && l.units_per_row == 1 && l.passes == 1);
    // one wave's worth, one block's worth and one unit more
    l = plan_combine_launch(64, 1, 1);
    CHECK(l.units == 64 && l.grid == 1 && l.passes == 1);
    l = plan_combine_launch(1, 128, 2);
    CHECK(l.units == 64 && l.units_per_row == 64 && l.grid == 1 && l.passes == 1 && l.drow == 4 && l.dcol == 0);
    l = plan_combine_launch(256, 1, 1);
    CHECK(l.units == 256 && l.grid == 1 && l.passes == 1);
    l = plan_combine_launch(257, 1, 1);
    CHECK(l.units == 257 && l.grid == 2 && l.passes == 1);
    // a full grid pass and one unit more: n = 65 (W = 2) packed and aligned -> one unit per row
    const uint32_t full = 2048u * 256u;
    CHECK(kCombineMaxGrid == 2048u && kCombineBlock == 256u && full == 524288u);
    l = plan_combine_launch(full, 2, 2);
    CHECK(l.units == full && l.grid == 2048 && l.passes == 1);
    l = plan_combine_launch(full + 1, 2, 2);
    CHECK(l.units == full + 1ull && l.grid == 2048 && l.passes == 2 && l.drow == full && l.dcol == 0);
    l = plan_combine_launch(full / 2 + 1, 2, 1);  // the same mask unaligned: two one-word units per row
    CHECK(l.units == full + 2ull && l.grid == 2048 && l.passes == 2 && l.units_per_row == 2 && l.drow == full / 2 && l.dcol == 0);
    // C3 packed (79 words: the one-word path) and pitched (80: wide), the C5 shard pitched, and the largest batch: 64-bit unit counts
    l = plan_combine_launch(100000, 79, 1);
    CHECK(l.units == 7900000ull && l.grid == 2048 && l.passes == 16 && l.drow == 6636 && l.dcol == 44 && l.drow2 == 13273 && l.dcol2 == 9);
    l = plan_combine_launch(100000, 79, 2);
    CHECK(l.units == 4000000ull && l.units_per_row == 40 && l.passes == 8 && l.drow == 13107 && l.dcol == 8 && l.drow2 == 26214 && l.dcol2 == 16);
    l = plan_combine_launch(125000, 782, 2);
    CHECK(l.units == 48875000ull && l.units_per_row == 391 && l.passes == 94);
    l = plan_combine_launch(0xFFFFFFFFu, 1u << 20, 2);
    CHECK(l.units == (uint64_t)0xFFFFFFFFu * (1u << 19) && l.grid == 2048 && l.drow == 1 && l.dcol == 0);
    l = plan_combine_launch(0, 5, 1);
    CHECK(l.units == 0 && l.grid == 0 && l.passes == 0);  // nothing to launch
    // executed: odd and even W, packed and pitched, both widths, fewer threads than units and more
    for (uint32_t W : {1u, 2u, 3u, 16u, 17u, 79u})
        for (uint32_t p : {1u, 2u, 37u, 257u})
            for (uint32_t extra : {0u, 1u, 15u})
                for (uint32_t vec : {1u, 2u})
                    if (vec == 1 || ((W + extra) & 1u) == 0) walk(p, W, W + extra, vec);
    walk(full / 2 + 1, 2, 2, 1);  // more than one pass, with and without a carry
    walk(7000, 79, 80, 2);
    walk(7000, 79, 79, 1);
    walk(full + 1, 2, 2, 2);
    walk(3 * full / 2 + 7, 2, 2, 2);   // three passes: an iteration with two units, then one with one
    walk(13000, 79, 80, 2);            // two full iterations at C3's row shape
}

// ---- the plan of a combining request ---------------------------------------------------------------------------------------------------
// a C3-like step (100 k pods x 5 k nodes, 5 tiles, every fused form applicable, default options) with `extra` flags and the mask given
static EvalFacts step(uint32_t extra, uint32_t attempts) {
    EvalFacts f;
    f.p = 100000;
    f.n = 5000;
    f.attempts = attempts;
    f.flags = KSCHED_FIT | KSCHED_SEL | extra;
    f.nkeys = 8;
    f.have_feas = true;
    f.have_psel = true;
    f.tiles = 5;
    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = true;
    f.bf_rows_built = true;
    f.fused_waves = 16;
    f.combine = combine_op(f.flags);
    return f;
}

struct Op {
    uint32_t flag;
    CombineOp op;
};
static const Op kOps[] = {{kAnd, CombineOp::kAnd}, {kOr, CombineOp::kOr}, {kAndNot, CombineOp::kAndNot}};

// the mask kernel into the scratch mask, the op, and exactly the named pick behind the combine; nothing rides, no pick ahead of the mask
static bool combining(const EvalPlan &pl, CombineOp op, MaskKernel mask, SampledPick s, BestfitPick b, RankedPick r, const char *last_pick) {
    return pl.error == KSCHED_OK && pl.why == PlanError::kNone && pl.combine == op && pl.mask == mask && pl.scratch_mask && pl.sampled == s &&
           pl.bestfit == b && pl.ranked == r && !pl.pick_rides() && !pl.bestfit_rows() &&
           pl.pick_from_mask() == (s != SampledPick::kNone || b != BestfitPick::kNone || r != RankedPick::kNone) && is(pl.last_pick, last_pick) &&
           is(pl.last_kernel, mask == MaskKernel::kFused ? "fused" : "direct");
}

static void the_plan_of_a_combining_request(const Op &o) {
    // under every option that steers a pick, with and without best-fit rows: the same plan
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
            for (int stages = 0; stages <= 2; ++stages)
                for (int bf = 0; bf < 2; ++bf)
                    for (uint32_t p : {1u, 100000u, 1u << 20})
                        for (uint32_t nlist : {0u, 2u}) {
                            auto with = [&](uint32_t pick, uint32_t attempts) {
                                EvalFacts f = step(o.flag | pick, attempts);
                                f.opt_pick_from_mask = from_mask;
                                f.opt_fused_pick = fused_pick;
                                f.opt_bestfit_stages = stages;
                                f.bf_rows_built = bf;
                                f.p = p;
                                f.nlist = nlist;
                                return plan_eval(f);
                            };
                            CHECK(combining(with(0, 0), o.op, MaskKernel::kFused, SampledPick::kNone, BestfitPick::kNone, RankedPick::kNone, "none"));
                            CHECK(combining(with(KSCHED_PICK_SAMPLED, 5), o.op, MaskKernel::kFused, SampledPick::kFromMask, BestfitPick::kNone, RankedPick::kNone, "from-mask"));
                            CHECK(combining(with(KSCHED_PICK_SAMPLED, 7), o.op, MaskKernel::kFused, SampledPick::kFromMask, BestfitPick::kNone, RankedPick::kNone, "from-mask"));
                            CHECK(combining(with(KSCHED_PICK_BESTFIT, 0), o.op, MaskKernel::kFused, SampledPick::kNone, BestfitPick::kFromMask, RankedPick::kNone, "from-mask"));
                            CHECK(combining(with(KSCHED_PICK_UNIFORM, 1), o.op, MaskKernel::kFused, SampledPick::kNone, BestfitPick::kNone, RankedPick::kUniform, "uniform"));
                            CHECK(combining(with(KSCHED_PICK_SPREAD, 3), o.op, MaskKernel::kFused, SampledPick::kNone, BestfitPick::kNone, RankedPick::kSpread, "spread"));
                            CHECK(combining(with(KSCHED_PICK_PACK, 3), o.op, MaskKernel::kFused, SampledPick::kNone, BestfitPick::kNone, RankedPick::kPack, "pack"));
                        }
    // best fit over list keys with more nodes than the two-stage pick takes is unsupported as a plain call; a combining call picks from the mask
    {
        EvalFacts f = step(o.flag | KSCHED_PICK_BESTFIT, 0);
        f.nlist = 2;
        f.n = kBfLanesMaxNodes + 1;
        CHECK(combining(plan_eval(f), o.op, MaskKernel::kFused, SampledPick::kNone, BestfitPick::kFromMask, RankedPick::kNone, "from-mask"));
        f.combine = CombineOp::kNone;
        f.flags &= ~KSCHED_COMBINE_ANY;
        CHECK(plan_eval(f).error == KSCHED_E_UNSUPPORTED);
    }
    // the mask kernel is the one a mask-only request of the same facts gets; a forced fused kernel that does not apply is unsupported
    for (uint32_t pick : {0u, (uint32_t)KSCHED_PICK_SAMPLED, (uint32_t)KSCHED_PICK_BESTFIT, (uint32_t)KSCHED_PICK_UNIFORM, (uint32_t)KSCHED_PICK_SPREAD, (uint32_t)KSCHED_PICK_PACK})
        for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
            for (int can = 0; can < 2; ++can) {
                EvalFacts a = step(o.flag | pick, 5), b = step(0, 0);
                a.opt_kernel = b.opt_kernel = opt;
                a.fused_applicable = b.fused_applicable = can;
                a.fused_pick_applicable = a.fused_tile_pick_applicable = can;
                const EvalPlan pa = plan_eval(a), pb = plan_eval(b);
                CHECK(pa.error == pb.error && pa.why == pb.why && pa.mask == pb.mask && is(pa.last_kernel, pb.last_kernel));
                if (opt == KSCHED_KERNEL_FUSED && !can) {
                    CHECK(pa.error == KSCHED_E_UNSUPPORTED && pa.why == PlanError::kFusedNotApplicable && pa.mask == MaskKernel::kNone && pa.combine == CombineOp::kNone &&
                          !pa.scratch_mask && pa.sampled == SampledPick::kNone && pa.bestfit == BestfitPick::kNone && pa.ranked == RankedPick::kNone && !pa.pick_from_mask());
                } else {
                    CHECK(pa.error == KSCHED_OK && pa.combine == o.op && pa.scratch_mask && !pb.scratch_mask);
                    CHECK(pa.mask == (opt == KSCHED_KERNEL_DIRECT || (opt == KSCHED_KERNEL_AUTO && !can) ? MaskKernel::kDirect : MaskKernel::kFused));
                }
            }
}

// ---- no op: today's plans -----------------------------------------------------------------------------------------------------------------
// plan_eval as it was before EvalFacts and EvalPlan had the combine field (the parent's function, word for word)
static EvalPlan plan_eval_as_it_was(const EvalFacts &f) {
    EvalPlan plan;
    const uint32_t p = f.p, flags = f.flags;
    const bool pick_s = flags & KSCHED_PICK_SAMPLED, pick_b = flags & KSCHED_PICK_BESTFIT;
    const bool want_mask = f.have_feas || f.have_fit;
    const bool can_fused = f.fused_applicable;
    const int kern = choose_kernel(f.opt_kernel, can_fused);
    if (const RankedMember *m = ranked_member(flags)) {
        if (kern == KSCHED_KERNEL_FUSED && !can_fused) return plan_unsupported(PlanError::kFusedNotApplicable);
        plan.scratch_mask = !f.have_feas;
        plan.mask = kern == KSCHED_KERNEL_FUSED ? MaskKernel::kFused : MaskKernel::kDirect;
        plan.last_kernel = kern == KSCHED_KERNEL_FUSED ? "fused" : "direct";
        plan.ranked = m->pick;
        plan.last_pick = m->name;
        return plan;
    }
    const bool select_direct = pick_s && !f.opt_pick_from_mask;
    const bool tile_pays = f.tiles >= 2u && f.tiles <= 12u;
    const bool tile_form = f.opt_fused_pick == 3 || (f.opt_fused_pick == 1 && can_fused && tile_pays && f.fused_tile_pick_applicable);
    bool ride_pays = true;
    if (f.opt_fused_pick == 1 && can_fused) {
        if (tile_form) {
            ride_pays = p <= (1u << 19);
        } else {
            const uint32_t tiles = std::max(1u, f.tiles), cus = f.opt_grid_cus ? f.opt_grid_cus : 256u;
            const uint32_t chunks = std::max(1u, std::min(cus / tiles, (p + 255u) / 256u));
            ride_pays = (uint64_t)p <= (uint64_t)chunks * 5u * 64u * f.fused_waves;
        }
    }
    const bool pick_rides = select_direct && want_mask && f.opt_fused_pick && kern == KSCHED_KERNEL_FUSED && can_fused && ride_pays &&
                            f.fused_pick_applicable;
    if (pick_rides) {
        if (tile_form && !f.fused_tile_pick_applicable) return plan_unsupported(PlanError::kTilePickNotApplicable);
        plan.sampled = tile_form ? SampledPick::kRidesTiles : SampledPick::kRidesFill;
        plan.last_pick = tile_form ? "fused-tile" : "fused";
    } else if (select_direct) {
        plan.sampled = SampledPick::kOwnLaunch;
        plan.last_pick = "select";
        if (!want_mask) return plan;
    }
    if (pick_b && !f.opt_pick_from_mask && f.bf_rows_built) {
        const bool sel = (flags & KSCHED_SEL) && f.have_psel && f.nkeys > 0;
        const bool lists = sel && f.nlist > 0;
        const bool two_stage = lists || f.opt_bestfit_stages == 2 || (f.opt_bestfit_stages == 0 && p >= 24576u);
        if (!lists && (!two_stage || (f.debug & 0x400u) || f.n > kBfLanesMaxNodes)) {
            plan.bestfit = BestfitPick::kRowsOneStage;
        } else {
            if (f.n > kBfLanesMaxNodes) return plan_unsupported(PlanError::kListKeysTooManyNodes);
            plan.bestfit = lists ? BestfitPick::kRowsTwoStagesListed : BestfitPick::kRowsTwoStages;
        }
        plan.last_pick = "bestfit-rows";
        if (!want_mask) return plan;
    }
    plan.scratch_mask = !f.have_feas;
    if (kern == KSCHED_KERNEL_FUSED && !can_fused) return plan_unsupported(PlanError::kFusedNotApplicable);
    plan.mask = kern == KSCHED_KERNEL_FUSED ? MaskKernel::kFused : MaskKernel::kDirect;
    plan.last_kernel = kern == KSCHED_KERNEL_FUSED ? "fused" : "direct";
    if (pick_reads_mask(flags, f.opt_pick_from_mask, f.bf_rows_built)) {
        if (pick_s) plan.sampled = SampledPick::kFromMask;
        else plan.bestfit = BestfitPick::kFromMask;
        plan.last_pick = "from-mask";
    }
    return plan;
}

static bool same_plan(const EvalPlan &a, const EvalPlan &b) {
    return a.error == b.error && a.why == b.why && a.mask == b.mask && a.scratch_mask == b.scratch_mask && a.sampled == b.sampled && a.bestfit == b.bestfit &&
           a.ranked == b.ranked && is(a.last_kernel, b.last_kernel) && is(a.last_pick, b.last_pick);
}

static void without_an_op_every_plan_is_what_it_was() {
    const uint32_t picks[] = {0u, KSCHED_PICK_SAMPLED, KSCHED_PICK_BESTFIT, KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD, KSCHED_PICK_PACK};
    const uint32_t preds[] = {KSCHED_FIT, KSCHED_FIT | KSCHED_SEL, KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT};
    unsigned plans = 0, errors = 0;
    for (uint32_t pick : picks)
        for (uint32_t pred : preds)
            for (uint32_t outs = 0; outs < 4; ++outs)  // bit 0: out_feasible, bit 1: out_fit (+ WANT_FIT_MASK)
                for (int opt_kernel : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
                    for (uint32_t applic = 0; applic < 4; ++applic)  // 0: nothing fused applies, 1: the mask kernel, 2: + riding pick, 3: + tile pick
                        for (int from_mask = 0; from_mask < 2; ++from_mask)
                            for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
                                for (int stages = 0; stages <= 2; ++stages)
                                    for (int bf = 0; bf < 2; ++bf)
                                        for (uint32_t p : {1u, 24575u, 24576u, 100000u, (1u << 19) + 1u})
                                            for (uint32_t shape = 0; shape < 4; ++shape) {  // (tiles, nlist, n)
                                                if (!pick && !outs) continue;  // (check_eval_args refuses a call with nothing to write)
                                                EvalFacts f;
                                                f.p = p;
                                                f.n = shape == 3 ? kBfLanesMaxNodes + 1 : 5000;
                                                f.attempts = pick & KSCHED_PICK_DRAWS ? 5 : 0;
                                                f.flags = pred | pick | ((outs & 2u) ? KSCHED_WANT_FIT_MASK : 0u);
                                                f.nkeys = 8;
                                                f.have_feas = outs & 1u;
                                                f.have_fit = outs & 2u;
                                                f.have_psel = pred & KSCHED_SEL;
                                                f.tiles = shape == 0 ? 1 : shape == 1 ? 5 : 13;
                                                f.nlist = shape >= 2 ? 2 : 0;
                                                f.fused_applicable = applic >= 1;
                                                f.fused_pick_applicable = applic >= 2;
                                                f.fused_tile_pick_applicable = applic >= 3;
                                                f.bf_rows_built = bf;
                                                f.fused_waves = 16;
                                                f.opt_kernel = opt_kernel;
                                                f.opt_fused_pick = fused_pick;
                                                f.opt_bestfit_stages = stages;
                                                f.opt_pick_from_mask = from_mask;
                                                f.combine = combine_op(f.flags);
                                                const EvalPlan now = plan_eval(f), was = plan_eval_as_it_was(f);
                                                CHECK(f.combine == CombineOp::kNone && now.combine == CombineOp::kNone);
                                                CHECK(same_plan(now, was));
                                                ++plans;
                                                errors += now.error != KSCHED_OK;
                                            }
    CHECK(plans > 100000 && errors > 0 && errors < plans);
    std::printf("no op: %u plans compared with the plan as it was (%u of them refusals)\n", plans, errors);
}

int main() {
    the_flags_and_their_ops();
    the_argument_rules();
    the_valid_bits_word();
    the_width_rule();
    the_geometry();
    for (const Op &o : kOps) the_plan_of_a_combining_request(o);
    without_an_op_every_plan_is_what_it_was();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
