// soft_plan_tests.cpp -- host-side check of the rules of a soft combining evaluation (extension E7, KSCHED_COMBINE_SOFT:
// csrc/mask_combine_soft.hpp, csrc/eval_plan.hpp), no GPU and no HIP: the constant and what it leaves alone; every refusal, for the entry
// points that accept combining calls and for those that refuse them; the row rule on hand-written rows; the launch plan at each side of
// every switch it has (the group sizes 1 .. 64, registers against two reads), for both unit widths, and the launch executed on the CPU as
// k_mask_combine_soft walks it (every word below W touched by exactly one lane of exactly one group, no padding word ever); and the plan of
// a request with the bit against the plain combining plan.  The expectations are written out here, not computed by the header.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/eval_plan.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/mask_combine_soft.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static bool is(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

static const uint32_t kAnd = 0x200u, kOr = 0x400u, kAndNot = 0x800u, kSoft = 0x2000u;

// ---- the constant ----------------------------------------------------------------------------------------------------------------------
static void the_flag() {
    CHECK(KSCHED_COMBINE_SOFT == kSoft && (kSoft & (kSoft - 1u)) == 0);
    CHECK(KSCHED_COMBINE_ANY == 0xE00u && !(kSoft & KSCHED_COMBINE_ANY) && !(kSoft & 0x1FFu) && !(kSoft & 0x1000u));
    CHECK((KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_ANY | KSCHED_WANT_FIT_MASK) == 0x1FFu);
    CHECK(!combine_soft(0) && !combine_soft(0x1FFu) && !combine_soft(0xE00u) && !combine_soft(0x1000u) && !combine_soft(~kSoft));
    CHECK(combine_soft(kSoft) && combine_soft(kSoft | kAnd) && combine_soft(0xFFFFFFFFu));
    // the modifier does not change which op a word names
    for (uint32_t rest : {0u, 0x1FFu, (uint32_t)KSCHED_SEL}) {
        CHECK(combine_op(rest | kSoft) == CombineOp::kNone && combine_op(rest | kSoft | kAnd) == CombineOp::kAnd &&
              combine_op(rest | kSoft | kOr) == CombineOp::kOr && combine_op(rest | kSoft | kAndNot) == CombineOp::kAndNot);
        CHECK(at_most_one_combine(rest | kSoft) && at_most_one_combine(rest | kSoft | kAnd) && !at_most_one_combine(rest | kSoft | kAnd | kAndNot));
    }
}

// ---- the refusals -----------------------------------------------------------------------------------------------------------------------
static void the_argument_rules() {
    for (uint32_t rest : {0u, (uint32_t)KSCHED_FIT, (uint32_t)(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT), (uint32_t)(KSCHED_SEL | KSCHED_PICK_BESTFIT),
                          (uint32_t)(KSCHED_TAINT | KSCHED_PICK_SPREAD)}) {
        for (uint32_t op : {kAnd, kAndNot}) {
            const uint32_t f = rest | op | kSoft;
            CHECK(check_soft_args(f, true, true, false) == KSCHED_OK);          // accepted, the mask given, no fit mask
            CHECK(check_soft_args(f, false, true, false) == KSCHED_E_INVAL);    // an entry point that refuses combining calls, whatever it was given
            CHECK(check_soft_args(f, false, false, false) == KSCHED_E_INVAL);
            CHECK(check_soft_args(f, true, false, false) == KSCHED_E_INVAL);    // out_feasible == NULL
            CHECK(check_soft_args(f, true, true, true) == KSCHED_E_INVAL);      // out_fit
            CHECK(check_soft_args(f | KSCHED_WANT_FIT_MASK, true, true, false) == KSCHED_E_INVAL);
            CHECK(check_soft_args(f | KSCHED_WANT_FIT_MASK, true, true, true) == KSCHED_E_INVAL);
            for (uint32_t second : {kAnd, kOr, kAndNot})
                if (second != op) CHECK(check_soft_args(f | second, true, true, false) == KSCHED_E_INVAL);  // two ops at once
            CHECK(check_soft_args(rest | 0xE00u | kSoft, true, true, false) == KSCHED_E_INVAL);
            // without the modifier the rule is check_combine_args'
            for (int accepted = 0; accepted < 2; ++accepted)
                for (int feas = 0; feas < 2; ++feas)
                    for (int fit = 0; fit < 2; ++fit)
                        CHECK(check_soft_args(rest | op, accepted, feas, fit) == check_combine_args(rest | op, accepted, feas, fit));
        }
        // the modifier with OR, and with no op: refused by accepting and refusing entry points alike, whatever the outputs
        for (int accepted = 0; accepted < 2; ++accepted)
            for (int feas = 0; feas < 2; ++feas)
                for (int fit = 0; fit < 2; ++fit) {
                    CHECK(check_soft_args(rest | kOr | kSoft, accepted, feas, fit) == KSCHED_E_INVAL);
                    CHECK(check_soft_args(rest | kSoft, accepted, feas, fit) == KSCHED_E_INVAL);
                    // a word with neither: the rule says nothing
                    CHECK(check_soft_args(rest, accepted, feas, fit) == KSCHED_OK);
                    CHECK(check_soft_args(rest | KSCHED_WANT_FIT_MASK, accepted, feas, fit) == KSCHED_OK);
                    CHECK(check_soft_args(rest | 0x1000u, accepted, feas, fit) == KSCHED_OK);  // (unknown: refused by the caller's `known` set)
                }
        CHECK(check_soft_args(rest | kOr, true, true, false) == KSCHED_OK);  // plain OR stays a combining call
    }
}

// ---- the row rule ---------------------------------------------------------------------------------------------------------------------
static void the_row_rule() {
    const uint64_t ones = ~0ull;
    struct Case {
        uint32_t n;
        CombineOp op;
        std::vector<uint64_t> old_row, new_row, want;
        bool narrows;
    };
    const Case cases[] = {
        {65, CombineOp::kAnd, {0, 0}, {ones, 1}, {0, 0}, false},                       // an empty row stays empty
        {65, CombineOp::kAndNot, {0, 0}, {0, 0}, {0, 0}, false},
        {65, CombineOp::kAnd, {0, ones << 1}, {ones, 1}, {0, 0}, false},               // only garbage at and beyond n: counts as empty, comes out zero
        {65, CombineOp::kAnd, {0x6, ones}, {0x4, 0}, {0x4, 0}, true},                  // narrows; the garbage goes
        {65, CombineOp::kAnd, {0x6, ones}, {0x9, 0}, {0x6, 1}, false},                 // would empty: old' (node 64 was set, bits beyond cleared)
        {65, CombineOp::kAnd, {0x6, ones}, {0, 1}, {0, 1}, true},                      // the only surviving bit is node n - 1
        {65, CombineOp::kAnd, {0x6, ones & ~1ull}, {0, 2}, {0x6, 0}, false},           // the only surviving bit would be node n: dropped
        {65, CombineOp::kAndNot, {0x6, ones}, {0x6, 0}, {0, 1}, true},                 // AND-NOT leaves node n - 1
        {65, CombineOp::kAndNot, {0x6, ones & ~1ull}, {0x6, 0}, {0x6, 0}, false},      // AND-NOT would leave only bits beyond n: dropped
        {65, CombineOp::kAndNot, {0x6, 1}, {ones, ones}, {0x6, 1}, false},
        {1, CombineOp::kAnd, {ones}, {1}, {1}, true},
        {1, CombineOp::kAnd, {ones}, {0}, {1}, false},
        {1, CombineOp::kAndNot, {ones}, {1}, {1}, false},
        {1, CombineOp::kAnd, {ones & ~1ull}, {1}, {0}, false},
        {63, CombineOp::kAnd, {ones}, {1ull << 62}, {1ull << 62}, true},
        {63, CombineOp::kAnd, {ones}, {1ull << 63}, {ones >> 1}, false},
        {64, CombineOp::kAnd, {ones}, {1ull << 63}, {1ull << 63}, true},
        {64, CombineOp::kAndNot, {ones}, {ones}, {ones}, false},
        {64, CombineOp::kAndNot, {ones}, {ones >> 1}, {1ull << 63}, true},
    };
    for (const Case &c : cases) {
        std::vector<uint64_t> row = c.old_row;
        const bool narrowed = soft_row(c.op, row.data(), c.new_row.data(), (uint32_t)row.size(), c.n);
        CHECK(narrowed == c.narrows);
        CHECK(row == c.want);
    }
}

// ---- the launch plan ----------------------------------------------------------------------------------------------------------------------
struct Shape {
    uint32_t units_per_row, group, shift, units_per_lane;
    bool keep;
};
// each side of every switch: the group doubles at 4 * 2^k | + 1 units per row up to the wave; registers up to 8 units per lane
static const Shape kShapes[] = {{1, 1, 0, 1, true},     {2, 1, 0, 2, true},     {3, 1, 0, 3, true},     {4, 1, 0, 4, true},      {5, 2, 1, 3, true},
                                {8, 2, 1, 4, true},     {9, 4, 2, 3, true},     {16, 4, 2, 4, true},    {17, 8, 3, 3, true},     {32, 8, 3, 4, true},
                                {33, 16, 4, 3, true},   {40, 16, 4, 3, true},   {64, 16, 4, 4, true},   {65, 32, 5, 3, true},    {128, 32, 5, 4, true},
                                {129, 64, 6, 3, true},  {256, 64, 6, 4, true},  {257, 64, 6, 5, true},  {391, 64, 6, 7, true},   {512, 64, 6, 8, true},
                                {513, 64, 6, 9, false}, {1000, 64, 6, 16, false}};

static bool shaped(const SoftLaunch &l, uint32_t vec, const Shape &s) {
    return l.vec == vec && l.units_per_row == s.units_per_row && l.group == s.group && l.group_shift == s.shift && l.units_per_lane == s.units_per_lane &&
           l.keep == s.keep && l.rows_per_block == 256u / s.group && l.block == 256u;
}

// every thread of the launch walks as k_mask_combine_soft does; `seen` counts the visits of every word of a [p][pitch] buffer
static void walk(uint32_t p, uint32_t W, uint32_t pitch, uint32_t vec) {
    const SoftLaunch l = plan_soft_launch(p, W, vec);
    CHECK(l.grid >= 1u && l.grid <= 2048u && l.rows_per_pass == l.grid * l.rows_per_block && l.rows_per_pass <= (1u << 19));
    CHECK((uint64_t)l.rows_per_pass >= (p < 2048u * l.rows_per_block ? p : 2048u * l.rows_per_block));
    CHECK(l.passes == ((uint64_t)p + l.rows_per_pass - 1) / l.rows_per_pass && (1u << l.group_shift) == l.group && l.group <= 64u);
    CHECK((uint64_t)l.units_per_lane * l.group >= l.units_per_row && (uint64_t)(l.units_per_lane - 1u) * l.group < l.units_per_row);
    CHECK(l.keep == (l.units_per_lane <= 8u) && (l.keep || l.group == 64u));
    std::vector<uint8_t> seen((size_t)p * pitch, 0);
    std::vector<uint32_t> group_of_row(p, 0xFFFFFFFFu);
    uint64_t most = 0;
    const uint32_t threads = l.grid * l.block;
    for (uint32_t t = 0; t < threads; ++t) {
        const uint32_t j = t & (l.group - 1u), group_id = t >> l.group_shift;
        CHECK((t & 63u) - j + l.group <= 64u);  // the group lies in one wave
        uint64_t rows = 0;
        for (uint64_t row = group_id; row < p; row += l.rows_per_pass) {
            ++rows;
            if (group_of_row[row] == 0xFFFFFFFFu) group_of_row[row] = group_id;
            if (group_of_row[row] != group_id) CHECK(!"a row is shared by two groups");
            for (uint32_t k = 0; k < l.units_per_lane; ++k) {
                const uint32_t col = j + (k << l.group_shift);
                if (col >= l.units_per_row) continue;
                const uint32_t w0 = vec == 2 ? 2u * col : col;
                if (w0 >= W) { CHECK(!"a unit starts in the padding"); continue; }
                ++seen[(size_t)row * pitch + w0];
                if (vec == 2 && w0 + 1u < W) ++seen[(size_t)row * pitch + w0 + 1u];
            }
        }
        if (rows > most) most = rows;
    }
    CHECK(most == l.passes);
    bool once = true, padding_alone = true;
    for (uint32_t r = 0; r < p; ++r)
        for (uint32_t w = 0; w < pitch; ++w) {
            const uint8_t s = seen[(size_t)r * pitch + w];
            if (w < W ? s != 1 : s != 0) (w < W ? once : padding_alone) = false;
        }
    CHECK(once);
    CHECK(padding_alone);
}

static void the_launch() {
    CHECK(kSoftBlock == 256u && kSoftMaxGrid == 2048u && kSoftWave == 64u && kSoftLaneUnits == 4u && kSoftKeepUnits == 8u);
    for (const Shape &s : kShapes) {
        // one-word units: W = units; 16-byte units: W = 2 * units and, ending in a one-word unit, 2 * units - 1
        CHECK(shaped(plan_soft_launch(1000, s.units_per_row, 1), 1, s));
        CHECK(shaped(plan_soft_launch(1000, 2u * s.units_per_row, 2), 2, s));
        CHECK(shaped(plan_soft_launch(1000, 2u * s.units_per_row - 1u, 2), 2, s));
        // executed: fewer rows than a block holds and more, packed and pitched
        const uint32_t rows_per_block = 256u / s.group;
        for (uint32_t p : {1u, 2u, 37u, rows_per_block, rows_per_block + 1u, 257u})
            for (uint32_t extra : {0u, 1u, 15u}) {
                walk(p, s.units_per_row, s.units_per_row + extra, 1);
                if ((extra & 1u) == 0) walk(p, 2u * s.units_per_row, 2u * s.units_per_row + extra, 2);
                else walk(p, 2u * s.units_per_row - 1u, 2u * s.units_per_row - 1u + extra, 2);
            }
    }
    // the numbers of a few launches
    SoftLaunch l = plan_soft_launch(1, 1, 1);
    CHECK(l.grid == 1 && l.rows_per_pass == 256 && l.passes == 1 && l.group == 1 && l.units_per_lane == 1 && l.keep);
    l = plan_soft_launch(1, 1, 2);  // the wide form of a one-word row: one one-word unit
    CHECK(l.grid == 1 && l.units_per_row == 1 && l.group == 1 && l.passes == 1);
    l = plan_soft_launch(256, 1, 1);
    CHECK(l.grid == 1 && l.passes == 1);
    l = plan_soft_launch(257, 1, 1);
    CHECK(l.grid == 2 && l.rows_per_pass == 512 && l.passes == 1);
    const uint32_t full = 2048u * 256u;  // rows of one word in one grid pass
    l = plan_soft_launch(full, 1, 1);
    CHECK(l.grid == 2048 && l.rows_per_pass == full && l.passes == 1);
    l = plan_soft_launch(full + 1, 1, 1);
    CHECK(l.grid == 2048 && l.rows_per_pass == full && l.passes == 2);
    l = plan_soft_launch(100000, 79, 2);  // C3 at the mask pitch: 40 units, 16 lanes a row, 3 units a lane
    CHECK(l.units_per_row == 40 && l.group == 16 && l.units_per_lane == 3 && l.keep && l.rows_per_block == 16 && l.grid == 2048 && l.rows_per_pass == 32768 && l.passes == 4);
    l = plan_soft_launch(100000, 79, 1);  // C3 packed: one-word units
    CHECK(l.units_per_row == 79 && l.group == 32 && l.units_per_lane == 3 && l.keep && l.rows_per_block == 8 && l.grid == 2048 && l.rows_per_pass == 16384 && l.passes == 7);
    l = plan_soft_launch(125000, 782, 2);  // the C5 shard: a wave per row, 7 units a lane, in registers
    CHECK(l.units_per_row == 391 && l.group == 64 && l.units_per_lane == 7 && l.keep && l.rows_per_block == 4 && l.grid == 2048 && l.rows_per_pass == 8192 && l.passes == 16);
    l = plan_soft_launch(0xFFFFFFFFu, 1, 1);
    CHECK(l.grid == 2048 && l.rows_per_pass == full && l.passes == 8192);
    l = plan_soft_launch(0xFFFFFFFFu, 1u << 26, 2);  // the longest row: read twice
    CHECK(l.units_per_row == (1u << 25) && l.group == 64 && l.units_per_lane == (1u << 19) && !l.keep && l.grid == 2048 && l.rows_per_pass == 8192);
    l = plan_soft_launch(0, 5, 1);
    CHECK(l.grid == 0 && l.passes == 0 && l.rows_per_pass == 0);  // nothing to launch
    // more than one grid pass: a lane a row, a wave a row in registers, a wave a row read twice
    walk(full + 1, 1, 1, 1);
    walk(full + 1, 2, 2, 2);
    walk(2048u * 4u + 1u, 258, 258, 2);
    walk(3u * 2048u * 4u + 5u, 129, 129, 1);
    walk(2048u * 4u + 1u, 1025, 1026, 2);
    walk(2048u * 4u + 1u, 513, 513, 1);
}

// ---- the plan of a request with the bit ---------------------------------------------------------------------------------------------------
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
    f.soft = combine_soft(f.flags);
    return f;
}

static bool same_but_soft(const EvalPlan &a, const EvalPlan &b) {
    return a.error == b.error && a.why == b.why && a.mask == b.mask && a.scratch_mask == b.scratch_mask && a.sampled == b.sampled && a.bestfit == b.bestfit &&
           a.ranked == b.ranked && a.combine == b.combine && is(a.last_kernel, b.last_kernel) && is(a.last_pick, b.last_pick);
}

static void the_plan_with_the_bit() {
    CHECK(!EvalFacts().soft && !EvalPlan().soft);
    for (uint32_t op : {kAnd, kAndNot})
        for (uint32_t pick : {0u, (uint32_t)KSCHED_PICK_SAMPLED, (uint32_t)KSCHED_PICK_BESTFIT, (uint32_t)KSCHED_PICK_UNIFORM, (uint32_t)KSCHED_PICK_SPREAD, (uint32_t)KSCHED_PICK_PACK})
            for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
                for (int can = 0; can < 2; ++can)
                    for (int from_mask = 0; from_mask < 2; ++from_mask)
                        for (int fused_pick = 0; fused_pick <= 3; ++fused_pick) {
                            EvalFacts a = step(op | kSoft | pick, 5), b = step(op | pick, 5);
                            for (EvalFacts *f : {&a, &b}) {
                                f->opt_kernel = opt;
                                f->fused_applicable = f->fused_pick_applicable = f->fused_tile_pick_applicable = can;
                                f->opt_pick_from_mask = from_mask;
                                f->opt_fused_pick = fused_pick;
                            }
                            CHECK(a.soft && !b.soft && a.combine == b.combine && a.combine != CombineOp::kNone);
                            const EvalPlan pa = plan_eval(a), pb = plan_eval(b);
                            CHECK(same_but_soft(pa, pb) && !pb.soft);
                            if (opt == KSCHED_KERNEL_FUSED && !can) CHECK(pa.error == KSCHED_E_UNSUPPORTED && !pa.soft && pa.combine == CombineOp::kNone);
                            else CHECK(pa.error == KSCHED_OK && pa.soft && pa.scratch_mask && !pa.pick_rides() && !pa.bestfit_rows());
                        }
    // without an op the field reaches no plan (check_soft_args refuses such a word before a plan is made)
    EvalFacts f = step(KSCHED_PICK_UNIFORM, 5);
    f.soft = true;
    CHECK(!plan_eval(f).soft && plan_eval(f).combine == CombineOp::kNone);
}

int main() {
    the_flag();
    the_argument_rules();
    the_row_rule();
    the_launch();
    the_plan_with_the_bit();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
