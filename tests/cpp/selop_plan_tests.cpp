// selop_plan_tests.cpp -- host-side check of the rules of an operator call (extension E8, KSCHED_SELOP_EXISTS / _GT / _LT:
// csrc/sel_ops.hpp, csrc/eval_plan.hpp), no GPU and no HIP: the constants and what they leave alone; every refusal and every accepted
// combination of check_selop_args; the rule for one (entry, id) pair on hand-written pairs and selop_row against a loop over single bits
// written here; the launch plan at its boundaries, and every launch walked on the CPU as k_eval_selop walks it (every word below W of every
// row by exactly one lane of exactly one wave, no padding word ever, every key by exactly one pass); the plan of an operator call -- with
// and without a combine, soft, each pick, KSCHED_OPT_KERNEL forced --; and that a request without an operator gets the plan it got before
// the field existed (plan_eval_as_it_was below).  The expectations are written out here, not computed by the header.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/eval_plan.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/mask_combine_soft.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/sel_ops.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static bool is(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

static const uint32_t kExists = 0x4000u, kGt = 0x8000u, kLt = 0x10000u, kAny = 0x1C000u;
static const uint32_t kAnd = 0x200u, kOr = 0x400u, kAndNot = 0x800u, kSoft = 0x2000u;
static const uint32_t kNever = 0xFFFFFFFFu;
static const uint32_t kOpFlags[] = {kExists, kGt, kLt};
static const SelOp kOps[] = {SelOp::kExists, SelOp::kGt, SelOp::kLt};
static const uint32_t kPicks[] = {0u, KSCHED_PICK_SAMPLED, KSCHED_PICK_BESTFIT, KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD, KSCHED_PICK_PACK};

// ---- the constants ---------------------------------------------------------------------------------------------------------------------
static void the_flags() {
    CHECK(KSCHED_SELOP_EXISTS == kExists && KSCHED_SELOP_GT == kGt && KSCHED_SELOP_LT == kLt && KSCHED_SELOP_ANY == kAny);
    for (uint32_t f : kOpFlags) CHECK((f & (f - 1u)) == 0 && !(f & 0x1FFu) && !(f & 0xE00u) && !(f & 0x2000u) && !(f & 0x1000u));
    CHECK((KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_ANY | KSCHED_WANT_FIT_MASK) == 0x1FFu && KSCHED_COMBINE_ANY == 0xE00u && KSCHED_COMBINE_SOFT == 0x2000u);
    CHECK(KSCHED_SEL_NEVER == kNever && KSCHED_ABI_VERSION == 7u);
    for (uint32_t rest : {0u, 0x1FFu, 0xE00u, 0x2000u, 0x1000u, 0x3FFFu, 0xFFFE0000u}) {
        CHECK(sel_op(rest) == SelOp::kNone && at_most_one_selop(rest));
        CHECK(sel_op(rest | kExists) == SelOp::kExists && sel_op(rest | kGt) == SelOp::kGt && sel_op(rest | kLt) == SelOp::kLt);
        CHECK(at_most_one_selop(rest | kExists) && at_most_one_selop(rest | kGt) && at_most_one_selop(rest | kLt));
        CHECK(!at_most_one_selop(rest | kExists | kGt) && !at_most_one_selop(rest | kGt | kLt) && !at_most_one_selop(rest | kExists | kLt) && !at_most_one_selop(rest | kAny));
        CHECK(sel_op(rest | kExists | kGt) == SelOp::kNone && sel_op(rest | kAny) == SelOp::kNone);
        // an operator flag changes neither the combine op of a word nor its modifier
        CHECK(combine_op(rest | kGt) == combine_op(rest) && combine_soft(rest | kAny) == combine_soft(rest));
    }
}

// ---- the refusals -----------------------------------------------------------------------------------------------------------------------
static void the_argument_rules() {
    for (uint32_t op : kOpFlags) {
        // accepted: SEL and the operator; a combine op, the modifier and a pick beside them change nothing here (their rules are their own)
        for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
            for (uint32_t pick : kPicks) {
                const uint32_t f = KSCHED_SEL | op | comb | pick;
                CHECK(check_selop_args(f, true, false) == KSCHED_OK);
                CHECK(check_selop_args(f, false, false) == KSCHED_E_INVAL);  // an entry point that takes no operator call
                CHECK(check_selop_args(f, true, true) == KSCHED_E_INVAL);    // out_fit
                CHECK(check_selop_args(f, false, true) == KSCHED_E_INVAL);
                CHECK(check_selop_args(f & ~(uint32_t)KSCHED_SEL, true, false) == KSCHED_E_INVAL);  // no KSCHED_SEL
                CHECK(check_selop_args(f | KSCHED_FIT, true, false) == KSCHED_E_INVAL);
                CHECK(check_selop_args(f | KSCHED_TAINT, true, false) == KSCHED_E_INVAL);
                CHECK(check_selop_args(f | KSCHED_FIT | KSCHED_TAINT, true, false) == KSCHED_E_INVAL);
                CHECK(check_selop_args(f | KSCHED_WANT_FIT_MASK, true, false) == KSCHED_E_INVAL);
                CHECK(check_selop_args(f | KSCHED_WANT_FIT_MASK, true, true) == KSCHED_E_INVAL);
                for (uint32_t second : kOpFlags)
                    if (second != op) CHECK(check_selop_args(f | second, true, false) == KSCHED_E_INVAL);  // two operators at once
                CHECK(check_selop_args(f | kAny, true, false) == KSCHED_E_INVAL);
            }
        CHECK(check_selop_args(op, true, false) == KSCHED_E_INVAL);  // the flag alone
    }
    // a word without an operator flag: the rule says nothing, whatever the rest
    for (uint32_t rest : {0u, 0x1FFu, (uint32_t)KSCHED_SEL, (uint32_t)(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT), 0xE00u, kSoft, 0x1000u, (uint32_t)KSCHED_WANT_FIT_MASK})
        for (int accepted = 0; accepted < 2; ++accepted)
            for (int fit = 0; fit < 2; ++fit) CHECK(check_selop_args(rest, accepted, fit) == KSCHED_OK);
    // the combine's and the modifier's own rules hold beside an operator flag as beside none
    for (uint32_t op : kOpFlags)
        for (uint32_t comb : {kAnd, kOr, kAndNot, kAnd | kSoft, kOr | kSoft, kSoft, kAnd | kOr})
            for (int accepted = 0; accepted < 2; ++accepted)
                for (int feas = 0; feas < 2; ++feas)
                    CHECK(check_soft_args(KSCHED_SEL | op | comb, accepted, feas, false) == check_soft_args(KSCHED_SEL | comb, accepted, feas, false));
}

// ---- one pair, one row ------------------------------------------------------------------------------------------------------------------
static void the_pair_rule() {
    struct Pair {
        uint32_t e, v;
        bool exists, gt, lt;
    };
    const Pair pairs[] = {
        {0, 0, true, true, true},        {0, 5, true, true, true},        {0, 0xFFFFFFFEu, true, true, true},
        {kNever, 0, false, false, false}, {kNever, 5, false, false, false}, {kNever, 0xFFFFFFFEu, false, false, false},
        {1, 0, false, false, false},     {1, 1, true, false, false},      {1, 2, true, true, false},
        {2, 1, true, false, true},       {2, 2, true, false, false},      {2, 0, false, false, false},
        {0x7FFFFFFFu, 0x80000000u, true, true, false}, {0x80000000u, 0x7FFFFFFFu, true, false, true},
        {0x7FFFFFFFu, 0xFFFFFFFEu, true, true, false}, {0xFFFFFFFEu, 0x7FFFFFFFu, true, false, true},
        {0x80000000u, 0xFFFFFFFEu, true, true, false}, {0xFFFFFFFEu, 0x80000000u, true, false, true},
        {0x80000000u, 1, true, false, true},           {1, 0x80000000u, true, true, false},
        {0xFFFFFFFEu, 0xFFFFFFFEu, true, false, false}, {0xFFFFFFFEu, 0xFFFFFFFDu, true, false, true},
        {0xFFFFFFFEu, 0, false, false, false},         {0x80000000u, 0, false, false, false},  // absent under LT with a large bound
    };
    for (const Pair &q : pairs) {
        CHECK(selop_pass(SelOp::kExists, q.e, q.v) == q.exists);
        CHECK(selop_pass(SelOp::kGt, q.e, q.v) == q.gt);
        CHECK(selop_pass(SelOp::kLt, q.e, q.v) == q.lt);
    }
    // what the kernel computes in their place: GT as the bare v > e, LT as v - 1 < e - 1, for every constrained entry
    const uint32_t ids[] = {0u, 1u, 2u, 3u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFDu, 0xFFFFFFFEu};
    for (uint32_t e : ids)
        for (uint32_t v : ids)
            if (e != 0u) {
                CHECK(selop_pass(SelOp::kGt, e, v) == (v > e));
                CHECK(selop_pass(SelOp::kLt, e, v) == ((uint32_t)(v - 1u) < (uint32_t)(e - 1u)));
            }
}

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static void the_row_rule() {
    const uint32_t pool[] = {0u, 1u, 2u, 3u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu};
    uint32_t seed = 0xE8u;
    unsigned rows = 0, full = 0, empty = 0;
    for (uint32_t n : {1u, 63u, 64u, 65u, 130u})
        for (uint32_t nkeys : {1u, 2u, 9u})
            for (SelOp op : kOps) {
                const uint32_t p = 7, W = (n + 63u) / 64u;
                std::vector<uint32_t> lab((size_t)nkeys * n), sel((size_t)nkeys * p);
                for (uint32_t &v : lab) v = pool[(lcg(seed) >> 8) % 7u];
                for (uint32_t &e : sel) {
                    const uint32_t r = (lcg(seed) >> 8) % 16u;
                    e = r < 7u ? pool[r] : r == 7u ? kNever : 0u;
                }
                for (uint32_t pod = 0; pod < p; ++pod) {
                    std::vector<uint64_t> row(W, ~0ull), want(W, 0);
                    selop_row(op, lab.data(), sel.data(), nkeys, n, p, pod, row.data());
                    for (uint32_t node = 0; node < n; ++node) {  // bit by bit, from the header's table
                        bool ok = true;
                        for (uint32_t k = 0; k < nkeys; ++k) {
                            const uint32_t e = sel[(size_t)k * p + pod], v = lab[(size_t)k * n + node];
                            if (e == 0u) continue;
                            if (e == kNever || v == 0u) ok = false;
                            else if (op == SelOp::kGt && !(v > e)) ok = false;
                            else if (op == SelOp::kLt && !(v < e)) ok = false;
                        }
                        if (ok) want[node / 64u] |= 1ull << (node % 64u);
                    }
                    CHECK(row == want);
                    ++rows;
                    bool all = true, none = true;
                    for (uint32_t w = 0; w < W; ++w) {
                        all = all && want[w] == (w + 1u < W || n % 64u == 0 ? ~0ull : (1ull << (n % 64u)) - 1ull);
                        none = none && want[w] == 0;
                    }
                    full += all;
                    empty += none;
                }
                // no selectors, and no keys: every node passes, padding bits zero
                std::vector<uint64_t> row(W, 0x5A5Aull);
                selop_row(op, lab.data(), nullptr, nkeys, n, p, 0, row.data());
                std::vector<uint64_t> row0(W, 0x5A5Aull);
                selop_row(op, nullptr, sel.data(), 0, n, p, 0, row0.data());
                for (uint32_t w = 0; w < W; ++w) {
                    const uint64_t valid = (w + 1u < W || n % 64u == 0) ? ~0ull : (1ull << (n % 64u)) - 1ull;
                    CHECK(row[w] == valid && row0[w] == valid);
                }
            }
    CHECK(rows == 5u * 3u * 3u * 7u && full > 0 && empty > 0 && full + empty < rows);
}

// ---- the launch plan ----------------------------------------------------------------------------------------------------------------------
// every thread block of every pass walks as k_eval_selop does; `seen` counts the stores into every word of a [p][pitch] buffer by the first
// pass (the later passes touch the same words: they AND into them)
static void walk(uint32_t p, uint32_t W, uint32_t pitch, uint32_t nkeys) {
    const SelopLaunch l = plan_selop_launch(p, W, nkeys);
    CHECK(l.block == 256u && l.gx == (W + 15u) / 16u && l.gy >= 1u && l.gy <= 2048u && l.pod_tiles == (p + 63u) / 64u);
    CHECK((uint64_t)l.gy * l.pod_tiles_per_block >= l.pod_tiles && (uint64_t)(l.gy - 1u) * l.pod_tiles_per_block < l.pod_tiles);
    CHECK(l.passes == (nkeys == 0 ? 1u : (nkeys + 7u) / 8u));
    // the keys: every key by exactly one pass, at most eight a pass, only the first pass overwrites
    std::vector<uint8_t> key_seen(nkeys, 0);
    for (uint32_t pass = 0; pass < l.passes; ++pass) {
        const uint32_t k0 = selop_pass_key0(pass), nk = selop_pass_keys(nkeys, pass);
        CHECK(k0 == 8u * pass && nk <= 8u && (nk > 0 || nkeys == 0) && k0 + nk <= nkeys);
        for (uint32_t k = 0; k < nk; ++k) ++key_seen[k0 + k];
    }
    for (uint8_t s : key_seen) CHECK(s == 1);
    CHECK(selop_pass_keys(nkeys, l.passes) == 0u);
    std::vector<uint8_t> seen((size_t)p * pitch, 0);
    for (uint32_t by = 0; by < l.gy; ++by)
        for (uint32_t bx = 0; bx < l.gx; ++bx)
            for (uint32_t wave = 0; wave < 4u; ++wave) {
                const uint32_t w0 = (bx * 4u + wave) * 4u;
                if (w0 >= W) continue;
                for (uint32_t t = 0; t < l.pod_tiles_per_block; ++t) {
                    const uint64_t first = (uint64_t)(by * l.pod_tiles_per_block + t) * 64u;
                    if (first >= p) break;
                    const uint32_t jmax = p - (uint32_t)first < 64u ? p - (uint32_t)first : 64u;
                    for (uint32_t lane = 0; lane < jmax; ++lane)
                        for (uint32_t c = 0; c < 4u; ++c)
                            if (w0 + c < W) ++seen[((size_t)first + lane) * pitch + w0 + c];
                }
            }
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
    CHECK(kSelopCW == 4u && kSelopWaves == 4u && kSelopKeys == 8u && kSelopTargetBlocks == 2048u && KSCHED_MAX_KEYS == 32u);
    for (uint32_t p : {1u, 63u, 64u, 65u, 129u, 4097u})
        for (uint32_t W : {1u, 2u, 4u, 5u, 15u, 16u, 17u, 33u, 65u})
            for (uint32_t extra : {0u, 1u, 15u})
                for (uint32_t nkeys : {0u, 1u, 8u, 9u, 16u, 17u, 32u}) walk(p, W, W + extra, nkeys);
    // the numbers of a few launches
    SelopLaunch l = plan_selop_launch(1, 1, 1);
    CHECK(l.gx == 1 && l.gy == 1 && l.pod_tiles == 1 && l.pod_tiles_per_block == 1 && l.passes == 1);
    l = plan_selop_launch(100000, 79, 8);  // C3: 5 column blocks, 391 block rows of 4 tiles (the last one of 3)
    CHECK(l.gx == 5 && l.pod_tiles == 1563 && l.gy == 391 && l.pod_tiles_per_block == 4 && l.passes == 1);
    l = plan_selop_launch(100000, 79, 9);
    CHECK(l.gx == 5 && l.passes == 2);
    l = plan_selop_launch(64, 16, 32);  // one block
    CHECK(l.gx == 1 && l.gy == 1 && l.pod_tiles_per_block == 1 && l.passes == 4);
    l = plan_selop_launch(65, 17, 0);  // one word and one pod more: two column blocks, two tiles, two block rows
    CHECK(l.gx == 2 && l.pod_tiles == 2 && l.gy == 2 && l.pod_tiles_per_block == 1 && l.passes == 1);
    l = plan_selop_launch(0xFFFFFFFFu, 1, 8);  // the most pods: the tile count does not wrap
    CHECK(l.gx == 1 && l.pod_tiles == (1u << 26) && l.gy == 2048 && l.pod_tiles_per_block == (1u << 15));
    l = plan_selop_launch(1000, 1u << 26, 8);  // the most nodes: one block row
    CHECK(l.gx == (1u << 22) && l.gy == 1 && l.pod_tiles == 16 && l.pod_tiles_per_block == 16);
    // the geometry the standing legs rely on (tests/apply_paths_worker.py case_sizes, tests/test_gpu_selop.py): 3000 pods over 50 000 and
    // 60 000 nodes -- 47 tiles, two a block, 24 block rows: 48 slots, so the last block breaks at `first >= p` --; 130 pods over 1024
    // column blocks; and a walk's 2000 pods over 4097 nodes with ten keys, which stays at one tile a block and takes two passes
    l = plan_selop_launch(3000, 782, 8);
    CHECK(l.gx == 49 && l.pod_tiles == 47 && l.pod_tiles_per_block == 2 && l.gy == 24 && l.passes == 1);
    l = plan_selop_launch(3000, 938, 8);
    CHECK(l.gx == 59 && l.pod_tiles == 47 && l.pod_tiles_per_block == 2 && l.gy == 24 && l.passes == 1);
    l = plan_selop_launch(130, 16384, 2);
    CHECK(l.gx == 1024 && l.pod_tiles == 3 && l.gy == 2 && l.pod_tiles_per_block == 2 && l.passes == 1);
    l = plan_selop_launch(2000, 65, 10);
    CHECK(l.gx == 5 && l.pod_tiles == 32 && l.gy == 32 && l.pod_tiles_per_block == 1 && l.passes == 2);
    walk(3000, 782, 784, 8);
    walk(130, 16384, 16384, 2);
    l = plan_selop_launch(0, 5, 8);
    CHECK(l.gx == 0 && l.gy == 0 && l.passes == 0);  // nothing to launch
    l = plan_selop_launch(5, 0, 8);
    CHECK(l.gx == 0 && l.gy == 0 && l.passes == 0);
    walk(2048u * 64u + 1u, 1, 1, 8);  // one pod more than 2048 block rows of one tile
    walk(3u * 2048u * 64u + 65u, 3, 4, 9);
}

// ---- the plan of an operator call -----------------------------------------------------------------------------------------------------------
static EvalFacts step(uint32_t flags, bool have_feas) {
    EvalFacts f;
    f.p = 100000;
    f.n = 5000;
    f.attempts = flags & KSCHED_PICK_DRAWS ? 5 : 0;
    f.flags = flags;
    f.nkeys = 8;
    f.have_feas = have_feas;
    f.have_psel = flags & KSCHED_SEL;
    f.tiles = 5;
    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = true;
    f.bf_rows_built = true;
    f.fused_waves = 16;
    f.combine = combine_op(flags);
    f.soft = combine_soft(flags);
    f.selop = sel_op(flags);
    return f;
}

static void the_plan_of_an_operator_call() {
    CHECK(EvalFacts().selop == SelOp::kNone && EvalPlan().selop == SelOp::kNone);
    unsigned plans = 0;
    for (int i = 0; i < 3; ++i)
        for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
            for (uint32_t pick : kPicks)
                for (int have_feas = 0; have_feas < 2; ++have_feas)
                    for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
                        for (int can = 0; can < 2; ++can)
                            for (int from_mask = 0; from_mask < 2; ++from_mask)
                                for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
                                    for (int bf = 0; bf < 2; ++bf) {
                                        if (comb && !have_feas) continue;  // (check_combine_args refuses a combining call without its mask)
                                        if (!pick && !have_feas) continue;  // (check_eval_args refuses a call with nothing to write)
                                        EvalFacts f = step(KSCHED_SEL | kOpFlags[i] | comb | pick, have_feas);
                                        f.opt_kernel = opt;
                                        f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = can;
                                        f.opt_pick_from_mask = from_mask;
                                        f.opt_fused_pick = fused_pick;
                                        f.bf_rows_built = bf;
                                        const EvalPlan pl = plan_eval(f);
                                        ++plans;
                                        // the operator kernel, whatever KSCHED_OPT_KERNEL says and whether or not the snapshot has an index
                                        CHECK(pl.error == KSCHED_OK && pl.why == PlanError::kNone);
                                        CHECK(pl.mask == MaskKernel::kSelOp && pl.selop == kOps[i] && is(pl.last_kernel, "selop"));
                                        CHECK(pl.combine == combine_op(comb) && pl.soft == ((comb & kSoft) != 0));
                                        CHECK(pl.scratch_mask == (comb != 0 || !have_feas));
                                        CHECK(!pl.pick_rides() && !pl.bestfit_rows());
                                        CHECK(pl.pick_from_mask() == (pick != 0));
                                        const char *name = !pick ? "none" : pick == KSCHED_PICK_UNIFORM ? "uniform" : pick == KSCHED_PICK_SPREAD ? "spread" :
                                                           pick == KSCHED_PICK_PACK ? "pack" : "from-mask";
                                        CHECK(is(pl.last_pick, name));
                                        CHECK(pl.sampled == (pick == KSCHED_PICK_SAMPLED ? SampledPick::kFromMask : SampledPick::kNone));
                                        CHECK(pl.bestfit == (pick == KSCHED_PICK_BESTFIT ? BestfitPick::kFromMask : BestfitPick::kNone));
                                        CHECK(pl.ranked == (pick == KSCHED_PICK_UNIFORM ? RankedPick::kUniform : pick == KSCHED_PICK_SPREAD ? RankedPick::kSpread :
                                                            pick == KSCHED_PICK_PACK ? RankedPick::kPack : RankedPick::kNone));
                                    }
    CHECK(plans > 5000);
    // the modifier without an op reaches no plan (check_soft_args refuses such a word before a plan is made)
    EvalFacts f = step(KSCHED_SEL | kGt, true);
    f.soft = true;
    CHECK(!plan_eval(f).soft && plan_eval(f).combine == CombineOp::kNone);
}

// ---- no operator: today's plans -------------------------------------------------------------------------------------------------------------
// plan_eval as it was before EvalFacts and EvalPlan had the selop field (the parent's function, word for word)
static EvalPlan plan_eval_as_it_was(const EvalFacts &f) {
    EvalPlan plan;
    const uint32_t p = f.p, flags = f.flags;
    const bool pick_s = flags & KSCHED_PICK_SAMPLED, pick_b = flags & KSCHED_PICK_BESTFIT;
    const bool want_mask = f.have_feas || f.have_fit;
    const bool can_fused = f.fused_applicable;
    const int kern = choose_kernel(f.opt_kernel, can_fused);
    if (f.combine != CombineOp::kNone) {
        if (kern == KSCHED_KERNEL_FUSED && !can_fused) return plan_unsupported(PlanError::kFusedNotApplicable);
        plan.combine = f.combine;
        plan.soft = f.soft;
        plan.scratch_mask = true;
        plan.mask = kern == KSCHED_KERNEL_FUSED ? MaskKernel::kFused : MaskKernel::kDirect;
        plan.last_kernel = kern == KSCHED_KERNEL_FUSED ? "fused" : "direct";
        if (const RankedMember *m = ranked_member(flags)) {
            plan.ranked = m->pick;
            plan.last_pick = m->name;
        } else if (pick_s || pick_b) {
            if (pick_s) plan.sampled = SampledPick::kFromMask;
            else plan.bestfit = BestfitPick::kFromMask;
            plan.last_pick = "from-mask";
        }
        return plan;
    }
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
           a.ranked == b.ranked && a.combine == b.combine && a.soft == b.soft && is(a.last_kernel, b.last_kernel) && is(a.last_pick, b.last_pick);
}

// the facts tests/cpp/combine_plan_tests.cpp walks for "no op", and the same with each combine op (and the modifier) beside them
static void without_an_operator_every_plan_is_what_it_was() {
    const uint32_t preds[] = {KSCHED_FIT, KSCHED_FIT | KSCHED_SEL, KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT};
    unsigned plans = 0, errors = 0;
    for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
        for (uint32_t pick : kPicks)
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
                                                    if (comb && outs != 1u) continue;  // (a combining call has its mask and no fit mask)
                                                    EvalFacts f;
                                                    f.p = p;
                                                    f.n = shape == 3 ? kBfLanesMaxNodes + 1 : 5000;
                                                    f.attempts = pick & KSCHED_PICK_DRAWS ? 5 : 0;
                                                    f.flags = pred | pick | comb | ((outs & 2u) ? KSCHED_WANT_FIT_MASK : 0u);
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
                                                    f.soft = combine_soft(f.flags);
                                                    f.selop = sel_op(f.flags);
                                                    const EvalPlan now = plan_eval(f), was = plan_eval_as_it_was(f);
                                                    CHECK(f.selop == SelOp::kNone && now.selop == SelOp::kNone && now.mask != MaskKernel::kSelOp);
                                                    CHECK(same_plan(now, was));
                                                    ++plans;
                                                    errors += now.error != KSCHED_OK;
                                                }
    CHECK(plans > 100000 && errors > 0 && errors < plans);
    std::printf("no operator: %u plans compared with the plan as it was (%u of them refusals)\n", plans, errors);
}

int main() {
    the_flags();
    the_argument_rules();
    the_pair_rule();
    the_row_rule();
    the_launch();
    the_plan_of_an_operator_call();
    without_an_operator_every_plan_is_what_it_was();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
