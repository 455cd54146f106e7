// spread_plan_tests.cpp -- host-side check of the plan of a KSCHED_PICK_SPREAD request (csrc/eval_plan.hpp), no GPU and no HIP: the
// mask kernel always runs (fused or direct, as for a mask-only request), the spread pick follows it, nothing else is planned.  The
// expectations are written out here, not computed by plan_eval.
#include <cstdio>
#include <cstring>

#include "../../kube_scheduler_rs_reference_amd/csrc/eval_plan.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static bool is(const char *a, const char *b) { return a && b && !std::strcmp(a, b); }

// a C3-like step (100 k pods x 5 k nodes, 5 tiles, every fused form applicable, default options) with `pick` and the mask wanted
static EvalFacts step(uint32_t pick, uint32_t attempts = 3) {
    EvalFacts f;
    f.p = 100000;
    f.n = 5000;
    f.attempts = attempts;
    f.flags = KSCHED_FIT | KSCHED_SEL | pick;
    f.nkeys = 8;
    f.have_feas = true;
    f.have_psel = true;
    f.tiles = 5;
    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = true;
    f.bf_rows_built = true;
    f.fused_waves = 16;
    return f;
}

// the spread pick behind `mask`, and nothing else
static bool spread_behind(const EvalPlan &pl, MaskKernel mask, bool scratch) {
    return pl.error == KSCHED_OK && pl.why == PlanError::kNone && pl.mask == mask && pl.scratch_mask == scratch &&
           pl.spread == SpreadPick::kFromMask && pl.uniform == UniformPick::kNone && pl.sampled == SampledPick::kNone &&
           pl.bestfit == BestfitPick::kNone && !pl.pick_rides() && !pl.bestfit_rows() && pl.pick_from_mask() && is(pl.last_pick, "spread") &&
           is(pl.last_kernel, mask == MaskKernel::kFused ? "fused" : "direct");
}

static void the_mask_kernel_always_runs() {
    for (uint32_t attempts : {1u, 2u, 5u, 64u}) {
        EvalFacts f = step(KSCHED_PICK_SPREAD, attempts);
        CHECK(spread_behind(plan_eval(f), MaskKernel::kFused, false));
        f.have_feas = false;  // bindings only: the mask kernel writes the ctx's scratch mask
        CHECK(spread_behind(plan_eval(f), MaskKernel::kFused, true));
        f.have_fit = true;  // the fit mask alone beside the pick: still the scratch feasible mask
        f.flags |= KSCHED_WANT_FIT_MASK;
        CHECK(spread_behind(plan_eval(f), MaskKernel::kFused, true));
        f = step(KSCHED_PICK_SPREAD, attempts);
        f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = false;  // AUTO follows applicability
        CHECK(spread_behind(plan_eval(f), MaskKernel::kDirect, false));
        f.have_feas = false;
        CHECK(spread_behind(plan_eval(f), MaskKernel::kDirect, true));
        f = step(KSCHED_PICK_SPREAD, attempts);
        f.opt_kernel = KSCHED_KERNEL_DIRECT;  // KSCHED_OPT_KERNEL is honoured
        CHECK(spread_behind(plan_eval(f), MaskKernel::kDirect, false));
        f.opt_kernel = KSCHED_KERNEL_FUSED;
        CHECK(spread_behind(plan_eval(f), MaskKernel::kFused, false));
        // a forced fused kernel that does not apply: unsupported, nothing planned -- with and without the caller's mask
        f.fused_applicable = false;
        for (int have = 0; have < 2; ++have) {
            f.have_feas = have;
            const EvalPlan pl = plan_eval(f);
            CHECK(pl.error == KSCHED_E_UNSUPPORTED && pl.why == PlanError::kFusedNotApplicable && pl.mask == MaskKernel::kNone &&
                  pl.spread == SpreadPick::kNone && pl.uniform == UniformPick::kNone && pl.sampled == SampledPick::kNone &&
                  pl.bestfit == BestfitPick::kNone && !pl.pick_from_mask());
        }
    }
}

// the mask kernel is the one a mask-only request of the same facts gets
static void the_mask_kernel_is_the_mask_only_requests() {
    for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
        for (int can = 0; can < 2; ++can) {
            EvalFacts a = step(KSCHED_PICK_SPREAD), b = step(0);
            a.opt_kernel = b.opt_kernel = opt;
            a.fused_applicable = b.fused_applicable = can;
            const EvalPlan pa = plan_eval(a), pb = plan_eval(b);
            CHECK(pa.error == pb.error && pa.mask == pb.mask && (pa.error || is(pa.last_kernel, pb.last_kernel)));
        }
}

static void the_options_of_the_other_picks_do_not_apply() {
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
            for (int stages = 0; stages <= 2; ++stages)
                for (int bf = 0; bf < 2; ++bf) {
                    EvalFacts f = step(KSCHED_PICK_SPREAD);
                    f.opt_pick_from_mask = from_mask;
                    f.opt_fused_pick = fused_pick;
                    f.opt_bestfit_stages = stages;
                    f.bf_rows_built = bf;
                    f.fused_tile_pick_applicable = false;  // (KSCHED_OPT_FUSED_PICK = 3 would refuse a riding sampled pick here)
                    CHECK(spread_behind(plan_eval(f), MaskKernel::kFused, false));
                    f.have_feas = false;
                    f.p = 1u << 20;
                    CHECK(spread_behind(plan_eval(f), MaskKernel::kFused, true));
                }
    // pick_reads_mask: true under every option, with any predicates beside the flag
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int bf = 0; bf < 2; ++bf) {
            CHECK(pick_reads_mask(KSCHED_PICK_SPREAD, from_mask, bf));
            CHECK(pick_reads_mask(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_SPREAD, from_mask, bf));
        }
}

// the other picks' plans name no spread pick, and the uniform pick's plan is what it was
static void the_other_picks_plan_no_spread_pick() {
    for (uint32_t pick : {0u, KSCHED_PICK_SAMPLED, KSCHED_PICK_BESTFIT, KSCHED_PICK_UNIFORM})
        for (int have = 0; have < 2; ++have) {
            EvalFacts f = step(pick, 5);
            f.have_feas = have || !pick;
            const EvalPlan pl = plan_eval(f);
            CHECK(pl.error == KSCHED_OK && pl.spread == SpreadPick::kNone && !is(pl.last_pick, "spread"));
        }
    const EvalPlan u = plan_eval(step(KSCHED_PICK_UNIFORM, 5));
    CHECK(u.uniform == UniformPick::kFromMask && u.mask == MaskKernel::kFused && !u.scratch_mask && is(u.last_pick, "uniform") && u.pick_from_mask());
    CHECK(!pick_reads_mask(KSCHED_PICK_SAMPLED, false, true) && !pick_reads_mask(KSCHED_PICK_BESTFIT, false, true) &&
          !pick_reads_mask(KSCHED_FIT | KSCHED_SEL, true, false));
}

int main() {
    CHECK(KSCHED_PICK_SPREAD == 0x80u);
    the_mask_kernel_always_runs();
    the_mask_kernel_is_the_mask_only_requests();
    the_options_of_the_other_picks_do_not_apply();
    the_other_picks_plan_no_spread_pick();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
