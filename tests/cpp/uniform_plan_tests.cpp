// uniform_plan_tests.cpp -- host-side check of the plan of a KSCHED_PICK_UNIFORM request (csrc/eval_plan.hpp), no GPU and no HIP:
// the mask kernel always runs, the pick follows it, nothing else is planned -- and a handful of today's requests still get today's
// plans.  The expectations are written out here, not computed by plan_eval.
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

// a C3-like step (100 k pods x 5 k nodes, 5 tiles, every fused form applicable, default options) with the uniform pick and the mask wanted
static EvalFacts step(uint32_t pick) {
    EvalFacts f;
    f.p = 100000;
    f.n = 5000;
    f.attempts = 5;
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

// the uniform pick behind `mask`, and nothing else
static bool uniform_behind(const EvalPlan &pl, MaskKernel mask, bool scratch) {
    return pl.error == KSCHED_OK && pl.why == PlanError::kNone && pl.mask == mask && pl.scratch_mask == scratch &&
           pl.uniform == UniformPick::kFromMask && pl.sampled == SampledPick::kNone && pl.bestfit == BestfitPick::kNone && !pl.pick_rides() &&
           !pl.bestfit_rows() && pl.pick_from_mask() && is(pl.last_pick, "uniform") &&
           is(pl.last_kernel, mask == MaskKernel::kFused ? "fused" : "direct");
}

static void the_mask_kernel_always_runs() {
    EvalFacts f = step(KSCHED_PICK_UNIFORM);
    CHECK(uniform_behind(plan_eval(f), MaskKernel::kFused, false));
    f.have_feas = false;  // bindings only: the mask kernel writes the ctx's scratch mask
    CHECK(uniform_behind(plan_eval(f), MaskKernel::kFused, true));
    f.have_fit = true;  // the fit mask alone beside the pick: still the scratch feasible mask
    f.flags |= KSCHED_WANT_FIT_MASK;
    CHECK(uniform_behind(plan_eval(f), MaskKernel::kFused, true));
    f = step(KSCHED_PICK_UNIFORM);
    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = false;  // AUTO follows applicability
    CHECK(uniform_behind(plan_eval(f), MaskKernel::kDirect, false));
    f.have_feas = false;
    CHECK(uniform_behind(plan_eval(f), MaskKernel::kDirect, true));
    f = step(KSCHED_PICK_UNIFORM);
    f.opt_kernel = KSCHED_KERNEL_DIRECT;  // KSCHED_OPT_KERNEL is honoured
    CHECK(uniform_behind(plan_eval(f), MaskKernel::kDirect, false));
    f.opt_kernel = KSCHED_KERNEL_FUSED;
    CHECK(uniform_behind(plan_eval(f), MaskKernel::kFused, false));
    // a forced fused kernel that does not apply: unsupported, nothing planned -- with and without the caller's mask
    f.fused_applicable = false;
    for (int have = 0; have < 2; ++have) {
        f.have_feas = have;
        const EvalPlan pl = plan_eval(f);
        CHECK(pl.error == KSCHED_E_UNSUPPORTED && pl.why == PlanError::kFusedNotApplicable && pl.mask == MaskKernel::kNone &&
              pl.uniform == UniformPick::kNone && pl.sampled == SampledPick::kNone && pl.bestfit == BestfitPick::kNone && !pl.pick_from_mask());
    }
}

static void the_options_of_the_other_picks_do_not_apply() {
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
            for (int stages = 0; stages <= 2; ++stages)
                for (int bf = 0; bf < 2; ++bf) {
                    EvalFacts f = step(KSCHED_PICK_UNIFORM);
                    f.opt_pick_from_mask = from_mask;
                    f.opt_fused_pick = fused_pick;
                    f.opt_bestfit_stages = stages;
                    f.bf_rows_built = bf;
                    f.fused_tile_pick_applicable = false;  // (KSCHED_OPT_FUSED_PICK = 3 would refuse a riding sampled pick here)
                    CHECK(uniform_behind(plan_eval(f), MaskKernel::kFused, false));
                    f.have_feas = false;
                    f.p = 1u << 20;
                    CHECK(uniform_behind(plan_eval(f), MaskKernel::kFused, true));
                }
    // pick_reads_mask: true for all four combinations of (KSCHED_OPT_PICK_FROM_MASK, best-fit rows), with any predicates beside the flag
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int bf = 0; bf < 2; ++bf) {
            CHECK(pick_reads_mask(KSCHED_PICK_UNIFORM, from_mask, bf));
            CHECK(pick_reads_mask(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_UNIFORM, from_mask, bf));
        }
}

// what plan_eval answers today for today's flags
static void todays_requests_get_todays_plans() {
    CHECK(!pick_reads_mask(KSCHED_PICK_SAMPLED, false, true) && pick_reads_mask(KSCHED_PICK_SAMPLED, true, true));
    CHECK(!pick_reads_mask(KSCHED_PICK_BESTFIT, false, true) && pick_reads_mask(KSCHED_PICK_BESTFIT, false, false));
    CHECK(!pick_reads_mask(KSCHED_FIT | KSCHED_SEL, true, false));
    EvalFacts f = step(0);  // the mask alone
    EvalPlan pl = plan_eval(f);
    CHECK(pl.error == KSCHED_OK && pl.mask == MaskKernel::kFused && !pl.scratch_mask && pl.sampled == SampledPick::kNone &&
          pl.bestfit == BestfitPick::kNone && pl.uniform == UniformPick::kNone && !pl.pick_from_mask() && is(pl.last_pick, "none"));
    f = step(KSCHED_PICK_SAMPLED);  // mask + sampled pick at C3: rides as tile tests
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kFused && pl.sampled == SampledPick::kRidesTiles && pl.uniform == UniformPick::kNone && is(pl.last_pick, "fused-tile") &&
          !pl.pick_from_mask());
    f.have_feas = false;  // bindings only: the pick alone, no mask kernel
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kNone && pl.sampled == SampledPick::kOwnLaunch && !pl.scratch_mask && pl.last_kernel == nullptr && is(pl.last_pick, "select"));
    f.opt_pick_from_mask = true;  // the cross-check form: scratch mask + the pick from it
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kFused && pl.scratch_mask && pl.sampled == SampledPick::kFromMask && pl.pick_from_mask() && is(pl.last_pick, "from-mask") &&
          pl.uniform == UniformPick::kNone);
    f = step(KSCHED_PICK_BESTFIT);  // best fit, bindings only: one stage below 24576 pods, two from there on
    f.have_feas = false;
    f.p = 24575;
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kNone && pl.bestfit == BestfitPick::kRowsOneStage && is(pl.last_pick, "bestfit-rows") && pl.uniform == UniformPick::kNone);
    f.p = 24576;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsTwoStages);
    f.bf_rows_built = false;  // no best-fit rows: from the mask
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kFused && pl.scratch_mask && pl.bestfit == BestfitPick::kFromMask && pl.pick_from_mask() && is(pl.last_pick, "from-mask"));
    f = step(0);  // forced fused where it does not apply
    f.fused_applicable = false;
    f.opt_kernel = KSCHED_KERNEL_FUSED;
    pl = plan_eval(f);
    CHECK(pl.error == KSCHED_E_UNSUPPORTED && pl.why == PlanError::kFusedNotApplicable);
}

int main() {
    the_mask_kernel_always_runs();
    the_options_of_the_other_picks_do_not_apply();
    todays_requests_get_todays_plans();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
