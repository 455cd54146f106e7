// plan_tests.cpp -- host-side check of the evaluation plan (csrc/eval_plan.hpp), no GPU and no HIP: which kernels a request runs,
// pinned at the boundaries of every rule.  The expectations restate the rules as the dispatch had them before the plan existed
// (and as DESIGN.md and the comments in eval_plan.hpp give them) -- they are written out here, not computed by plan_eval.
#include <algorithm>
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

// a C3-like step: 100 k pods x 5 k nodes (5 tiles), fit + selector, the sampled pick with five draws, the feasible mask wanted;
// an index on which every fused form applies; default options
static EvalFacts step() {
    EvalFacts f;
    f.p = 100000;
    f.n = 5000;
    f.attempts = 5;
    f.flags = KSCHED_FIT | KSCHED_SEL | KSCHED_PICK_SAMPLED;
    f.nkeys = 8;
    f.have_feas = true;
    f.have_psel = true;
    f.tiles = 5;
    f.nlist = 0;
    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = true;
    f.bf_rows_built = true;
    f.fused_waves = 16;
    return f;
}

// the same snapshot, the best-fit pick, bindings only
static EvalFacts bestfit(uint32_t p) {
    EvalFacts f = step();
    f.p = p;
    f.flags = KSCHED_FIT | KSCHED_SEL | KSCHED_PICK_BESTFIT;
    f.have_feas = false;
    return f;
}

static bool unsupported(const EvalPlan &pl, PlanError why) {
    return pl.error == KSCHED_E_UNSUPPORTED && pl.why == why && pl.mask == MaskKernel::kNone && pl.sampled == SampledPick::kNone &&
           pl.bestfit == BestfitPick::kNone;
}

// the fill form rides up to chunks * 5 * 64 * waves pods, chunks = max(1, min(cus / tiles, ceil(p / 256)))
static uint64_t fill_limit(uint32_t p, uint32_t tiles, uint32_t cus, uint32_t waves) {
    const uint32_t chunks = std::max(1u, std::min(cus / tiles, (p + 255u) / 256u));
    return (uint64_t)chunks * 5u * 64u * waves;
}

static void kernel_choice() {
    EvalFacts f = step();
    f.flags = KSCHED_FIT | KSCHED_SEL;  // the mask alone
    EvalPlan pl = plan_eval(f);
    CHECK(pl.error == KSCHED_OK && pl.mask == MaskKernel::kFused && is(pl.last_kernel, "fused") && is(pl.last_pick, "none"));
    CHECK(!pl.scratch_mask && pl.sampled == SampledPick::kNone && pl.bestfit == BestfitPick::kNone);
    f.fused_applicable = false;  // AUTO follows applicability
    pl = plan_eval(f);
    CHECK(pl.error == KSCHED_OK && pl.mask == MaskKernel::kDirect && is(pl.last_kernel, "direct"));
    f.opt_kernel = KSCHED_KERNEL_FUSED;  // forced without it
    CHECK(unsupported(plan_eval(f), PlanError::kFusedNotApplicable));
    f.opt_kernel = KSCHED_KERNEL_DIRECT;
    CHECK(plan_eval(f).mask == MaskKernel::kDirect);
    f.fused_applicable = true;  // forced direct on an indexed snapshot
    CHECK(plan_eval(f).mask == MaskKernel::kDirect);
    // a fit-mask-only request: the mask kernels always write the feasible mask, into a scratch one
    f = step();
    f.flags = KSCHED_FIT | KSCHED_WANT_FIT_MASK;
    f.have_feas = false;
    f.have_fit = true;
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kFused && pl.scratch_mask);
    // a forced fused kernel is no error where no mask kernel runs at all
    f = step();
    f.have_feas = false;
    f.fused_applicable = false;
    f.opt_kernel = KSCHED_KERNEL_FUSED;
    pl = plan_eval(f);
    CHECK(pl.error == KSCHED_OK && pl.mask == MaskKernel::kNone && pl.sampled == SampledPick::kOwnLaunch);
    f.have_feas = true;  // ... and is one as soon as a mask is wanted (the pick does not ride: it would be its own launch)
    CHECK(unsupported(plan_eval(f), PlanError::kFusedNotApplicable));
}

static void sampled_without_mask() {
    EvalFacts f = step();
    f.have_feas = false;
    const EvalPlan pl = plan_eval(f);
    CHECK(pl.error == KSCHED_OK && pl.sampled == SampledPick::kOwnLaunch && is(pl.last_pick, "select"));
    CHECK(pl.mask == MaskKernel::kNone && pl.last_kernel == nullptr && !pl.scratch_mask);
}

static void riding_default() {
    EvalFacts f = step();
    f.p = 1000;
    for (uint32_t tiles : {2u, 12u}) {
        f.tiles = tiles;
        const EvalPlan pl = plan_eval(f);
        CHECK(pl.sampled == SampledPick::kRidesTiles && pl.mask == MaskKernel::kFused && is(pl.last_pick, "fused-tile") && is(pl.last_kernel, "fused"));
    }
    for (uint32_t tiles : {1u, 13u}) {
        f.tiles = tiles;
        const EvalPlan pl = plan_eval(f);
        CHECK(pl.sampled == SampledPick::kRidesFill && pl.mask == MaskKernel::kFused && is(pl.last_pick, "fused"));
    }
    // tile tests ride up to 524 288 pods per call
    f.tiles = 5;
    f.p = 524288;
    CHECK(plan_eval(f).sampled == SampledPick::kRidesTiles);
    f.p = 524289;
    EvalPlan pl = plan_eval(f);
    CHECK(pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kFused && is(pl.last_pick, "select") && is(pl.last_kernel, "fused"));
    // the fill form: at most five rounds per wave
    struct Case {
        uint32_t tiles, grid_cus;
        bool tile_ok;
        uint64_t limit;  // written out: (cus / tiles) chunks x 5 rounds x 64 pods x 16 waves
    } cases[] = {
        {1, 0, true, 256ull * 5120},    // C2-like, whole chip
        {13, 0, true, 19ull * 5120},    // 256 / 13 = 19 chunks
        {13, 64, true, 4ull * 5120},    // KSCHED_OPT_GRID_CUS = 64
        {5, 0, false, 51ull * 5120},    // 2 .. 12 tiles, but the tile tests do not apply to the request (say, taints)
        {300, 0, true, 1ull * 5120},    // more tiles than compute units: one chunk
    };
    for (const Case &k : cases) {
        f = step();
        f.tiles = k.tiles;
        f.opt_grid_cus = k.grid_cus;
        f.fused_tile_pick_applicable = k.tile_ok;
        f.p = (uint32_t)k.limit;
        CHECK(k.limit == fill_limit(f.p, k.tiles, k.grid_cus ? k.grid_cus : 256u, 16));
        pl = plan_eval(f);
        CHECK(pl.sampled == SampledPick::kRidesFill && is(pl.last_pick, "fused"));
        f.p = (uint32_t)k.limit + 1;
        CHECK(k.limit == fill_limit(f.p, k.tiles, k.grid_cus ? k.grid_cus : 256u, 16));
        pl = plan_eval(f);
        CHECK(pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kFused && is(pl.last_pick, "select"));
    }
    // a short batch: ceil(p / 256) chunks bound the count, and every such batch rides
    f = step();
    f.tiles = 1;
    for (uint32_t p : {1u, 256u, 257u, 5120u, 5121u}) {
        f.p = p;
        CHECK((uint64_t)p <= fill_limit(p, 1, 256, 16) && plan_eval(f).sampled == SampledPick::kRidesFill);
    }
    // no riding on the direct kernel
    f = step();
    f.opt_kernel = KSCHED_KERNEL_DIRECT;
    pl = plan_eval(f);
    CHECK(pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kDirect);
}

static void riding_forced() {
    // 0: the pick is its own launch
    EvalFacts f = step();
    f.opt_fused_pick = 0;
    EvalPlan pl = plan_eval(f);
    CHECK(pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kFused && is(pl.last_pick, "select"));
    // 2: only as waves of the fill, whatever the tiles and however long the batch
    f.opt_fused_pick = 2;
    for (uint32_t tiles : {1u, 5u, 13u})
        for (uint32_t p : {1000u, 524289u, 2000000u}) {
            f.tiles = tiles;
            f.p = p;
            CHECK(plan_eval(f).sampled == SampledPick::kRidesFill);
        }
    // 3: only as tile tests, whatever the tiles and however long the batch ...
    f = step();
    f.opt_fused_pick = 3;
    for (uint32_t tiles : {1u, 5u, 13u})
        for (uint32_t p : {1000u, 524289u}) {
            f.tiles = tiles;
            f.p = p;
            pl = plan_eval(f);
            CHECK(pl.sampled == SampledPick::kRidesTiles && is(pl.last_pick, "fused-tile"));
        }
    // ... unsupported where they do not apply -- but only when the pick would ride
    f = step();
    f.opt_fused_pick = 3;
    f.fused_tile_pick_applicable = false;
    CHECK(unsupported(plan_eval(f), PlanError::kTilePickNotApplicable));
    EvalFacts g = f;
    g.have_feas = false;  // bindings only
    pl = plan_eval(g);
    CHECK(pl.error == KSCHED_OK && pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kNone);
    g = f;
    g.opt_kernel = KSCHED_KERNEL_DIRECT;
    pl = plan_eval(g);
    CHECK(pl.error == KSCHED_OK && pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kDirect);
    g = f;
    g.fused_pick_applicable = false;
    pl = plan_eval(g);
    CHECK(pl.error == KSCHED_OK && pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kFused);
    g = f;
    g.opt_pick_from_mask = true;
    pl = plan_eval(g);
    CHECK(pl.error == KSCHED_OK && pl.sampled == SampledPick::kFromMask);
    // a wanted fit mask, or list keys (fused_pick_applicable says no to both): the pick never rides
    for (int opt : {1, 2, 3}) {
        f = step();
        f.opt_fused_pick = opt;
        f.p = 1000;
        f.fused_pick_applicable = false;
        f.flags |= KSCHED_WANT_FIT_MASK;
        f.have_fit = true;
        pl = plan_eval(f);
        CHECK(pl.error == KSCHED_OK && pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kFused && is(pl.last_pick, "select"));
        f = step();
        f.opt_fused_pick = opt;
        f.p = 1000;
        f.fused_pick_applicable = false;
        f.nlist = 1;
        pl = plan_eval(f);
        CHECK(pl.error == KSCHED_OK && pl.sampled == SampledPick::kOwnLaunch && pl.mask == MaskKernel::kFused && is(pl.last_pick, "select"));
    }
}

static void from_mask() {
    EvalFacts f = step();
    f.opt_pick_from_mask = true;
    EvalPlan pl = plan_eval(f);
    CHECK(pl.sampled == SampledPick::kFromMask && pl.mask == MaskKernel::kFused && !pl.scratch_mask && is(pl.last_pick, "from-mask"));
    f.have_feas = false;  // the caller gave no mask: a scratch one
    pl = plan_eval(f);
    CHECK(pl.sampled == SampledPick::kFromMask && pl.mask == MaskKernel::kFused && pl.scratch_mask && is(pl.last_pick, "from-mask"));
    f = bestfit(1000);
    f.opt_pick_from_mask = true;
    pl = plan_eval(f);
    CHECK(pl.bestfit == BestfitPick::kFromMask && pl.mask == MaskKernel::kFused && pl.scratch_mask && is(pl.last_pick, "from-mask"));
    f = bestfit(1000);  // no best-fit rows (a snapshot without an index): the mask-reading best fit on the direct kernel
    f.bf_rows_built = false;
    f.fused_applicable = false;
    pl = plan_eval(f);
    CHECK(pl.bestfit == BestfitPick::kFromMask && pl.mask == MaskKernel::kDirect && pl.scratch_mask && is(pl.last_pick, "from-mask"));

    CHECK(!pick_reads_mask(KSCHED_FIT, true, false));  // no pick, nothing to read
    CHECK(!pick_reads_mask(KSCHED_PICK_SAMPLED, false, false) && !pick_reads_mask(KSCHED_PICK_SAMPLED, false, true));
    CHECK(pick_reads_mask(KSCHED_PICK_SAMPLED, true, true));
    CHECK(!pick_reads_mask(KSCHED_PICK_BESTFIT, false, true));
    CHECK(pick_reads_mask(KSCHED_PICK_BESTFIT, false, false) && pick_reads_mask(KSCHED_PICK_BESTFIT, true, true));
}

static void best_fit() {
    // one stage below 24 576 pods, two from there on
    EvalPlan pl = plan_eval(bestfit(24575));
    CHECK(pl.bestfit == BestfitPick::kRowsOneStage && pl.mask == MaskKernel::kNone && pl.last_kernel == nullptr && is(pl.last_pick, "bestfit-rows"));
    CHECK(plan_eval(bestfit(24576)).bestfit == BestfitPick::kRowsTwoStages);
    // KSCHED_OPT_BESTFIT_STAGES
    EvalFacts f = bestfit(100000);
    f.opt_bestfit_stages = 1;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsOneStage);
    f = bestfit(10);
    f.opt_bestfit_stages = 2;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsTwoStages);
    // list keys force two stages plus the listed kernel
    for (int stages : {0, 1, 2}) {
        f = bestfit(10);
        f.nlist = 2;
        f.opt_bestfit_stages = stages;
        f.debug = 0x400u;
        CHECK(plan_eval(f).bestfit == BestfitPick::kRowsTwoStagesListed);
    }
    f = bestfit(10);  // ... when the request has an active selector term: selectors given, the flag, keys in the snapshot
    f.nlist = 2;
    f.have_psel = false;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsOneStage);
    f.have_psel = true;
    f.flags &= ~(uint32_t)KSCHED_SEL;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsOneStage);
    // more than 2^21 nodes: one stage without list keys, unsupported with them
    f = bestfit(100000);
    f.n = 1u << 21;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsTwoStages);
    f.n = (1u << 21) + 1u;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsOneStage);
    f.nlist = 1;
    CHECK(unsupported(plan_eval(f), PlanError::kListKeysTooManyNodes));
    f.n = 1u << 21;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsTwoStagesListed);
    // debug bit 0x400 forces one stage
    f = bestfit(100000);
    f.debug = 0x400u;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsOneStage);
    f.opt_bestfit_stages = 2;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsOneStage);
    // with a mask wanted as well: the rows, then the mask kernel; the pick does not read the mask
    f = bestfit(1000);
    f.have_feas = true;
    pl = plan_eval(f);
    CHECK(pl.bestfit == BestfitPick::kRowsOneStage && pl.mask == MaskKernel::kFused && !pl.scratch_mask && is(pl.last_pick, "bestfit-rows") &&
          is(pl.last_kernel, "fused"));
    f.fused_applicable = false;
    f.opt_kernel = KSCHED_KERNEL_FUSED;
    CHECK(unsupported(plan_eval(f), PlanError::kFusedNotApplicable));
}

int main() {
    kernel_choice();
    sampled_without_mask();
    riding_default();
    riding_forced();
    from_mask();
    best_fit();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
