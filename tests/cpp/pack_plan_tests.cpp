// pack_plan_tests.cpp -- host-side check of the plan of a KSCHED_PICK_PACK request (csrc/eval_plan.hpp) and of the pipe's waits for it
// (csrc/pipe_plan.hpp), no GPU and no HIP: the mask kernel always runs (fused or direct, as for a mask-only request), the pack pick follows
// it, nothing else is planned; a pipe submit with the flag waits for what a spread submit waits for.  The expectations of plan_eval are
// written out here, not computed by it.
#include <cstdio>
#include <cstring>

#include "../../kube_scheduler_rs_reference_amd/csrc/eval_plan.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/pipe_plan.hpp"

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

// the pack pick behind `mask`, and nothing else
static bool pack_behind(const EvalPlan &pl, MaskKernel mask, bool scratch) {
    return pl.error == KSCHED_OK && pl.why == PlanError::kNone && pl.mask == mask && pl.scratch_mask == scratch &&
           pl.pack == PackPick::kFromMask && pl.spread == SpreadPick::kNone && pl.uniform == UniformPick::kNone &&
           pl.sampled == SampledPick::kNone && pl.bestfit == BestfitPick::kNone && !pl.pick_rides() && !pl.bestfit_rows() &&
           pl.pick_from_mask() && is(pl.last_pick, "pack") && is(pl.last_kernel, mask == MaskKernel::kFused ? "fused" : "direct");
}

static void the_mask_kernel_always_runs() {
    for (uint32_t attempts : {1u, 2u, 5u, 64u}) {
        EvalFacts f = step(KSCHED_PICK_PACK, attempts);
        CHECK(pack_behind(plan_eval(f), MaskKernel::kFused, false));
        f.have_feas = false;  // bindings only: the mask kernel writes the ctx's scratch mask
        CHECK(pack_behind(plan_eval(f), MaskKernel::kFused, true));
        f.have_fit = true;  // the fit mask alone beside the pick: still the scratch feasible mask
        f.flags |= KSCHED_WANT_FIT_MASK;
        CHECK(pack_behind(plan_eval(f), MaskKernel::kFused, true));
        f = step(KSCHED_PICK_PACK, attempts);
        f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = false;  // AUTO follows applicability
        CHECK(pack_behind(plan_eval(f), MaskKernel::kDirect, false));
        f.have_feas = false;
        CHECK(pack_behind(plan_eval(f), MaskKernel::kDirect, true));
        f = step(KSCHED_PICK_PACK, attempts);
        f.opt_kernel = KSCHED_KERNEL_DIRECT;  // KSCHED_OPT_KERNEL is honoured
        CHECK(pack_behind(plan_eval(f), MaskKernel::kDirect, false));
        f.opt_kernel = KSCHED_KERNEL_FUSED;
        CHECK(pack_behind(plan_eval(f), MaskKernel::kFused, false));
        // a forced fused kernel that does not apply: unsupported, nothing planned -- with and without the caller's mask
        f.fused_applicable = false;
        for (int have = 0; have < 2; ++have) {
            f.have_feas = have;
            const EvalPlan pl = plan_eval(f);
            CHECK(pl.error == KSCHED_E_UNSUPPORTED && pl.why == PlanError::kFusedNotApplicable && pl.mask == MaskKernel::kNone &&
                  pl.pack == PackPick::kNone && pl.spread == SpreadPick::kNone && pl.uniform == UniformPick::kNone &&
                  pl.sampled == SampledPick::kNone && pl.bestfit == BestfitPick::kNone && !pl.pick_from_mask());
        }
    }
}

// the mask kernel is the one a mask-only request of the same facts gets
static void the_mask_kernel_is_the_mask_only_requests() {
    for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
        for (int can = 0; can < 2; ++can) {
            EvalFacts a = step(KSCHED_PICK_PACK), b = step(0);
            a.opt_kernel = b.opt_kernel = opt;
            a.fused_applicable = b.fused_applicable = can;
            const EvalPlan pa = plan_eval(a), pb = plan_eval(b);
            CHECK(pa.error == pb.error && pa.mask == pb.mask && (pa.error || is(pa.last_kernel, pb.last_kernel)));
        }
}

// both option bits, the best-fit options and the state of the best-fit rows: none of them changes the plan
static void the_options_of_the_other_picks_do_not_apply() {
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
            for (int stages = 0; stages <= 2; ++stages)
                for (int bf = 0; bf < 2; ++bf) {
                    EvalFacts f = step(KSCHED_PICK_PACK);
                    f.opt_pick_from_mask = from_mask;
                    f.opt_fused_pick = fused_pick;
                    f.opt_bestfit_stages = stages;
                    f.bf_rows_built = bf;
                    f.fused_tile_pick_applicable = false;  // (KSCHED_OPT_FUSED_PICK = 3 would refuse a riding sampled pick here)
                    CHECK(pack_behind(plan_eval(f), MaskKernel::kFused, false));
                    f.have_feas = false;
                    f.p = 1u << 20;
                    CHECK(pack_behind(plan_eval(f), MaskKernel::kFused, true));
                }
    // pick_reads_mask: true under every option, with any predicates beside the flag
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int bf = 0; bf < 2; ++bf) {
            CHECK(pick_reads_mask(KSCHED_PICK_PACK, from_mask, bf));
            CHECK(pick_reads_mask(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_PACK, from_mask, bf));
        }
}

// the other picks' plans name no pack pick, and the spread pick's plan is what it was
static void the_other_picks_plan_no_pack_pick() {
    for (uint32_t pick : {0u, KSCHED_PICK_SAMPLED, KSCHED_PICK_BESTFIT, KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD})
        for (int have = 0; have < 2; ++have) {
            EvalFacts f = step(pick, 5);
            f.have_feas = have || !pick;
            const EvalPlan pl = plan_eval(f);
            CHECK(pl.error == KSCHED_OK && pl.pack == PackPick::kNone && !is(pl.last_pick, "pack"));
        }
    const EvalPlan s = plan_eval(step(KSCHED_PICK_SPREAD, 5));
    CHECK(s.spread == SpreadPick::kFromMask && s.mask == MaskKernel::kFused && !s.scratch_mask && is(s.last_pick, "spread") && s.pick_from_mask());
    CHECK(!pick_reads_mask(KSCHED_PICK_SAMPLED, false, true) && !pick_reads_mask(KSCHED_PICK_BESTFIT, false, true) &&
          !pick_reads_mask(KSCHED_FIT | KSCHED_SEL, true, false));
}

static bool same_plan(const PipePlan &a, const PipePlan &b) {
    return a.whole == b.whole && a.mask_stream == b.mask_stream && a.pick_stream == b.pick_stream &&
           a.mask_waits_pick_done == b.mask_waits_pick_done && a.mask_waits_mask_done == b.mask_waits_mask_done &&
           a.pick_waits_pick_done == b.pick_waits_pick_done && a.pick_waits_mask_done == b.pick_waits_mask_done &&
           a.record_mask_done == b.record_mask_done && a.next.mask_stream == b.next.mask_stream && a.next.pick_stream == b.next.pick_stream &&
           a.next.pick_read_mask == b.next.pick_read_mask;
}

// Every sequence of six submits to one slot, each a pack (or, in the twin run, a spread) submit or a sampled one, in every pipe mode and
// with the mode changing half way: submit by submit the two runs plan the same streams, waits and records.  A pack submit is split, its
// pick waits for its own mask kernel, and the slot's next mask kernel waits for that pick.
static void the_pipe_waits_for_what_a_spread_submit_waits_for() {
    for (int mode_a = 0; mode_a <= 4; ++mode_a)
        for (int mode_b = 0; mode_b <= 4; ++mode_b)
            for (uint32_t slot = 0; slot < 3; ++slot)
                for (uint32_t seq = 0; seq < 64; ++seq) {
                    PipeSlot sp, ss;
                    bool prev_pack = false;
                    for (int i = 0; i < 6; ++i) {
                        const bool ours = (seq >> i) & 1u;
                        const int mode = i < 3 ? mode_a : mode_b;
                        for (int opt = 0; opt < 2; ++opt) CHECK(!ours || pick_reads_mask(KSCHED_PICK_PACK, opt, true));
                        const bool rp = pick_reads_mask(ours ? KSCHED_PICK_PACK : KSCHED_PICK_SAMPLED, false, true);
                        const bool rs = pick_reads_mask(ours ? KSCHED_PICK_SPREAD : KSCHED_PICK_SAMPLED, false, true);
                        const PipePlan pp = plan_pipe_submit(sp, slot, mode, rp), ps = plan_pipe_submit(ss, slot, mode, rs);
                        CHECK(same_plan(pp, ps));
                        if (ours) CHECK(!pp.whole && pp.mask_stream == kPipeMaskStream && pp.pick_stream == kPipePickStream && pp.record_mask_done && pp.pick_waits_mask_done && pp.next.pick_read_mask);
                        if (prev_pack) CHECK(pp.mask_waits_pick_done);  // the slot's mask is not overwritten before its pack pick has read it
                        prev_pack = ours;
                        sp = pp.next;
                        ss = ps.next;
                    }
                }
}

int main() {
    CHECK(KSCHED_PICK_PACK == 0x100u);
    the_mask_kernel_always_runs();
    the_mask_kernel_is_the_mask_only_requests();
    the_options_of_the_other_picks_do_not_apply();
    the_other_picks_plan_no_pack_pick();
    the_pipe_waits_for_what_a_spread_submit_waits_for();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
