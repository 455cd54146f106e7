// ranked_plan_tests.cpp -- host-side check of the plan of a ranked-pick request (KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD, KSCHED_PICK_PACK:
// csrc/eval_plan.hpp) and of the pipe's waits for it (csrc/pipe_plan.hpp), no GPU and no HIP: the mask kernel always runs (fused or direct,
// as for a mask-only request), the member's pick follows it, nothing else is planned; a pipe submit with one member's flag waits for what a
// submit with another member's waits for -- and a handful of today's requests still get today's plans.  Every check runs for every member.
// The expectations are written out here, the members' names included, not computed by plan_eval.
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

// the family: the flag, its value in the ABI, what the plan calls the member and what ksched_last_pick says
struct Member {
    uint32_t flag, value;
    RankedPick pick;
    const char *name;
};
static const Member kMembers[] = {{KSCHED_PICK_UNIFORM, 0x40u, RankedPick::kUniform, "uniform"},
                                  {KSCHED_PICK_SPREAD, 0x80u, RankedPick::kSpread, "spread"},
                                  {KSCHED_PICK_PACK, 0x100u, RankedPick::kPack, "pack"}};

// a C3-like step (100 k pods x 5 k nodes, 5 tiles, every fused form applicable, default options) with `pick` and the mask wanted
static EvalFacts step(uint32_t pick, uint32_t attempts) {
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

// the member's pick behind `mask`, and nothing else (one field: no other member can be planned beside it)
static bool ranked_behind(const EvalPlan &pl, const Member &m, MaskKernel mask, bool scratch) {
    return pl.error == KSCHED_OK && pl.why == PlanError::kNone && pl.mask == mask && pl.scratch_mask == scratch && pl.ranked == m.pick &&
           pl.sampled == SampledPick::kNone && pl.bestfit == BestfitPick::kNone && !pl.pick_rides() && !pl.bestfit_rows() &&
           pl.pick_from_mask() && is(pl.last_pick, m.name) && is(pl.last_kernel, mask == MaskKernel::kFused ? "fused" : "direct");
}

static void the_mask_kernel_always_runs(const Member &m) {
    for (uint32_t attempts : {1u, 2u, 3u, 5u, 64u}) {
        EvalFacts f = step(m.flag, attempts);
        CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kFused, false));
        f.have_feas = false;  // bindings only: the mask kernel writes the ctx's scratch mask
        CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kFused, true));
        f.have_fit = true;  // the fit mask alone beside the pick: still the scratch feasible mask
        f.flags |= KSCHED_WANT_FIT_MASK;
        CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kFused, true));
        f = step(m.flag, attempts);
        f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = false;  // AUTO follows applicability
        CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kDirect, false));
        f.have_feas = false;
        CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kDirect, true));
        f = step(m.flag, attempts);
        f.opt_kernel = KSCHED_KERNEL_DIRECT;  // KSCHED_OPT_KERNEL is honoured
        CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kDirect, false));
        f.opt_kernel = KSCHED_KERNEL_FUSED;
        CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kFused, false));
        // a forced fused kernel that does not apply: unsupported, nothing planned -- with and without the caller's mask
        f.fused_applicable = false;
        for (int have = 0; have < 2; ++have) {
            f.have_feas = have;
            const EvalPlan pl = plan_eval(f);
            CHECK(pl.error == KSCHED_E_UNSUPPORTED && pl.why == PlanError::kFusedNotApplicable && pl.mask == MaskKernel::kNone &&
                  pl.ranked == RankedPick::kNone && pl.sampled == SampledPick::kNone && pl.bestfit == BestfitPick::kNone && !pl.pick_from_mask());
        }
    }
}

// the mask kernel is the one a mask-only request of the same facts gets
static void the_mask_kernel_is_the_mask_only_requests(const Member &m) {
    for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
        for (int can = 0; can < 2; ++can) {
            EvalFacts a = step(m.flag, 3), b = step(0, 3);
            a.opt_kernel = b.opt_kernel = opt;
            a.fused_applicable = b.fused_applicable = can;
            const EvalPlan pa = plan_eval(a), pb = plan_eval(b);
            CHECK(pa.error == pb.error && pa.mask == pb.mask && (pa.error || is(pa.last_kernel, pb.last_kernel)));
        }
}

// both option bits, the best-fit options and the state of the best-fit rows: none of them changes the plan
static void the_options_of_the_other_picks_do_not_apply(const Member &m) {
    for (uint32_t attempts : {3u, 5u})
        for (int from_mask = 0; from_mask < 2; ++from_mask)
            for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
                for (int stages = 0; stages <= 2; ++stages)
                    for (int bf = 0; bf < 2; ++bf)
                        for (int have_fit = 0; have_fit < 2; ++have_fit) {
                            EvalFacts f = step(m.flag, attempts);
                            f.opt_pick_from_mask = from_mask;
                            f.opt_fused_pick = fused_pick;
                            f.opt_bestfit_stages = stages;
                            f.bf_rows_built = bf;
                            f.fused_tile_pick_applicable = false;  // (KSCHED_OPT_FUSED_PICK = 3 would refuse a riding sampled pick here)
                            f.have_fit = have_fit;
                            if (have_fit) f.flags |= KSCHED_WANT_FIT_MASK;
                            CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kFused, false));
                            f.have_feas = false;
                            f.p = 1u << 20;
                            CHECK(ranked_behind(plan_eval(f), m, MaskKernel::kFused, true));
                        }
    // pick_reads_mask: true for all four combinations of (KSCHED_OPT_PICK_FROM_MASK, best-fit rows), with any predicates beside the flag
    for (int from_mask = 0; from_mask < 2; ++from_mask)
        for (int bf = 0; bf < 2; ++bf) {
            CHECK(pick_reads_mask(m.flag, from_mask, bf));
            CHECK(pick_reads_mask(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | m.flag, from_mask, bf));
        }
}

// the other picks' plans do not name this member, and the other members' plans are their own
static void the_other_picks_plan_no_pick_of_this_member(const Member &m) {
    for (uint32_t pick : {0u, KSCHED_PICK_SAMPLED, KSCHED_PICK_BESTFIT, KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD, KSCHED_PICK_PACK}) {
        if (pick == m.flag) continue;
        for (int have = 0; have < 2; ++have) {
            EvalFacts f = step(pick, 5);
            f.have_feas = have || !pick;
            const EvalPlan pl = plan_eval(f);
            CHECK(pl.error == KSCHED_OK && pl.ranked != m.pick && !is(pl.last_pick, m.name));
        }
    }
    for (const Member &o : kMembers) {
        if (o.flag == m.flag) continue;
        const EvalPlan pl = plan_eval(step(o.flag, 5));
        CHECK(pl.ranked == o.pick && pl.mask == MaskKernel::kFused && !pl.scratch_mask && is(pl.last_pick, o.name) && pl.pick_from_mask());
    }
    CHECK(!pick_reads_mask(KSCHED_PICK_SAMPLED, false, true) && !pick_reads_mask(KSCHED_PICK_BESTFIT, false, true) &&
          !pick_reads_mask(KSCHED_FIT | KSCHED_SEL, true, false));
}

// what plan_eval answers today for today's flags: no ranked pick in any of them
static void todays_requests_get_todays_plans() {
    CHECK(!pick_reads_mask(KSCHED_PICK_SAMPLED, false, true) && pick_reads_mask(KSCHED_PICK_SAMPLED, true, true));
    CHECK(!pick_reads_mask(KSCHED_PICK_BESTFIT, false, true) && pick_reads_mask(KSCHED_PICK_BESTFIT, false, false));
    CHECK(!pick_reads_mask(KSCHED_FIT | KSCHED_SEL, true, false));
    EvalFacts f = step(0, 5);  // the mask alone
    EvalPlan pl = plan_eval(f);
    CHECK(pl.error == KSCHED_OK && pl.mask == MaskKernel::kFused && !pl.scratch_mask && pl.sampled == SampledPick::kNone &&
          pl.bestfit == BestfitPick::kNone && pl.ranked == RankedPick::kNone && !pl.pick_from_mask() && is(pl.last_pick, "none"));
    f = step(KSCHED_PICK_SAMPLED, 5);  // mask + sampled pick at C3: rides as tile tests
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kFused && pl.sampled == SampledPick::kRidesTiles && pl.ranked == RankedPick::kNone && is(pl.last_pick, "fused-tile") &&
          !pl.pick_from_mask());
    f.have_feas = false;  // bindings only: the pick alone, no mask kernel
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kNone && pl.sampled == SampledPick::kOwnLaunch && !pl.scratch_mask && pl.last_kernel == nullptr && is(pl.last_pick, "select"));
    f.opt_pick_from_mask = true;  // the cross-check form: scratch mask + the pick from it
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kFused && pl.scratch_mask && pl.sampled == SampledPick::kFromMask && pl.pick_from_mask() && is(pl.last_pick, "from-mask") &&
          pl.ranked == RankedPick::kNone);
    f = step(KSCHED_PICK_BESTFIT, 5);  // best fit, bindings only: one stage below 24576 pods, two from there on
    f.have_feas = false;
    f.p = 24575;
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kNone && pl.bestfit == BestfitPick::kRowsOneStage && is(pl.last_pick, "bestfit-rows") && pl.ranked == RankedPick::kNone);
    f.p = 24576;
    CHECK(plan_eval(f).bestfit == BestfitPick::kRowsTwoStages);
    f.bf_rows_built = false;  // no best-fit rows: from the mask
    pl = plan_eval(f);
    CHECK(pl.mask == MaskKernel::kFused && pl.scratch_mask && pl.bestfit == BestfitPick::kFromMask && pl.pick_from_mask() && is(pl.last_pick, "from-mask"));
    f = step(0, 5);  // forced fused where it does not apply
    f.fused_applicable = false;
    f.opt_kernel = KSCHED_KERNEL_FUSED;
    pl = plan_eval(f);
    CHECK(pl.error == KSCHED_E_UNSUPPORTED && pl.why == PlanError::kFusedNotApplicable);
}

static bool same_plan(const PipePlan &a, const PipePlan &b) {
    return a.whole == b.whole && a.mask_stream == b.mask_stream && a.pick_stream == b.pick_stream &&
           a.mask_waits_pick_done == b.mask_waits_pick_done && a.mask_waits_mask_done == b.mask_waits_mask_done &&
           a.pick_waits_pick_done == b.pick_waits_pick_done && a.pick_waits_mask_done == b.pick_waits_mask_done &&
           a.record_mask_done == b.record_mask_done && a.next.mask_stream == b.next.mask_stream && a.next.pick_stream == b.next.pick_stream &&
           a.next.pick_read_mask == b.next.pick_read_mask;
}

// Every sequence of six submits to one slot, each a submit with member m's pick (in the twin run: with member o's) or a sampled one, in
// every pipe mode and with the mode changing half way: submit by submit the two runs plan the same streams, waits and records.  A ranked
// submit is split, its pick waits for its own mask kernel, and the slot's next mask kernel waits for that pick.
static void the_pipe_waits_for_what_another_members_submit_waits_for(const Member &m, const Member &o) {
    for (int mode_a = 0; mode_a <= 4; ++mode_a)
        for (int mode_b = 0; mode_b <= 4; ++mode_b)
            for (uint32_t slot = 0; slot < 3; ++slot)
                for (uint32_t seq = 0; seq < 64; ++seq) {
                    PipeSlot sm, so;
                    bool prev_ours = false;
                    for (int i = 0; i < 6; ++i) {
                        const bool ours = (seq >> i) & 1u;
                        const int mode = i < 3 ? mode_a : mode_b;
                        for (int opt = 0; opt < 2; ++opt) CHECK(!ours || pick_reads_mask(m.flag, opt, true));
                        const bool rm = pick_reads_mask(ours ? m.flag : KSCHED_PICK_SAMPLED, false, true);
                        const bool ro = pick_reads_mask(ours ? o.flag : KSCHED_PICK_SAMPLED, false, true);
                        const PipePlan pm = plan_pipe_submit(sm, slot, mode, rm), po = plan_pipe_submit(so, slot, mode, ro);
                        CHECK(same_plan(pm, po));
                        if (ours) CHECK(!pm.whole && pm.mask_stream == kPipeMaskStream && pm.pick_stream == kPipePickStream && pm.record_mask_done && pm.pick_waits_mask_done && pm.next.pick_read_mask);
                        if (prev_ours) CHECK(pm.mask_waits_pick_done);  // the slot's mask is not overwritten before its ranked pick has read it
                        prev_ours = ours;
                        sm = pm.next;
                        so = po.next;
                    }
                }
}

int main() {
    for (const Member &m : kMembers) {
        CHECK(m.flag == m.value);
        CHECK((KSCHED_PICK_RANKED & m.flag) && (KSCHED_PICK_DRAWS & m.flag) && (KSCHED_PICK_ANY & m.flag));
        the_mask_kernel_always_runs(m);
        the_mask_kernel_is_the_mask_only_requests(m);
        the_options_of_the_other_picks_do_not_apply(m);
        the_other_picks_plan_no_pick_of_this_member(m);
        for (const Member &o : kMembers)
            if (o.flag != m.flag) the_pipe_waits_for_what_another_members_submit_waits_for(m, o);
    }
    CHECK(KSCHED_PICK_RANKED == 0x1C0u && KSCHED_PICK_DRAWS == 0x1C8u && KSCHED_PICK_ANY == 0x1D8u);
    todays_requests_get_todays_plans();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
