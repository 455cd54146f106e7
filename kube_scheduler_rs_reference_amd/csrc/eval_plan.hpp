// eval_plan.hpp -- which kernels one evaluation request runs: a pure function of a few scalars.
//
// Host-only on purpose: no HIP include, no ksched_ctx, no kernel header, so that plain g++ compiles it and
// tests/cpp/plan_tests.cpp pins every rule at its boundary without a GPU.  eval_on_device (ksched_api.hip) gathers the
// EvalFacts, calls plan_eval and hands the EvalPlan to its launchers; nothing else decides which path a request takes.
// The measured thresholds of the dispatch live here, with their measurements.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/ksched.h"
#include "bestfit_layout.hpp"
#include "mask_combine.hpp"
#include "sel_ops.hpp"
#include "sel_tags.hpp"
#include "sel_terms.hpp"

namespace ksched {

// Does the pick read the feasibility mask?  By default it does not (sampled: the drawn candidates are tested from the columns;
// best fit: bitmaps kept in best-fit order); it does with KSCHED_OPT_PICK_FROM_MASK, and a best-fit pick does when the snapshot
// has no best-fit rows (`bf_rows`: they exist, or will once ensure_bestfit has run).  The ranked picks (KSCHED_PICK_RANKED) always do:
// the uniform pick counts and ranks the row's set bits; the spread and the pack pick do so once per draw.
inline bool pick_reads_mask(uint32_t flags, bool opt_pick_from_mask, bool bf_rows) {
    if (flags & KSCHED_PICK_RANKED) return true;
    return (flags & (KSCHED_PICK_SAMPLED | KSCHED_PICK_BESTFIT)) && (opt_pick_from_mask || ((flags & KSCHED_PICK_BESTFIT) && !bf_rows));
}

// fused (one launch over the bitmap index) where it applies, else the always-applicable direct kernel; KSCHED_OPT_KERNEL can force
// one (a forced fused kernel that does not apply is the caller's KSCHED_E_UNSUPPORTED).  Evaluations and summaries alike, each with
// its own applicability test.
inline int choose_kernel(int opt_kernel, bool can_fused) {
    if (opt_kernel != KSCHED_KERNEL_AUTO) return opt_kernel;
    return can_fused ? KSCHED_KERNEL_FUSED : KSCHED_KERNEL_DIRECT;
}

struct EvalFacts {
    uint32_t p = 0, n = 0, attempts = 0, flags = 0;  // the request (p > 0) over a snapshot of n > 0 nodes with `nkeys` label keys
    uint32_t nkeys = 0;
    bool have_feas = false, have_fit = false, have_psel = false;  // which outputs the caller gave, and whether it gave selectors
    uint32_t tiles = 0, nlist = 0;  // the bitmap index's layout: tiles, list keys (read only where the index is known to exist)
    // kernels_fused.hpp's answers (they need the LDS carve-up, tile_launch.hpp): fused_applicable, fused_pick_applicable, fused_tile_pick_applicable
    bool fused_applicable = false, fused_pick_applicable = false, fused_tile_pick_applicable = false;
    bool bf_rows_built = false;
    uint32_t fused_waves = 0;  // kFusedWaves
    int opt_kernel = KSCHED_KERNEL_AUTO, opt_fused_pick = 1, opt_bestfit_stages = 0;
    bool opt_pick_from_mask = false;
    uint32_t opt_grid_cus = 0;
    uint32_t debug = 0;  // KSCHED_OPT_DEBUG (bit 0x400: best fit in one stage)
    CombineOp combine = CombineOp::kNone;  // combine_op(flags) of a combining call (extension E6, mask_combine.hpp); the caller gave out_feasible and no out_fit
    bool soft = false;  // combine_soft(flags) (extension E7, mask_combine_soft.hpp): with kAnd or kAndNot only
    SelOp selop = SelOp::kNone;  // sel_op(flags) of an operator call (extension E8, sel_ops.hpp): KSCHED_SEL alone beside it, no out_fit
    bool seltag = false;  // sel_tagged(flags) of a tagged call (extension E9, sel_tags.hpp): KSCHED_SEL alone beside it, no operator flag, no out_fit
    uint32_t terms = 0;  // sel_terms(flags) (extension E10, sel_terms.hpp): not 0 only in a tagged call -- the pod's row is the OR of that many tagged rows
};

enum class MaskKernel { kNone, kFused, kDirect, kSelOp, kSelTag, kSelTerms };
enum class SampledPick { kNone, kOwnLaunch, kRidesFill, kRidesTiles, kFromMask };
enum class BestfitPick { kNone, kRowsOneStage, kRowsTwoStages, kRowsTwoStagesListed, kFromMask };
enum class RankedPick { kNone, kUniform, kSpread, kPack };  // k_pick_uniform / k_pick_spread / k_pick_pack behind the mask kernel: the only form
enum class PlanError { kNone, kFusedNotApplicable, kTilePickNotApplicable, kListKeysTooManyNodes };

struct EvalPlan {
    int error = KSCHED_OK;  // KSCHED_E_UNSUPPORTED: nothing is enqueued, `why` names the message
    PlanError why = PlanError::kNone;
    MaskKernel mask = MaskKernel::kNone;
    bool scratch_mask = false;  // the mask kernel writes the feasible mask into the ctx's scratch one (the caller gave none, or the call combines into the caller's)
    SampledPick sampled = SampledPick::kNone;
    BestfitPick bestfit = BestfitPick::kNone;
    RankedPick ranked = RankedPick::kNone;
    CombineOp combine = CombineOp::kNone;  // not kNone: k_mask_combine folds the scratch mask into the caller's mask, between the mask kernel and the pick
    const char *last_kernel = nullptr;  // ksched_last_kernel after the launch; nullptr = no mask kernel runs, it stays what it was
    const char *last_pick = "none";     // ksched_last_pick
    bool soft = false;  // with a combine: k_mask_combine_soft in k_mask_combine's place -- a row the fold would empty keeps what it held
    SelOp selop = SelOp::kNone;  // with mask == kSelOp: the operator k_eval_selop answers
    bool seltag = false;  // mask == kSelTag: k_eval_seltag reads the operator out of every selector entry
    uint32_t terms = 0;  // mask == kSelTerms: k_eval_selterms ORs that many tagged rows per pod (not 0, T = 1 included; `seltag` is set too)

    bool pick_rides() const { return sampled == SampledPick::kRidesFill || sampled == SampledPick::kRidesTiles; }
    bool bestfit_rows() const { return bestfit != BestfitPick::kNone && bestfit != BestfitPick::kFromMask; }
    // a pick launch follows the mask kernel and reads what it wrote
    bool pick_from_mask() const { return sampled == SampledPick::kFromMask || bestfit == BestfitPick::kFromMask || ranked != RankedPick::kNone; }
};

inline EvalPlan plan_unsupported(PlanError why) {
    EvalPlan e;
    e.error = KSCHED_E_UNSUPPORTED;
    e.why = why;
    return e;
}

// The ranked picks, member by member: the flag, the plan's name for it and ksched_last_pick.  (A call carries one pick flag; the
// first row whose flag is set answers.)
struct RankedMember {
    uint32_t flag;
    RankedPick pick;
    const char *name;
};
constexpr RankedMember kRankedMembers[] = {{KSCHED_PICK_SPREAD, RankedPick::kSpread, "spread"},
                                           {KSCHED_PICK_PACK, RankedPick::kPack, "pack"},
                                           {KSCHED_PICK_UNIFORM, RankedPick::kUniform, "uniform"}};
inline const RankedMember *ranked_member(uint32_t flags) {
    for (const RankedMember &m : kRankedMembers)
        if (flags & m.flag) return &m;
    return nullptr;
}

inline EvalPlan plan_eval(const EvalFacts &f) {
    EvalPlan plan;
    const uint32_t p = f.p, flags = f.flags;
    const bool pick_s = flags & KSCHED_PICK_SAMPLED, pick_b = flags & KSCHED_PICK_BESTFIT;
    // kernel choice: fused (one launch over the bitmap index) when the snapshot has an index that fits LDS, else the
    // always-applicable direct kernel; KSCHED_OPT_KERNEL can force one.
    const bool want_mask = f.have_feas || f.have_fit;
    const bool can_fused = f.fused_applicable;
    const int kern = choose_kernel(f.opt_kernel, can_fused);
    // An operator call (extension E8) answers the selector term alone, by the operator kernel: the only form, whatever KSCHED_OPT_KERNEL
    // says and whether or not the snapshot has a bitmap index -- so no plan of it is unsupported.  Nothing rides in that kernel and no pick
    // has structures for the operators: a pick runs behind the mask (behind the combine, if the call combines) and reads it, as in a
    // combining call, whatever KSCHED_OPT_PICK_FROM_MASK / KSCHED_OPT_FUSED_PICK say.  The mask goes into the ctx's scratch mask when the
    // call combines (the caller's is the combine's left operand) or the caller gave none.
    // A tagged call (extension E9) is planned the same way, with the tagged kernel in the operator kernel's place; it carries no operator
    // (check_seltag_args), so an operator decides first only where a caller of plan_eval gives both.
    // A term count (extension E10) modifies a tagged call and nothing else (check_selterms_args): the terms kernel takes the tagged
    // kernel's place whenever the count is not 0, one term included; everything around it is the tagged call's plan.
    if (f.selop != SelOp::kNone || f.seltag) {
        if (f.selop != SelOp::kNone) {
            plan.selop = f.selop;
            plan.mask = MaskKernel::kSelOp;
            plan.last_kernel = "selop";
        } else {
            plan.seltag = true;
            plan.terms = f.terms;
            plan.mask = f.terms ? MaskKernel::kSelTerms : MaskKernel::kSelTag;
            plan.last_kernel = f.terms ? "selterms" : "seltag";
        }
        plan.combine = f.combine;
        plan.soft = f.combine != CombineOp::kNone && f.soft;
        plan.scratch_mask = f.combine != CombineOp::kNone || !f.have_feas;
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
    // A combining call (extension E6) is a mask-only evaluation into the ctx's scratch mask -- although the caller gave a mask: that one
    // is the combine's left operand --, then the combine, then the pick from the COMBINED mask.  So the mask kernel is chosen as for a
    // mask-only request, nothing rides in it (a riding pick would test the call's own predicates, not the combined mask), and the sampled
    // and the best-fit pick read the mask, whatever KSCHED_OPT_PICK_FROM_MASK / KSCHED_OPT_FUSED_PICK say; the ranked picks always did.
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
    // The ranked picks (KSCHED_PICK_RANKED) count and rank the set bits of the pod's whole row -- the uniform pick once, the spread and the
    // pack pick once per draw, comparing the candidates: the mask kernel always runs (into the ctx's scratch mask when the caller gave
    // none), the pick is its own launch behind it, and neither KSCHED_OPT_PICK_FROM_MASK nor KSCHED_OPT_FUSED_PICK applies.  One plan for
    // the family; a member has its own kernel and its own name.
    if (const RankedMember *m = ranked_member(flags)) {
        if (kern == KSCHED_KERNEL_FUSED && !can_fused) return plan_unsupported(PlanError::kFusedNotApplicable);
        plan.scratch_mask = !f.have_feas;
        plan.mask = kern == KSCHED_KERNEL_FUSED ? MaskKernel::kFused : MaskKernel::kDirect;
        plan.last_kernel = kern == KSCHED_KERNEL_FUSED ? "fused" : "direct";
        plan.ranked = m->pick;
        plan.last_pick = m->name;
        return plan;
    }
    // The sampled pick tests only the drawn candidates, from the node records: it does not need the mask.  When a mask is
    // asked for too and the fused kernel runs, the pick RIDES in that launch (KSCHED_OPT_FUSED_PICK, kernels_fused.hpp "PICK":
    // a step is one kernel); otherwise it is its own launch, first (nothing waits on a mask kernel), and a bindings-only
    // request launches no mask kernel at all.  KSCHED_OPT_PICK_FROM_MASK restores the mask-reading pick (a cross-check).
    const bool select_direct = pick_s && !f.opt_pick_from_mask;
    // Does a riding pick pay?  Two forms (kernels_fused.hpp PICK): TILE TESTS -- every tile-block of a pod range tests the draws that fall into
    // its tile from the rows it holds -- and WAVES OF THE FILL, which run select_one_pod while the tile is staged.
    //  * Waves of the fill only hide in the fill: they ride when a wave has at most five rounds (C3: 2, the C4 shard: 5; beyond that they cost
    //    twice the stand-alone kernel, round 3's measurement, re-measured in round 6: 400 k x 5 k 67.1 us riding against 66.1).
    //  * Tile tests re-read a pod's operands and draws once per tile; the tile-blocks of a pod range sit on one XCD, so tiles - 1 of those reads
    //    come from that XCD's L2 -- as long as the XCD's share of the batch's operands and draws (68 B per pod / 8 XCDs) stays in its 4 MiB.
    //    Round 6 (session r7a, interleaved round order, step us riding / own launch): 100 k x 5 k  17.6 / 22.6;  400 k x 5 k  53.4 / 65.9;
    //    250 k x 10 k  64.8 / 75.0;  500 k x 10 k  123.3 / 142.8;  but 800 k x 5 k  143.4 / 125.3, 1 M x 10 k  322.0 / 288.6, 1.6 M x 5 k  281.8 / 241.6.
    //    (Rounds 3 - 5 had the tile tests stop riding at five rounds per wave too: with every wave on its own contiguous pod range the blocks of
    //    a pod range drifted apart much earlier.)  They ride up to 524 288 pods per call.
    // The form: tile tests in phase 1 (no node records fetched, no wave taken off the staging) where the request allows it, else
    // waves of the fill running select_one_pod.
    // Which form when both apply: the tile tests cost every (pod, tile) pair five draw loads and a handful of LDS reads, the waves
    // of the fill cost every block a longer fill.  Measured (session r3g3, rotated outputs, step): 5 tiles (C3) 19.8 us against 21.6;
    // 10 tiles (the C4 shard) 45.3 us against 42.1; 1 tile (C2) 7.1 us against 6.8.  With one device-scope atomic per unit of eight pods and
    // the draws loaded coalesced (later in round 3) the C4 shard reads 40.9 - 41.5 us against 42.1 - 42.3, C2 6.8 against 6.4: 2 .. 12 tiles.
    // KSCHED_OPT_FUSED_PICK = 3 asks for the tile tests whatever the request: where they do not apply, a pick that would ride is unsupported.
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
    // The best-fit pick likewise: from bitmaps kept in best-fit order (k_pick_bestfit_rows), no mask involved.
    if (pick_b && !f.opt_pick_from_mask && f.bf_rows_built) {
        const bool sel = (flags & KSCHED_SEL) && f.have_psel && f.nkeys > 0;
        // one stage (a wave per pod) or two (a lane per pod first): the second launch and the hand-over list pay off from tens of
        // thousands of pods on (20k pods: 33 us against 44; 125k pods: 160 against 120) -- KSCHED_OPT_BESTFIT_STAGES overrides
        // pods that constrain a list key are split off by the first stage: two stages it is.  (Only with the selector term active: the
        // listed kernel is then given the selector columns and key count every other pick of the request is given, launch_bestfit_listed.)
        const bool lists = sel && f.nlist > 0;
        const bool two_stage = lists || f.opt_bestfit_stages == 2 || (f.opt_bestfit_stages == 0 && p >= 24576u);  // (measured crossover at the C5 shard's snapshot: ~24 k pods)
        if (!lists && (!two_stage || (f.debug & 0x400u) || f.n > kBfLanesMaxNodes)) {  // (the first stage's searches carry kBfMaxLevels level arrays)
            plan.bestfit = BestfitPick::kRowsOneStage;
        } else {
            if (f.n > kBfLanesMaxNodes) return plan_unsupported(PlanError::kListKeysTooManyNodes);
            plan.bestfit = lists ? BestfitPick::kRowsTwoStagesListed : BestfitPick::kRowsTwoStages;
        }
        plan.last_pick = "bestfit-rows";
        if (!want_mask) return plan;
    }
    // the mask kernels always write the feasible mask: a pick that reads it, or a fit-mask-only request, gets a scratch one
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

}  // namespace ksched
