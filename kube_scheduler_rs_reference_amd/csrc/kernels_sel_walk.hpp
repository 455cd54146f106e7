// kernels_sel_walk.hpp -- what the selector kernels share: the walk over the pods, the decode of a tagged entry, and the one launch path of
// the three selector calls (extensions E8 sel_ops.hpp / kernels_selop.hpp, E9 sel_tags.hpp / kernels_seltag.hpp, E10 sel_terms.hpp /
// kernels_selterms.hpp).  Each kernel file keeps what is its own: the per-operator compare, the term OR and its early exit, the wide kernel's
// pass walk.
//
// The mapping.  k_eval_direct's (kernels_direct.hpp), with the selector term alone.  One wave owns kSelopCW consecutive 64-node word columns,
// whose label ids live in VGPRs (selop, seltag, selterms: for the whole kernel; selterms_wide: for one key pass).  It walks pods 64 at a
// time; a pod's entries are wave-uniform, so they come in through the scalar cache, and each v_cmp against them yields the 64-node result
// word directly in an SGPR pair.  The word of pod j is parked in lane j (v_writelane: sel_park), and after 64 pods every lane stores
// kSelopCW consecutive words of "its" pod row (sel_store_rows).  A pod's unconstrained keys are skipped by a wave-uniform branch: they cost
// no VALU work.  A lane at or beyond n holds id 0; an unconstrained row starts from the valid-bits words.  Plain vector stores only; rows
// and offsets are 64-bit (p * pitch may pass 2^32).
//
// The decode (sel_and_entry).  In a tagged call the operator varies per (pod, key).  A wave-uniform switch over the tag around every key is
// what E8's first form did for ONE extra case -- written as a second wave-uniform branch inside the first, the compiler built a three-way
// switch of a dozen scalar instructions and four branches around EVERY key of every pod, constrained or not -- and paid 1.5 times the
// kernel's time for (profiles/selop_cost.txt), so there is no branch on the tag: the entry is decoded on the scalar side into the one form of
// sel_tags.hpp's seltag_form,
//     word = ballot(v - lo < len) ^ neg        -- v in [lo, lo + len), negated for NE and ABSENT; len == 0 for what passes nowhere
// -- lo, len and neg in scalar integer arithmetic on the tag's three bits, then a v_sub, one v_cmp, an s_xor_b64 and an s_and_b64 per
// constrained (key, column).  A lane at or beyond n holds id 0 and PASSES a negated range (NE, ABSENT): the valid-bits word is applied
// after the xor -- every row starts from it and only ANDs.  The decode is some forty scalar instructions per constrained key, and the
// compute unit's one scalar unit is what the kernels wait for (DESIGN section 4 has the measurement and two forms that were no faster).
// sel_tags.hpp's seltag_form_bits restates the arithmetic on the host, where tests/cpp/seltag_plan_tests.cpp pins it against seltag_pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ksched.h"
#include "eval_plan.hpp"       // MaskKernel
#include "kernels_direct.hpp"  // (the writelane behind sel_park)
#include "sel_terms.hpp"       // (and through it sel_ops.hpp, sel_tags.hpp)

namespace ksched {

// m[c] &= [entry e against the label ids v[c]] for a constrained entry (e != 0): seltag_form(e) from the tag's three bits, in scalar integer
// arithmetic -- no compare, no branch on the tag --, then a v_sub and one v_cmp per column.  Two compiler traps, one v_readfirstlane each
// (the values are wave-uniform already):
//  * neg.  A 64-bit all-ones-or-zero word that the compiler can trace back to a condition is a lane mask to it, and the whole chain of
//    words moves onto the vector unit.
//  * len.  Behind the v_readfirstlane the compiler can no longer turn the masks back into conditions and fold "tag < 6" into every lane's
//    compare -- three vector instructions per column where one v_cmp does, what E8's LT paid for its SEL_NEVER select.
__device__ __forceinline__ void sel_and_entry(uint32_t e, const uint32_t (&v)[kSelopCW], uint64_t (&m)[kSelopCW]) {
    const uint32_t tag = e >> KSCHED_SELTAG_SHIFT, id = e & KSCHED_SELTAG_ID_MASK;
    const uint32_t t0 = tag & 1u, t1 = (tag >> 1) & 1u, t2 = tag >> 2;
    const uint32_t neg32 = __builtin_amdgcn_readfirstlane(0u - (t0 & (t2 ^ 1u)));  // NE, ABSENT: all ones
    const uint64_t neg = ((uint64_t)neg32 << 32) | neg32;
    const uint32_t by_id = 0u - ((t1 ^ 1u) & ((t0 & t2) ^ 1u));  // EQ, NE, GT: the range starts at the id
    const uint32_t lo = (id & by_id) + (t1 | t2);                // ... (+ 1 for GT); EXISTS, ABSENT, LT: at 1
    const uint32_t len45 = ((id - (id != 0u ? 1u : 0u)) & (0u - t0)) | (~id & (t0 - 1u));  // LT: [1, id) -- none for id 0 and 1; GT: (id, 2^32)
    const uint32_t len03 = 1u | (0u - t1);                                                 // EQ, NE: the id alone; EXISTS, ABSENT: [1, 2^32)
    const uint32_t len = __builtin_amdgcn_readfirstlane(((len45 & (0u - t2)) | (len03 & (t2 - 1u))) & (0u - ((t1 & t2) ^ 1u)));  // tags 6, 7: empty
#pragma unroll
    for (uint32_t c = 0; c < kSelopCW; ++c) m[c] &= __ballot(v[c] - lo < len) ^ neg;  // (m starts as the valid-bits word: applied after the xor)
}

// park the words m of pod j (wave-uniform) in lane j of lo / hi
__device__ __forceinline__ void sel_park(const uint64_t (&m)[kSelopCW], uint32_t j, uint32_t (&lo)[kSelopCW], uint32_t (&hi)[kSelopCW]) {
#pragma unroll
    for (uint32_t c = 0; c < kSelopCW; ++c) {
        lo[c] = ksched_writelane_u32((uint32_t)m[c], j, lo[c]);
        hi[c] = ksched_writelane_u32((uint32_t)(m[c] >> 32), j, hi[c]);
    }
}

// lane l < jmax stores the words [w0, w0 + kSelopCW) below W of pod row p0 + l, rows `pitch` words apart; `accumulate`: ANDs them in
__device__ __forceinline__ void sel_store_rows(uint64_t *__restrict__ out_feas, uint32_t pitch, uint32_t W, uint32_t w0, uint32_t p0, uint32_t lane, uint32_t jmax,
                                               const uint32_t (&lo)[kSelopCW], const uint32_t (&hi)[kSelopCW], uint32_t accumulate) {
    if (lane < jmax) {
        const size_t row = (size_t)(p0 + lane) * pitch;
#pragma unroll
        for (uint32_t c = 0; c < kSelopCW; ++c) {
            if (w0 + c < W) {
                const uint64_t f = ((uint64_t)hi[c] << 32) | lo[c];
                if (accumulate) out_feas[row + w0 + c] &= f;
                else out_feas[row + w0 + c] = f;
            }
        }
    }
}

// ---- the launch -----------------------------------------------------------------------------------------------------------------
// the arguments of k_eval_selop<OP> and k_eval_seltag
struct SelopArgs {
    uint32_t n, p, W;
    uint32_t pitch;                // words between consecutive pod rows of the mask (>= W)
    uint32_t key0, nkeys;          // this pass handles keys [key0, key0 + nkeys), nkeys <= kSelopKeys (0: no key at all)
    uint32_t pod_tiles_per_block;  // 64-pod tiles walked by one block
    uint32_t accumulate;           // AND into out_feas instead of overwriting (key passes after the first)
};

// the arguments of k_eval_selterms and k_eval_selterms_wide
struct SeltermsArgs {
    uint32_t n, p, W;
    uint32_t pitch;                // words between consecutive pod rows of the mask (>= W)
    uint32_t nkeys;                // all of the snapshot's keys (0: no key at all); k_eval_selterms: <= kSelopKeys
    uint32_t terms;                // T >= 1
    uint32_t pod_tiles_per_block;  // 64-pod tiles walked by one block
    uint32_t key_passes;           // k_eval_selterms_wide: ceil(nkeys / kSelopKeys)
};

// one launch of a call's kernel with finished arguments: each kernel file defines its own (launch_selop: false for no operator)
inline bool launch_selop(SelOp op, const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, const SelopLaunch &l, const SelopArgs &a, hipStream_t s);
inline void launch_seltag(const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, const SeltagLaunch &l, const SelopArgs &a, hipStream_t s);
inline void launch_selterms(const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, const SeltermsLaunch &l, const SeltermsArgs &a, hipStream_t s);

// what every selector kernel's walk reads, into zeroed arguments
template <class Args>
inline Args sel_walk_args(uint32_t n, uint32_t p, uint32_t W, uint32_t pitch, uint32_t pod_tiles_per_block) {
    Args a{};
    a.n = n;
    a.p = p;
    a.W = W;
    a.pitch = pitch;
    a.pod_tiles_per_block = pod_tiles_per_block;
    return a;
}

// The mask of a selector call -- kind: kSelOp under `op`, kSelTag, or kSelTerms with `terms` >= 1 terms -- over [p] rows of W = ceil(n / 64)
// words, `pitch` words apart, enqueued on `s`: nlab = the snapshot's label columns [nkeys][n], psel = the batch's selector entries [nkeys][p]
// (kSelTerms: [terms][nkeys][p]; nullptr, or nkeys == 0: no pod constrains anything -- the all-valid rows).  The geometry is sel_ops.hpp's,
// sel_tags.hpp's or sel_terms.hpp's.  kSelOp and kSelTag take one launch per kSelopKeys keys, the launches after the first ANDing into the
// mask (`accumulate`, as run_direct's do); kSelTerms takes ONE launch (kernels_selterms.hpp says why).  The one launch path (ksched_api.hip's
// launch_mask).
inline hipError_t run_selector_mask(MaskKernel kind, SelOp op, uint32_t terms, const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, uint32_t p, uint32_t n,
                                    uint32_t W, uint32_t pitch, uint32_t nkeys, hipStream_t s) {
    if (p == 0 || W == 0) return hipSuccess;
    if (!out_feas || pitch < W) return hipErrorInvalidValue;
    if (!psel || !nlab) nkeys = 0;
    if (kind == MaskKernel::kSelTerms) {
        if (terms == 0 || terms > KSCHED_MAX_TERMS) return hipErrorInvalidValue;
        const SeltermsLaunch l = plan_selterms_launch(p, W, nkeys, terms);
        SeltermsArgs a = sel_walk_args<SeltermsArgs>(n, p, W, pitch, l.pod_tiles_per_block);
        a.nkeys = nkeys;
        a.terms = l.terms;
        a.key_passes = l.key_passes;
        launch_selterms(nlab, psel, out_feas, l, a, s);
        return hipGetLastError();
    }
    if (kind != MaskKernel::kSelOp && kind != MaskKernel::kSelTag) return hipErrorInvalidValue;
    const SelopLaunch l = kind == MaskKernel::kSelTag ? plan_seltag_launch(p, W, nkeys) : plan_selop_launch(p, W, nkeys);
    SelopArgs a = sel_walk_args<SelopArgs>(n, p, W, pitch, l.pod_tiles_per_block);
    for (uint32_t pass = 0; pass < l.passes; ++pass) {
        a.key0 = selop_pass_key0(pass);
        a.nkeys = selop_pass_keys(nkeys, pass);
        a.accumulate = pass > 0 ? 1u : 0u;
        if (kind == MaskKernel::kSelTag) launch_seltag(nlab, psel, out_feas, l, a, s);
        else if (!launch_selop(op, nlab, psel, out_feas, l, a, s)) return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ksched
