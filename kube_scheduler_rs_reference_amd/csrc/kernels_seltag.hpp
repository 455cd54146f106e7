// kernels_seltag.hpp -- k_eval_seltag: the mask of a TAGGED call (extension E9, include/ksched.h: KSCHED_SELOP_TAGGED).
//
// The contract (sel_tags.hpp: seltag_pass, seltag_row): per pod and key, with e the pod's selector entry, tag = e >> 29, id = e & 0x1FFFFFFF
// and v the node's whole label id: e == 0 passes; EQ: v == id; NE: v != id; EXISTS: v != 0; ABSENT: v == 0; GT: v != 0 && v > id;
// LT: v != 0 && v < id; tags 6 and 7 (KSCHED_SEL_NEVER among them) nowhere -- unsigned compares; the row is the AND over the keys, bits at
// or beyond n zero.
//
// Mapping: k_eval_selop's (kernels_selop.hpp), geometry and arguments included.  One wave owns kSelopCW consecutive 64-node word columns,
// whose label ids live in VGPRs for the whole kernel.  It walks pods 64 at a time; a pod's entries are wave-uniform, so they come in
// through the scalar cache.  The word of pod j is parked in lane j (v_writelane), and after 64 pods every lane stores kSelopCW consecutive
// words of "its" pod row.  A pod's unconstrained keys are skipped by a wave-uniform branch: they cost no VALU work.
//
// The operator varies per (pod, key).  A wave-uniform switch over the tag around every key is what E8's first form did for ONE extra case
// and paid 1.5 times the kernel's time for (profiles/selop_cost.txt), so there is no branch on the tag: the entry is decoded on the scalar
// side into the one form of sel_tags.hpp's seltag_form,
//     word = ballot(v - lo < len) ^ neg        -- v in [lo, lo + len), negated for NE and ABSENT; len == 0 for what passes nowhere
// -- lo, len and neg in scalar integer arithmetic on the tag's three bits, then a v_sub, one v_cmp, an s_xor_b64 and an s_and_b64 per
// constrained (key, column).  A lane at or beyond n holds id 0 and PASSES a negated range (NE, ABSENT): the valid-bits word is applied
// after the xor -- every row starts from it and only ANDs.  The decode is some forty scalar instructions per constrained key, and the
// compute unit's one scalar unit is what the kernel waits for (DESIGN section 4 has the measurement and two forms that were no faster).
//
// Snapshots of more than kSelopKeys keys take one launch per kSelopKeys keys; the launches after the first AND into the mask
// (`accumulate`).  Plain vector stores only; rows and offsets are 64-bit (p * pitch may pass 2^32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ksched.h"
#include "kernarg.hpp"
#include "kernels_direct.hpp"  // ksched_writelane_u32
#include "kernels_selop.hpp"   // SelopArgs: the same arguments
#include "sel_tags.hpp"

namespace ksched {

// (pointers as separate __restrict__ parameters, as in k_eval_direct: the pod entries stay on the scalar unit)
__global__ __launch_bounds__(64 * kSelopWaves) void k_eval_seltag(const uint32_t *__restrict__ g_nlab, const uint32_t *__restrict__ g_psel,
                                                                   uint64_t *__restrict__ out_feas, const SelopArgs a) {
    kernarg_warm<3 * 8 + sizeof(SelopArgs)>();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t w0 = (blockIdx.x * kSelopWaves + wave) * kSelopCW;  // first word column of this wave
    if (w0 >= a.W) return;

    // ---- node columns of this wave -> registers --------------------------------------------------------------------------------------
    uint32_t nlab[kSelopKeys][kSelopCW];
    uint64_t valid[kSelopCW];
#pragma unroll
    for (uint32_t c = 0; c < kSelopCW; ++c) {
        const uint32_t node = (w0 + c) * 64u + lane;
        const bool in = w0 + c < a.W && node < a.n;  // (a column at or beyond W holds no node, whatever the product wrapped to)
        valid[c] = __ballot(in);
#pragma unroll
        for (uint32_t k = 0; k < kSelopKeys; ++k) nlab[k][c] = (in && k < a.nkeys) ? g_nlab[(size_t)(a.key0 + k) * a.n + node] : 0u;
    }

    const uint32_t tile0 = blockIdx.y * a.pod_tiles_per_block;
    for (uint32_t t = 0; t < a.pod_tiles_per_block; ++t) {
        const uint64_t first = (uint64_t)(tile0 + t) * 64u;
        if (first >= a.p) break;
        const uint32_t p0 = (uint32_t)first;
        const uint32_t jmax = min(64u, a.p - p0);

        uint32_t flo[kSelopCW], fhi[kSelopCW];  // the word of pod (p0 + lane)
#pragma unroll
        for (uint32_t c = 0; c < kSelopCW; ++c) flo[c] = fhi[c] = 0u;

        for (uint32_t j = 0; j < jmax; ++j) {
            const uint32_t p = p0 + j;  // wave-uniform -> scalar loads
            uint64_t m[kSelopCW];
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) m[c] = valid[c];
#pragma unroll
            for (uint32_t k = 0; k < kSelopKeys; ++k) {
                const uint32_t e = (k < a.nkeys) ? g_psel[(size_t)(a.key0 + k) * a.p + p] : 0u;
                if (e != 0u) {  // wave-uniform branch: unconstrained keys cost no VALU work
                    // seltag_form(e) from the tag's three bits, in scalar integer arithmetic: no compare, no branch on the tag
                    const uint32_t tag = e >> KSCHED_SELTAG_SHIFT, id = e & KSCHED_SELTAG_ID_MASK;
                    const uint32_t t0 = tag & 1u, t1 = (tag >> 1) & 1u, t2 = tag >> 2;
                    // NE, ABSENT: all ones.  (Opaque for the same reason as `len` below: a 64-bit all-ones-or-zero word that the compiler can
                    // trace back to a condition is a lane mask to it, and the whole chain of words moves onto the vector unit.)
                    const uint32_t neg32 = __builtin_amdgcn_readfirstlane(0u - (t0 & (t2 ^ 1u)));
                    const uint64_t neg = ((uint64_t)neg32 << 32) | neg32;
                    const uint32_t by_id = 0u - ((t1 ^ 1u) & ((t0 & t2) ^ 1u));         // EQ, NE, GT: the range starts at the id
                    const uint32_t lo = (id & by_id) + (t1 | t2);                       // ... (+ 1 for GT); EXISTS, ABSENT, LT: at 1
                    const uint32_t len45 = ((id - (id != 0u ? 1u : 0u)) & (0u - t0)) | (~id & (t0 - 1u));  // LT: [1, id) -- none for id 0 and 1; GT: (id, 2^32)
                    const uint32_t len03 = 1u | (0u - t1);                              // EQ, NE: the id alone; EXISTS, ABSENT: [1, 2^32)
                    // tags 6 and 7: the empty range.  (v_readfirstlane: the value is wave-uniform already; behind it the compiler can no longer
                    // turn the masks back into conditions and fold "tag < 6" into every lane's compare -- three vector instructions per
                    // column where one v_cmp does, what E8's LT paid for its SEL_NEVER select)
                    const uint32_t len = __builtin_amdgcn_readfirstlane(((len45 & (0u - t2)) | (len03 & (t2 - 1u))) & (0u - ((t1 & t2) ^ 1u)));
#pragma unroll
                    for (uint32_t c = 0; c < kSelopCW; ++c) m[c] &= __ballot(nlab[k][c] - lo < len) ^ neg;  // (m starts as the valid-bits word: applied after the xor)
                }
            }
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) {
                flo[c] = ksched_writelane_u32((uint32_t)m[c], j, flo[c]);
                fhi[c] = ksched_writelane_u32((uint32_t)(m[c] >> 32), j, fhi[c]);
            }
        }

        // ---- lane l stores kSelopCW consecutive words of pod row p0 + l -------------------------------------------------------------
        if (lane < jmax) {
            const size_t row = (size_t)(p0 + lane) * a.pitch;
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) {
                if (w0 + c < a.W) {
                    const uint64_t f = ((uint64_t)fhi[c] << 32) | flo[c];
                    if (a.accumulate) out_feas[row + w0 + c] &= f;
                    else out_feas[row + w0 + c] = f;
                }
            }
        }
    }
}

// The mask of a tagged call over [p] rows of W = ceil(n / 64) words, `pitch` words apart, enqueued on `s`: nlab = the snapshot's label
// columns [nkeys][n], psel = the batch's tagged selector entries [nkeys][p] (nullptr, or nkeys == 0: no pod constrains anything -- the
// all-valid rows).  The geometry is sel_tags.hpp's; the one launch path (ksched_api.hip's launch_mask).
inline hipError_t run_seltag(const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, uint32_t p, uint32_t n, uint32_t W, uint32_t pitch, uint32_t nkeys,
                             hipStream_t s) {
    if (p == 0 || W == 0) return hipSuccess;
    if (!out_feas || pitch < W) return hipErrorInvalidValue;
    if (!psel || !nlab) nkeys = 0;
    const SeltagLaunch l = plan_seltag_launch(p, W, nkeys);
    SelopArgs a{};
    a.n = n;
    a.p = p;
    a.W = W;
    a.pitch = pitch;
    a.pod_tiles_per_block = l.pod_tiles_per_block;
    for (uint32_t pass = 0; pass < l.passes; ++pass) {
        a.key0 = selop_pass_key0(pass);
        a.nkeys = selop_pass_keys(nkeys, pass);
        a.accumulate = pass > 0 ? 1u : 0u;
        hipLaunchKernelGGL(k_eval_seltag, dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a);
    }
    return hipGetLastError();
}

}  // namespace ksched
