// kernels_selop.hpp -- k_eval_selop: the mask of an OPERATOR call (extension E8, include/ksched.h: KSCHED_SELOP_EXISTS / _GT / _LT).
//
// The contract (sel_ops.hpp: selop_pass, selop_row): per pod and key, with e the pod's selector entry and v the node's label id,
// e == 0 passes, e == KSCHED_SEL_NEVER never passes, otherwise EXISTS: v != 0, GT: v != 0 && v > e, LT: v != 0 && v < e -- unsigned
// compares of the ids; the row is the AND over the keys, bits at or beyond n zero.
//
// The mapping, the walk over the pods and the launch are kernels_sel_walk.hpp's.  This kernel's own, per operator:
//  * GT   one v_cmp per constrained (key, column): v > e with e >= 1 already says v != 0.
//  * LT   one v_cmp too: the registers hold v - 1 (an absent node: 0xFFFFFFFF), and v - 1 < e - 1 is v != 0 && v < e for every e >= 1.
//  * EXISTS  the word ballot(v != 0) of a (key, column) does not depend on the pod: it is taken ONCE, before the pod loop, into wave-uniform
//         values (the label ids' registers are then free), and the pod loop is scalar ANDs of those words.
// KSCHED_SEL_NEVER gives an all-zero row under every operator WITHOUT a branch of its own: no id is above 0xFFFFFFFF, so GT's compare
// already fails; LT compares against the bound 0 instead of e - 1; EXISTS ANDs with zero -- one scalar select each (kernels_sel_walk.hpp
// and profiles/selop_cost.txt say what the branch cost).  A lane at or beyond n holds id 0 and fails every compare.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ksched.h"
#include "kernarg.hpp"
#include "kernels_sel_walk.hpp"
#include "sel_ops.hpp"

namespace ksched {

// (pointers as separate __restrict__ parameters, as in k_eval_direct: the pod entries stay on the scalar unit)
template <SelOp OP>
__global__ __launch_bounds__(64 * kSelopWaves) void k_eval_selop(const uint32_t *__restrict__ g_nlab, const uint32_t *__restrict__ g_psel,
                                                                  uint64_t *__restrict__ out_feas, const SelopArgs a) {
    static_assert(OP == SelOp::kExists || OP == SelOp::kGt || OP == SelOp::kLt, "an operator kernel");
    kernarg_warm<3 * 8 + sizeof(SelopArgs)>();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t w0 = (blockIdx.x * kSelopWaves + wave) * kSelopCW;  // first word column of this wave
    if (w0 >= a.W) return;

    // ---- node columns of this wave -> registers (EXISTS: -> wave-uniform presence words) -----------------------------------------
    uint32_t nlab[kSelopKeys][kSelopCW];    // GT: v; LT: v - 1
    uint64_t has[kSelopKeys][kSelopCW];     // EXISTS: ballot(v != 0)
    uint64_t valid[kSelopCW];
#pragma unroll
    for (uint32_t c = 0; c < kSelopCW; ++c) {
        const uint32_t node = (w0 + c) * 64u + lane;
        const bool in = w0 + c < a.W && node < a.n;  // (a column at or beyond W holds no node, whatever the product wrapped to)
        valid[c] = __ballot(in);
#pragma unroll
        for (uint32_t k = 0; k < kSelopKeys; ++k) {
            const uint32_t v = (in && k < a.nkeys) ? g_nlab[(size_t)(a.key0 + k) * a.n + node] : 0u;
            if (OP == SelOp::kExists) has[k][c] = __ballot(v != 0u);
            else nlab[k][c] = OP == SelOp::kLt ? v - 1u : v;
        }
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
                    // KSCHED_SEL_NEVER without a branch of its own (one scalar select): no id is above 0xFFFFFFFF, so GT needs nothing; LT
                    // compares against the bound 0, which no v - 1 is below; EXISTS ANDs with zero
                    const uint32_t below = e == KSCHED_SEL_NEVER ? 0u : e - 1u;
                    const uint64_t keep = e == KSCHED_SEL_NEVER ? 0ull : ~0ull;
#pragma unroll
                    for (uint32_t c = 0; c < kSelopCW; ++c) {
                        if (OP == SelOp::kExists) m[c] &= has[k][c] & keep;
                        else if (OP == SelOp::kGt) m[c] &= __ballot(nlab[k][c] > e);
                        else m[c] &= __ballot(nlab[k][c] < below);
                    }
                }
            }
            sel_park(m, j, flo, fhi);
        }
        sel_store_rows(out_feas, a.pitch, a.W, w0, p0, lane, jmax, flo, fhi, a.accumulate);
    }
}

inline bool launch_selop(SelOp op, const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, const SelopLaunch &l, const SelopArgs &a, hipStream_t s) {
    switch (op) {
        case SelOp::kExists: hipLaunchKernelGGL((k_eval_selop<SelOp::kExists>), dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a); return true;
        case SelOp::kGt: hipLaunchKernelGGL((k_eval_selop<SelOp::kGt>), dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a); return true;
        case SelOp::kLt: hipLaunchKernelGGL((k_eval_selop<SelOp::kLt>), dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a); return true;
        default: return false;
    }
}

}  // namespace ksched
