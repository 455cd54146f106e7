// kernels_selop.hpp -- k_eval_selop: the mask of an OPERATOR call (extension E8, include/ksched.h: KSCHED_SELOP_EXISTS / _GT / _LT).
//
// The contract (sel_ops.hpp: selop_pass, selop_row): per pod and key, with e the pod's selector entry and v the node's label id,
// e == 0 passes, e == KSCHED_SEL_NEVER never passes, otherwise EXISTS: v != 0, GT: v != 0 && v > e, LT: v != 0 && v < e -- unsigned
// compares of the ids; the row is the AND over the keys, bits at or beyond n zero.
//
// Mapping: k_eval_direct's (kernels_direct.hpp), with the selector term alone.  One wave owns kSelopCW consecutive 64-node word columns,
// whose label ids live in VGPRs for the whole kernel.  It walks pods 64 at a time; a pod's entries are wave-uniform, so they come in
// through the scalar cache, and each v_cmp against them yields the 64-node result word directly in an SGPR pair.  The word of pod j is
// parked in lane j (v_writelane), and after 64 pods every lane stores kSelopCW consecutive words of "its" pod row.  A pod's unconstrained
// keys are skipped by a wave-uniform branch: they cost no VALU work.
//
// Per operator:
//  * GT   one v_cmp per constrained (key, column): v > e with e >= 1 already says v != 0.
//  * LT   one v_cmp too: the registers hold v - 1 (an absent node: 0xFFFFFFFF), and v - 1 < e - 1 is v != 0 && v < e for every e >= 1.
//  * EXISTS  the word ballot(v != 0) of a (key, column) does not depend on the pod: it is taken ONCE, before the pod loop, into wave-uniform
//         values (the label ids' registers are then free), and the pod loop is scalar ANDs of those words.
// KSCHED_SEL_NEVER gives an all-zero row under every operator WITHOUT a branch of its own: no id is above 0xFFFFFFFF, so GT's compare
// already fails; LT compares against the bound 0 instead of e - 1; EXISTS ANDs with zero -- one scalar select each.  (Written as a second
// wave-uniform branch inside the first, the compiler built a three-way switch of a dozen scalar instructions and four branches around EVERY
// key of every pod, constrained or not, and the kernel ran at 1.5 times the direct kernel's time: profiles/selop_cost.txt.)  A lane at or
// beyond n holds id 0 and fails every compare; an unconstrained row starts from the valid-bits words.
//
// Snapshots of more than kSelopKeys keys take one launch per kSelopKeys keys; the launches after the first AND into the mask
// (`accumulate`), as run_direct's do.  Plain vector stores only; rows and offsets are 64-bit (p * pitch may pass 2^32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ksched.h"
#include "kernarg.hpp"
#include "kernels_direct.hpp"  // ksched_writelane_u32
#include "sel_ops.hpp"

namespace ksched {

struct SelopArgs {
    uint32_t n, p, W;
    uint32_t pitch;                // words between consecutive pod rows of the mask (>= W)
    uint32_t key0, nkeys;          // this pass handles keys [key0, key0 + nkeys), nkeys <= kSelopKeys (0: no key at all)
    uint32_t pod_tiles_per_block;  // 64-pod tiles walked by one block
    uint32_t accumulate;           // AND into out_feas instead of overwriting (key passes after the first)
};

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

template <SelOp OP>
inline void launch_selop(const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, const SelopLaunch &l, SelopArgs a, uint32_t nkeys, hipStream_t s) {
    for (uint32_t pass = 0; pass < l.passes; ++pass) {
        a.key0 = selop_pass_key0(pass);
        a.nkeys = selop_pass_keys(nkeys, pass);
        a.accumulate = pass > 0 ? 1u : 0u;
        hipLaunchKernelGGL((k_eval_selop<OP>), dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a);
    }
}

// The mask of an operator call over [p] rows of W = ceil(n / 64) words, `pitch` words apart, enqueued on `s`: nlab = the snapshot's label
// columns [nkeys][n], psel = the batch's selector entries [nkeys][p] (nullptr, or nkeys == 0: no pod constrains anything -- the
// all-valid rows).  The geometry is sel_ops.hpp's; the one launch path (ksched_api.hip's launch_mask).
inline hipError_t run_selop(SelOp op, const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, uint32_t p, uint32_t n, uint32_t W, uint32_t pitch,
                            uint32_t nkeys, hipStream_t s) {
    if (p == 0 || W == 0) return hipSuccess;
    if (!out_feas || pitch < W) return hipErrorInvalidValue;
    if (!psel || !nlab) nkeys = 0;
    const SelopLaunch l = plan_selop_launch(p, W, nkeys);
    SelopArgs a{};
    a.n = n;
    a.p = p;
    a.W = W;
    a.pitch = pitch;
    a.pod_tiles_per_block = l.pod_tiles_per_block;
    switch (op) {
        case SelOp::kExists: launch_selop<SelOp::kExists>(nlab, psel, out_feas, l, a, nkeys, s); break;
        case SelOp::kGt: launch_selop<SelOp::kGt>(nlab, psel, out_feas, l, a, nkeys, s); break;
        case SelOp::kLt: launch_selop<SelOp::kLt>(nlab, psel, out_feas, l, a, nkeys, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ksched
