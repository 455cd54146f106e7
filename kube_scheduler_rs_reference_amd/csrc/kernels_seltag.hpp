// kernels_seltag.hpp -- k_eval_seltag: the mask of a TAGGED call (extension E9, include/ksched.h: KSCHED_SELOP_TAGGED).
//
// The contract (sel_tags.hpp: seltag_pass, seltag_row): per pod and key, with e the pod's selector entry, tag = e >> 29, id = e & 0x1FFFFFFF
// and v the node's whole label id: e == 0 passes; EQ: v == id; NE: v != id; EXISTS: v != 0; ABSENT: v == 0; GT: v != 0 && v > id;
// LT: v != 0 && v < id; tags 6 and 7 (KSCHED_SEL_NEVER among them) nowhere -- unsigned compares; the row is the AND over the keys, bits at
// or beyond n zero.
//
// k_eval_selop's mapping, geometry and arguments; the walk, the decode of an entry (sel_and_entry: no branch on the tag) and the launch are
// kernels_sel_walk.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ksched.h"
#include "kernarg.hpp"
#include "kernels_sel_walk.hpp"
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
                if (e != 0u) sel_and_entry(e, nlab[k], m);  // wave-uniform branch: unconstrained keys cost no VALU work
            }
            sel_park(m, j, flo, fhi);
        }
        sel_store_rows(out_feas, a.pitch, a.W, w0, p0, lane, jmax, flo, fhi, a.accumulate);
    }
}

inline void launch_seltag(const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, const SeltagLaunch &l, const SelopArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_eval_seltag, dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a);
}

}  // namespace ksched
