// kernels_selterms.hpp -- k_eval_selterms, k_eval_selterms_wide: the mask of a tagged call with a term count (extension E10,
// include/ksched.h: KSCHED_SEL_TERMS).
//
// The contract (sel_terms.hpp: selterms_row): the selector entries are [T][nkeys][p]; per pod the row is
//     valid bits AND ( OR over t of ( AND over k of seltag_pass(e[t][k][pod], v[k][node]) ) ),
// an entry read as sel_tags.hpp reads it (tag << 29 | id, tags 6 and 7 pass nowhere, entry 0 passes), bits at or beyond n zero.
//
// k_eval_seltag's mapping, geometry included; the walk, the decode of an entry (sel_and_entry) and the launch are kernels_sel_walk.hpp's.
//
// What the OR changes.  Per pod the T term words are formed and ORed in scalar registers, THEN parked once and stored once: the walk's
// fixed cost -- the writelanes, the row stores, the tile loop -- is paid once, not T times, and there is no combine pass over the mask.
// One wave-uniform shortcut: once a pod's OR equals the valid-bits word in every column of the wave, no further term can add a bit, and
// the remaining terms are not loaded.  A pod without affinity (all zeros) so costs one term whatever T is, and so does every pod whose
// first term is all zeros; the bits are unchanged because OR is monotonic and the row is ANDed with the valid bits anyway.  A padding term
// (KSCHED_SEL_NEVER in one key) needs no case of its own: its one entry decodes to the empty range and costs one key's work.
//
// Snapshots of more than kSelopKeys keys.  k_eval_seltag runs one launch per kSelopKeys keys and ANDs into the mask across launches.
// Under an OR that is wrong -- (A0 & A1) | (B0 & B1) is not (A0 | B0) & (A1 | B1) --: a term's AND must be complete over ALL keys before
// it is ORed.  k_eval_selterms_wide therefore walks the key passes inside the kernel: per pod tile and per term it runs the passes one after
// the other, reloading the wave's label ids of the pass's keys (kSelopKeys * kSelopCW dwords per lane: 8 KB per wave, from L2 -- the
// wave's whole label footprint is nkeys KB), parks the pass's words of the 64 pods in lanes and ANDs them into the term's words on the
// vector side; the finished term is ORed into the tile's words.  Chosen over keeping T partial words per pod in LDS: that is
// 64 pods x T x kSelopCW x 8 bytes = 30 KB per WAVE at T = 15, 120 KB per block, which would take the block to one per compute unit for a
// case (more than eight label keys AND several terms) that pays L2 reads instead.  The price is T * passes label reloads per pod tile and
// no early exit (the 64 pods of a tile do not agree on it).  The <= kSelopKeys case is a kernel of its own and pays none of this: its
// labels are loaded once per kernel and stay in registers.
//
// Rows and offsets are 64-bit (p * pitch and T * nkeys * p may pass 2^32).  Reads: labels [0, nkeys) x [0, n), entries
// [0, T * nkeys) x [0, p).  Writes: words [0, W) of rows [0, p).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ksched.h"
#include "kernarg.hpp"
#include "kernels_sel_walk.hpp"
#include "sel_terms.hpp"

namespace ksched {

// One term's entries of one pod, keys [0, nk) of the columns that start at `col`, `p` entries apart; e[k] = 0 for k >= nk.  ALL loads are
// issued before the first is used: a load per key under its own `k < nk` test is what the compiler turns into eight dependent
// load-and-wait steps (k_eval_seltag's form; against it this form measured 1 % faster at two terms per pod and 10 % at four -- DESIGN
// section 4: the scalar decode, not the loads' latency, is what the kernel waits for).  The key index is clamped instead, so that the
// loads are unconditional and stay inside the term's columns; nk == 0 (no selectors) loads nothing.
__device__ __forceinline__ void selterms_load_entries(const uint32_t *__restrict__ col, uint32_t p, uint32_t nk, uint32_t (&e)[kSelopKeys]) {
#pragma unroll
    for (uint32_t k = 0; k < kSelopKeys; ++k) e[k] = 0u;
    if (nk == 0u) return;
    const uint32_t last = nk - 1u;
    uint32_t raw[kSelopKeys];
#pragma unroll
    for (uint32_t k = 0; k < kSelopKeys; ++k) raw[k] = col[(size_t)min(k, last) * p];
#pragma unroll
    for (uint32_t k = 0; k < kSelopKeys; ++k) e[k] = k <= last ? raw[k] : 0u;
}

// up to kSelopKeys keys: the labels stay in registers for the whole kernel
__global__ __launch_bounds__(64 * kSelopWaves) void k_eval_selterms(const uint32_t *__restrict__ g_nlab, const uint32_t *__restrict__ g_psel,
                                                                     uint64_t *__restrict__ out_feas, const SeltermsArgs a) {
    kernarg_warm<3 * 8 + sizeof(SeltermsArgs)>();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t w0 = (blockIdx.x * kSelopWaves + wave) * kSelopCW;  // first word column of this wave
    if (w0 >= a.W) return;

    uint32_t nlab[kSelopKeys][kSelopCW];
    uint64_t valid[kSelopCW];
#pragma unroll
    for (uint32_t c = 0; c < kSelopCW; ++c) {
        const uint32_t node = (w0 + c) * 64u + lane;
        const bool in = w0 + c < a.W && node < a.n;
        valid[c] = __ballot(in);
#pragma unroll
        for (uint32_t k = 0; k < kSelopKeys; ++k) nlab[k][c] = (in && k < a.nkeys) ? g_nlab[(size_t)k * a.n + node] : 0u;
    }

    const uint32_t tile0 = blockIdx.y * a.pod_tiles_per_block;
    for (uint32_t tl = 0; tl < a.pod_tiles_per_block; ++tl) {
        const uint64_t first = (uint64_t)(tile0 + tl) * 64u;
        if (first >= a.p) break;
        const uint32_t p0 = (uint32_t)first;
        const uint32_t jmax = min(64u, a.p - p0);

        uint32_t flo[kSelopCW], fhi[kSelopCW];  // the word of pod (p0 + lane)
#pragma unroll
        for (uint32_t c = 0; c < kSelopCW; ++c) flo[c] = fhi[c] = 0u;

        for (uint32_t j = 0; j < jmax; ++j) {
            const uint32_t pod = p0 + j;  // wave-uniform -> scalar loads
            uint64_t acc[kSelopCW];
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) acc[c] = 0;
            for (uint32_t t = 0; t < a.terms; ++t) {
                uint64_t m[kSelopCW];
#pragma unroll
                for (uint32_t c = 0; c < kSelopCW; ++c) m[c] = valid[c];
                uint32_t e[kSelopKeys];
                selterms_load_entries(g_psel + (size_t)t * a.nkeys * a.p + pod, a.p, a.nkeys, e);
#pragma unroll
                for (uint32_t k = 0; k < kSelopKeys; ++k)
                    if (e[k] != 0u) sel_and_entry(e[k], nlab[k], m);  // wave-uniform branch: unconstrained keys cost no VALU work
                uint64_t missing = 0;
#pragma unroll
                for (uint32_t c = 0; c < kSelopCW; ++c) {
                    acc[c] |= m[c];
                    missing |= acc[c] ^ valid[c];
                }
                if (missing == 0) break;  // wave-uniform: every valid bit is set, no further term can add one
            }
            sel_park(acc, j, flo, fhi);
        }
        sel_store_rows(out_feas, a.pitch, a.W, w0, p0, lane, jmax, flo, fhi, 0u);
    }
}

// more than kSelopKeys keys: the key passes walked inside the kernel, per pod tile and term (the header comment says why)
__global__ __launch_bounds__(64 * kSelopWaves) void k_eval_selterms_wide(const uint32_t *__restrict__ g_nlab, const uint32_t *__restrict__ g_psel,
                                                                          uint64_t *__restrict__ out_feas, const SeltermsArgs a) {
    kernarg_warm<3 * 8 + sizeof(SeltermsArgs)>();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t w0 = (blockIdx.x * kSelopWaves + wave) * kSelopCW;
    if (w0 >= a.W) return;

    uint64_t valid[kSelopCW];
    bool in[kSelopCW];
#pragma unroll
    for (uint32_t c = 0; c < kSelopCW; ++c) {
        const uint32_t node = (w0 + c) * 64u + lane;
        in[c] = w0 + c < a.W && node < a.n;
        valid[c] = __ballot(in[c]);
    }

    const uint32_t tile0 = blockIdx.y * a.pod_tiles_per_block;
    for (uint32_t tl = 0; tl < a.pod_tiles_per_block; ++tl) {
        const uint64_t first = (uint64_t)(tile0 + tl) * 64u;
        if (first >= a.p) break;
        const uint32_t p0 = (uint32_t)first;
        const uint32_t jmax = min(64u, a.p - p0);

        uint32_t flo[kSelopCW], fhi[kSelopCW];  // the OR over the terms, word of pod (p0 + lane)
#pragma unroll
        for (uint32_t c = 0; c < kSelopCW; ++c) flo[c] = fhi[c] = 0u;

        for (uint32_t t = 0; t < a.terms; ++t) {
            uint32_t tlo[kSelopCW], thi[kSelopCW];  // the term's AND over the passes done so far
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) tlo[c] = thi[c] = 0xFFFFFFFFu;

            for (uint32_t pass = 0; pass < a.key_passes; ++pass) {
                const uint32_t key0 = pass * kSelopKeys;
                const uint32_t nk = min(kSelopKeys, a.nkeys - key0);  // (key_passes = ceil(nkeys / kSelopKeys): key0 < nkeys)
                uint32_t nlab[kSelopKeys][kSelopCW];
#pragma unroll
                for (uint32_t c = 0; c < kSelopCW; ++c) {
                    const uint32_t node = (w0 + c) * 64u + lane;
#pragma unroll
                    for (uint32_t k = 0; k < kSelopKeys; ++k) nlab[k][c] = (in[c] && k < nk) ? g_nlab[(size_t)(key0 + k) * a.n + node] : 0u;
                }
                uint32_t plo[kSelopCW], phi[kSelopCW];  // this pass's word of pod (p0 + lane)
#pragma unroll
                for (uint32_t c = 0; c < kSelopCW; ++c) plo[c] = phi[c] = 0u;

                for (uint32_t j = 0; j < jmax; ++j) {
                    const uint32_t pod = p0 + j;  // wave-uniform -> scalar loads
                    uint64_t m[kSelopCW];
#pragma unroll
                    for (uint32_t c = 0; c < kSelopCW; ++c) m[c] = valid[c];
                    // (a load per key, as in k_eval_seltag: with the pass loop's state the batched form of selterms_load_entries takes
                    // this kernel past the scalar register file -- three SGPRs spilled -- and the wide case is the rare one)
                    const uint32_t *col = g_psel + ((size_t)t * a.nkeys + key0) * a.p + pod;
#pragma unroll
                    for (uint32_t k = 0; k < kSelopKeys; ++k) {
                        const uint32_t e = (k < nk) ? col[(size_t)k * a.p] : 0u;
                        if (e != 0u) sel_and_entry(e, nlab[k], m);
                    }
                    sel_park(m, j, plo, phi);
                }
#pragma unroll
                for (uint32_t c = 0; c < kSelopCW; ++c) tlo[c] &= plo[c], thi[c] &= phi[c];
            }
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) flo[c] |= tlo[c], fhi[c] |= thi[c];
        }
        sel_store_rows(out_feas, a.pitch, a.W, w0, p0, lane, jmax, flo, fhi, 0u);
    }
}

inline void launch_selterms(const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, const SeltermsLaunch &l, const SeltermsArgs &a, hipStream_t s) {
    if (l.wide) hipLaunchKernelGGL(k_eval_selterms_wide, dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a);
    else hipLaunchKernelGGL(k_eval_selterms, dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a);
}

}  // namespace ksched
