// kernels_selterms.hpp -- k_eval_selterms, k_eval_selterms_wide: the mask of a tagged call with a term count (extension E10,
// include/ksched.h: KSCHED_SEL_TERMS).
//
// The contract (sel_terms.hpp: selterms_row): the selector entries are [T][nkeys][p]; per pod the row is
//     valid bits AND ( OR over t of ( AND over k of seltag_pass(e[t][k][pod], v[k][node]) ) ),
// an entry read as sel_tags.hpp reads it (tag << 29 | id, tags 6 and 7 pass nowhere, entry 0 passes), bits at or beyond n zero.
//
// Mapping: k_eval_seltag's (kernels_seltag.hpp), geometry included.  One wave owns kSelopCW consecutive 64-node word columns whose label
// ids live in VGPRs; it walks pods 64 at a time; a pod's entries are wave-uniform and come in through the scalar cache; the tag is decoded
// on the scalar side into the one compare form  word = ballot(v - lo < len) ^ neg  (no branch on the tag); the word of pod j is parked in
// lane j by v_writelane, and after 64 pods every lane stores kSelopCW consecutive words of its pod row with plain vector stores.
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
#include "kernels_direct.hpp"  // ksched_writelane_u32
#include "sel_terms.hpp"

namespace ksched {

struct SeltermsArgs {
    uint32_t n, p, W;
    uint32_t pitch;                // words between consecutive pod rows of the mask (>= W)
    uint32_t nkeys;                // all of the snapshot's keys (0: no key at all); k_eval_selterms: <= kSelopKeys
    uint32_t terms;                // T >= 1
    uint32_t pod_tiles_per_block;  // 64-pod tiles walked by one block
    uint32_t key_passes;           // k_eval_selterms_wide: ceil(nkeys / kSelopKeys)
};

// m[c] &= [entry e against the label ids v[c]] for a constrained entry (e != 0): kernels_seltag.hpp's decode, seltag_form_bits' arithmetic
// (sel_tags.hpp) on the scalar side, then a v_sub and one v_cmp per column.  The two v_readfirstlane keep the chain of words on the scalar
// unit (kernels_seltag.hpp says what happens without them).
__device__ __forceinline__ void selterms_and_entry(uint32_t e, const uint32_t (&v)[kSelopCW], uint64_t (&m)[kSelopCW]) {
    const uint32_t tag = e >> KSCHED_SELTAG_SHIFT, id = e & KSCHED_SELTAG_ID_MASK;
    const uint32_t t0 = tag & 1u, t1 = (tag >> 1) & 1u, t2 = tag >> 2;
    const uint32_t neg32 = __builtin_amdgcn_readfirstlane(0u - (t0 & (t2 ^ 1u)));  // NE, ABSENT: all ones
    const uint64_t neg = ((uint64_t)neg32 << 32) | neg32;
    const uint32_t by_id = 0u - ((t1 ^ 1u) & ((t0 & t2) ^ 1u));  // EQ, NE, GT: the range starts at the id
    const uint32_t lo = (id & by_id) + (t1 | t2);                // ... (+ 1 for GT); EXISTS, ABSENT, LT: at 1
    const uint32_t len45 = ((id - (id != 0u ? 1u : 0u)) & (0u - t0)) | (~id & (t0 - 1u));  // LT: [1, id); GT: (id, 2^32)
    const uint32_t len03 = 1u | (0u - t1);                                                 // EQ, NE: the id alone; EXISTS, ABSENT: [1, 2^32)
    const uint32_t len = __builtin_amdgcn_readfirstlane(((len45 & (0u - t2)) | (len03 & (t2 - 1u))) & (0u - ((t1 & t2) ^ 1u)));  // tags 6, 7: empty
#pragma unroll
    for (uint32_t c = 0; c < kSelopCW; ++c) m[c] &= __ballot(v[c] - lo < len) ^ neg;  // (m starts as the valid-bits word: applied after the xor)
}

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
                    if (e[k] != 0u) selterms_and_entry(e[k], nlab[k], m);  // wave-uniform branch: unconstrained keys cost no VALU work
                uint64_t missing = 0;
#pragma unroll
                for (uint32_t c = 0; c < kSelopCW; ++c) {
                    acc[c] |= m[c];
                    missing |= acc[c] ^ valid[c];
                }
                if (missing == 0) break;  // wave-uniform: every valid bit is set, no further term can add one
            }
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) {
                flo[c] = ksched_writelane_u32((uint32_t)acc[c], j, flo[c]);
                fhi[c] = ksched_writelane_u32((uint32_t)(acc[c] >> 32), j, fhi[c]);
            }
        }

        if (lane < jmax) {
            const size_t row = (size_t)(p0 + lane) * a.pitch;
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c)
                if (w0 + c < a.W) out_feas[row + w0 + c] = ((uint64_t)fhi[c] << 32) | flo[c];
        }
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
                        if (e != 0u) selterms_and_entry(e, nlab[k], m);
                    }
#pragma unroll
                    for (uint32_t c = 0; c < kSelopCW; ++c) {
                        plo[c] = ksched_writelane_u32((uint32_t)m[c], j, plo[c]);
                        phi[c] = ksched_writelane_u32((uint32_t)(m[c] >> 32), j, phi[c]);
                    }
                }
#pragma unroll
                for (uint32_t c = 0; c < kSelopCW; ++c) tlo[c] &= plo[c], thi[c] &= phi[c];
            }
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c) flo[c] |= tlo[c], fhi[c] |= thi[c];
        }

        if (lane < jmax) {
            const size_t row = (size_t)(p0 + lane) * a.pitch;
#pragma unroll
            for (uint32_t c = 0; c < kSelopCW; ++c)
                if (w0 + c < a.W) out_feas[row + w0 + c] = ((uint64_t)fhi[c] << 32) | flo[c];
        }
    }
}

// The mask of a tagged call with `terms` >= 1 terms over [p] rows of W = ceil(n / 64) words, `pitch` words apart, enqueued on `s`: nlab =
// the snapshot's label columns [nkeys][n], psel = the batch's tagged entries [terms][nkeys][p] (nullptr, or nkeys == 0: no pod constrains
// anything -- the all-valid rows).  ONE launch; the geometry is sel_terms.hpp's; the one launch path (ksched_api.hip's launch_mask).
inline hipError_t run_selterms(const uint32_t *nlab, const uint32_t *psel, uint64_t *out_feas, uint32_t p, uint32_t n, uint32_t W, uint32_t pitch, uint32_t nkeys,
                               uint32_t terms, hipStream_t s) {
    if (p == 0 || W == 0) return hipSuccess;
    if (!out_feas || pitch < W || terms == 0 || terms > KSCHED_MAX_TERMS) return hipErrorInvalidValue;
    if (!psel || !nlab) nkeys = 0;
    const SeltermsLaunch l = plan_selterms_launch(p, W, nkeys, terms);
    SeltermsArgs a{};
    a.n = n;
    a.p = p;
    a.W = W;
    a.pitch = pitch;
    a.nkeys = nkeys;
    a.terms = l.terms;
    a.pod_tiles_per_block = l.pod_tiles_per_block;
    a.key_passes = l.key_passes;
    if (l.wide) hipLaunchKernelGGL(k_eval_selterms_wide, dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a);
    else hipLaunchKernelGGL(k_eval_selterms, dim3(l.gx, l.gy), dim3(l.block), 0, s, nlab, psel, out_feas, a);
    return hipGetLastError();
}

}  // namespace ksched
