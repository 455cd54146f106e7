// kernels_pick_spread.hpp -- KSCHED_PICK_SPREAD (extension E4): the least loaded of d uniformly drawn feasible nodes, from the mask.
//
// The contract (include/ksched.h): with c = the set bits of the pod's row over nodes [0, n), d = attempts and u_j = samples[pod * d + j],
// the binding is -1 when c == 0; else candidate v_j is the index of set bit number k_j = (uint64(u_j) * c) >> 32 in ascending node order
// (the uniform pick's rule, once per draw) and the binding is the candidate with the largest signed (avail_mem[v], avail_cpu[v]), memory
// first, the lowest node index among equals.  Exact integer arithmetic throughout: same inputs, same bits, whatever the draws' order.
//
// Shape: k_pick_uniform's (kernels_pick_uniform.hpp, whose helpers this header uses) -- a wave per pod, nothing shared between waves: no
// atomics, no LDS, no barrier, no wave waits on another; a wave that exits early (pod >= p) affects nobody.  Lane j < d holds draw j (one
// coalesced load of the pod's d draws), then k_j, then candidate v_j: that is why d <= 64 (KSCHED_MAX_ATTEMPTS).
//  * W <= 128: the row is loaded once and stays in registers; one popcount and one wave scan serve all d selections.  Selection j takes k_j
//    out of lane j (the loop counter is wave-uniform), the lane whose range holds it selects the bit inside its two words, and the node
//    goes back into lane j.
//  * longer rows: a first pass accumulates c; a second pass walks the chunks in row order with a running base.  In every chunk a ballot names
//    the draws whose k_j fall into it -- in whatever order they arrived -- and each of them is resolved there: a chunk is read at most once
//    however large d is, and the walk stops with the chunk that resolves the last draw (that partial second read comes from cache).
//  * comparison: lanes j < d gather avail_mem[v_j] and avail_cpu[v_j] (two 8-byte columns, 800 KB at 50 k nodes: L2 resident); lanes at or
//    beyond d repeat candidate 0, which changes no maximum; ceil(log2 d) shuffle-down steps leave the maximum of (mem, cpu, lowest node) in
//    lane 0, which stores it.
// Per pod: W words of mask (as the uniform pick), 4 d bytes of draws, 16 d bytes of gathered columns, 4 bytes of binding.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_pick_uniform.hpp"

namespace ksched {

constexpr uint32_t kSpreadWaves = 4;  // waves (= pods) per block

// draw j's candidate out of one chunk (k < the chunk's set bits): the lane whose range [excl, excl + popc(a) + popc(b)) holds k selects
// the node of set bit number k, and lane j takes it.  j and k are wave-uniform.
__device__ __forceinline__ void spread_take(uint64_t a, uint64_t b, uint32_t incl, uint32_t k, uint32_t base, uint32_t lane, uint32_t j,
                                            uint32_t &cand) {
    const uint32_t ca = (uint32_t)__popcll(a), cnt = ca + (uint32_t)__popcll(b), excl = incl - cnt;
    const bool mine = k >= excl && k < incl;  // exactly one lane: the ranges are disjoint and cover [0, total)
    uint32_t node = 0;
    if (mine) {
        const uint32_t r = k - excl, w0 = base + 2u * lane;
        node = r < ca ? w0 * 64u + select_bit64(a, r) : (w0 + 1u) * 64u + select_bit64(b, r - ca);
    }
    const uint32_t owner = (uint32_t)__ffsll((unsigned long long)__ballot(mine)) - 1u;
    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)node, (int)owner);
    if (lane == j) cand = v;
}

// n >= 1, W = ceil(n / 64), pitch >= W, 1 <= d <= 64; nmem / ncpu: the snapshot's [n] columns
__global__ __launch_bounds__(64 * kSpreadWaves) void k_pick_spread(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ samples,
                                                                   const int64_t *__restrict__ nmem, const int64_t *__restrict__ ncpu,
                                                                   int32_t *__restrict__ binding, uint32_t p, uint32_t n, uint32_t W,
                                                                   uint32_t pitch, uint32_t d) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pod = blockIdx.x * kSpreadWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pod >= p) return;  // the whole wave
    const uint64_t *__restrict__ row = mask + (size_t)pod * pitch;
    const uint32_t u = lane < d ? samples[(size_t)pod * d + lane] : 0u;
    const uint64_t last_mask = (n & 63u) ? ((1ull << (n & 63u)) - 1ull) : ~0ull;
    int32_t *out = binding + pod;
    uint32_t cand = 0;  // lane j < d: candidate v_j

    if (W <= kUniformChunkWords) {
        uint64_t a, b;
        load_pair(row, 0, lane, W, last_mask, a, b);
        const uint32_t incl = wave_inclusive_scan((uint32_t)__popcll(a) + (uint32_t)__popcll(b), lane);
        const uint32_t c = wave_total(incl);
        if (c == 0) {
            if (lane == 0) *out = -1;
            return;
        }
        const uint32_t kv = (uint32_t)(((uint64_t)u * c) >> 32);
        for (uint32_t j = 0; j < d; ++j) spread_take(a, b, incl, (uint32_t)__builtin_amdgcn_readlane((int)kv, (int)j), 0, lane, j, cand);
    } else {
        // first pass: c
        uint32_t mine = 0;
#pragma unroll 4
        for (uint32_t base = 0; base < W; base += kUniformChunkWords) {
            uint64_t a, b;
            load_pair(row, base, lane, W, last_mask, a, b);
            mine += (uint32_t)__popcll(a) + (uint32_t)__popcll(b);
        }
        const uint32_t c = wave_total(wave_inclusive_scan(mine, lane));
        if (c == 0) {
            if (lane == 0) *out = -1;
            return;
        }
        const uint32_t kv = (uint32_t)(((uint64_t)u * c) >> 32);
        // second pass: every chunk resolves the draws that fall into it (every k_j < c: each falls into one)
        uint32_t run = 0, left = d;
        for (uint32_t base = 0; base < W && left; base += kUniformChunkWords) {
            uint64_t a, b;
            load_pair(row, base, lane, W, last_mask, a, b);
            const uint32_t incl = wave_inclusive_scan((uint32_t)__popcll(a) + (uint32_t)__popcll(b), lane);
            const uint32_t tot = wave_total(incl);
            unsigned long long here = __ballot(lane < d && kv >= run && kv - run < tot);
            left -= (uint32_t)__popcll(here);
            while (here) {
                const uint32_t j = (uint32_t)__ffsll(here) - 1u;
                here &= here - 1ull;
                spread_take(a, b, incl, (uint32_t)__builtin_amdgcn_readlane((int)kv, (int)j) - run, base, lane, j, cand);
            }
            run += tot;
        }
    }

    // the largest (mem, cpu), the lowest node among equals; lanes at or beyond d repeat candidate 0
    // (read before the select, with every lane active: inside the select's other arm the first active lane would be lane d)
    const uint32_t cand0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cand);
    uint32_t v = lane < d ? cand : cand0;
    int64_t m = nmem[v], q = ncpu[v];
    for (uint32_t s = 1; s < d; s <<= 1) {  // lane 0 ends with the maximum over lanes [0, 2^steps), which holds [0, d); a lane without a source keeps its own
        const int64_t om = __shfl_down(m, s, 64), oq = __shfl_down(q, s, 64);
        const uint32_t ov = (uint32_t)__shfl_down((int)v, s, 64);
        if (om > m || (om == m && (oq > q || (oq == q && ov < v)))) m = om, q = oq, v = ov;
    }
    if (lane == 0) *out = (int32_t)v;
}

}  // namespace ksched
