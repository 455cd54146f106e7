// kernels_pick_pack.hpp -- KSCHED_PICK_PACK (extension E5): the tightest of d uniformly drawn feasible nodes, from the mask.
//
// The contract (include/ksched.h): with c = the set bits of the pod's row over nodes [0, n), d = attempts and u_j = samples[pod * d + j],
// the binding is -1 when c == 0; else candidate v_j is the index of set bit number k_j = (uint64(u_j) * c) >> 32 in ascending node order
// (the uniform pick's rule, once per draw) and the binding is the candidate with the SMALLEST signed (avail_mem[v], avail_cpu[v]), memory
// first -- best fit's key: for a fixed pod the residual orders as `available` does -- the lowest node index among equals.  Integers and
// comparisons only: same inputs, same bits, whatever the draws' order.
//
// Shape: k_pick_spread's (kernels_pick_spread.hpp), whose spread_take this header uses together with kernels_pick_uniform.hpp's helpers --
// a wave per pod, nothing shared between waves: no atomics, no LDS, no barrier; a wave that exits early (pod >= p) affects nobody.  Lane
// j < d holds draw j, then k_j, then candidate v_j.
//  * W <= 128: the row is loaded once and stays in registers; one popcount and one wave scan serve all d selections.
//  * longer rows: a counting pass for c, then one walk over the chunks in row order; in every chunk a ballot names the draws whose k_j fall
//    into it and each is resolved there, so a chunk is read at most once and the walk stops with the chunk that resolves the last draw.
//  * comparison: lanes j < d gather avail_mem[v_j] and avail_cpu[v_j]; lanes at or beyond d repeat candidate 0, which changes no minimum;
//    ceil(log2 d) shuffle-down steps leave the minimum of (mem, cpu), then the lowest node, in lane 0, which stores it.
// The same bytes per pod as the spread pick.  The two kernels are separate bodies on purpose: with the candidate selection moved into one
// shared __device__ function the compiler allocates k_pick_spread's registers differently, and that kernel's instructions are to stay
// what they were (tools/same_device_code.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_pick_spread.hpp"

namespace ksched {

constexpr uint32_t kPackWaves = 4;  // waves (= pods) per block

// n >= 1, W = ceil(n / 64), pitch >= W, 1 <= d <= 64; nmem / ncpu: the snapshot's [n] columns
__global__ __launch_bounds__(64 * kPackWaves) void k_pick_pack(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ samples,
                                                               const int64_t *__restrict__ nmem, const int64_t *__restrict__ ncpu,
                                                               int32_t *__restrict__ binding, uint32_t p, uint32_t n, uint32_t W,
                                                               uint32_t pitch, uint32_t d) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pod = blockIdx.x * kPackWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
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

    // the smallest (mem, cpu), the lowest node among equals; lanes at or beyond d repeat candidate 0
    // (read before the select, with every lane active: inside the select's other arm the first active lane would be lane d)
    const uint32_t cand0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cand);
    uint32_t v = lane < d ? cand : cand0;
    int64_t m = nmem[v], q = ncpu[v];
    for (uint32_t s = 1; s < d; s <<= 1) {  // lane 0 ends with the minimum over lanes [0, 2^steps), which holds [0, d); a lane without a source keeps its own
        const int64_t om = __shfl_down(m, s, 64), oq = __shfl_down(q, s, 64);
        const uint32_t ov = (uint32_t)__shfl_down((int)v, s, 64);
        if (om < m || (om == m && (oq < q || (oq == q && ov < v)))) m = om, q = oq, v = ov;
    }
    if (lane == 0) *out = (int32_t)v;
}

}  // namespace ksched
