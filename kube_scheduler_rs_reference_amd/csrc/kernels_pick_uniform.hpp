// kernels_pick_uniform.hpp -- KSCHED_PICK_UNIFORM (extension E3): a uniform pick among each pod's feasible nodes, from the mask.
//
// The contract (include/ksched.h): with c = the set bits of the pod's row over nodes [0, n) and u = samples[pod * attempts],
// the binding is -1 when c == 0, else the index of set bit number k = (uint64(u) * c) >> 32 in ascending node order.  Exact
// integer arithmetic throughout: same inputs, same bits.
//
// Shape: a wave per pod, nothing shared between waves -- no atomics, no LDS, no barrier, no wave waits on another; a wave that
// exits early (pod >= p) affects nobody.  Lane l of a wave takes words 2l and 2l + 1 of every 128-word (1 KB) chunk of the row:
// neighbouring lanes read neighbouring 16 bytes.  Row bases are 8-byte aligned only (pitch = W = 79 at 5 000 nodes), so the two
// words are loaded as two 8-byte loads; words at or beyond W are never loaded, bits at or beyond n never counted.
//  * W <= 128: the row stays in registers -- per-lane population count, wave inclusive scan (in registers too: DPP), the lane whose
//    range holds k selects the bit inside its two words.
//  * longer rows: a first pass accumulates c; a second pass walks the chunks in row order with a running base and stops in the
//    chunk that holds k (that partial second read of the row comes from cache: a row is at most 256 KB).
// A read-bandwidth kernel: W words of mask, 4 B of draw and 4 B of binding per pod.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ksched {

constexpr uint32_t kUniformWaves = 4;         // waves (= pods) per block
constexpr uint32_t kUniformChunkWords = 128;  // words of a row one wave holds at a time: two per lane

// index of set bit number r (0-based, ascending) of x; r < popcount(x)
__device__ __forceinline__ uint32_t select_bit64(uint64_t x, uint32_t r) {
    uint32_t pos = 0;
    const uint32_t c32 = (uint32_t)__popc((uint32_t)x);
    uint32_t v = (uint32_t)x;
    if (r >= c32) {
        r -= c32;
        v = (uint32_t)(x >> 32);
        pos = 32;
    }
#pragma unroll
    for (uint32_t s = 16; s >= 1; s >>= 1) {
        const uint32_t c = (uint32_t)__popc(v & ((1u << s) - 1u));
        if (r >= c) {
            r -= c;
            v >>= s;
            pos += s;
        }
    }
    return pos;
}

// KSCHED_UNIFORM_SCAN: how a wave's prefix sum runs (a build-time variant for A/B timing, tools/build_variants.sh): 1 (default) = in
// registers, six DPP adds; 0 = six cross-lane shuffles through the LDS crossbar.  Same sums either way.
#ifndef KSCHED_UNIFORM_SCAN
#define KSCHED_UNIFORM_SCAN 1
#endif

// inclusive prefix sum over the 64 lanes of a wave (every lane active)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#if KSCHED_UNIFORM_SCAN
    // log steps within each row of 16 lanes (row_shr: a lane without a source adds 0), then the last lane of rows 0 / 2 into rows 1 / 3
    // (row_bcast:15, row mask 0xa) and lane 31 into rows 2 and 3 (row_bcast:31, row mask 0xc)
    (void)lane;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
#else
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += up;
    }
#endif
    return v;
}

// the wave's total: lane 63 of the inclusive scan, as a wave-uniform value
__device__ __forceinline__ uint32_t wave_total(uint32_t incl) { return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63); }

// the lane's two words of the chunk that starts at word `base`: words at or beyond W read as zero, the last word loses its bits at or beyond n
__device__ __forceinline__ void load_pair(const uint64_t *__restrict__ row, uint32_t base, uint32_t lane, uint32_t W, uint64_t last_mask,
                                          uint64_t &a, uint64_t &b) {
    const uint32_t w0 = base + 2u * lane, w1 = w0 + 1u;
    a = w0 < W ? row[w0] : 0ull;
    b = w1 < W ? row[w1] : 0ull;
    if (w0 == W - 1u) a &= last_mask;
    if (w1 == W - 1u) b &= last_mask;
}

// the lane whose range [excl, excl + popc(a) + popc(b)) holds k writes the node of set bit number k
__device__ __forceinline__ void select_in_chunk(uint64_t a, uint64_t b, uint32_t incl, uint32_t k, uint32_t base, uint32_t lane,
                                                int32_t *__restrict__ out) {
    const uint32_t ca = (uint32_t)__popcll(a), cnt = ca + (uint32_t)__popcll(b), excl = incl - cnt;
    if (k >= excl && k < incl) {
        const uint32_t r = k - excl, w0 = base + 2u * lane;
        *out = r < ca ? (int32_t)(w0 * 64u + select_bit64(a, r)) : (int32_t)((w0 + 1u) * 64u + select_bit64(b, r - ca));
    }
}

// n >= 1, W = ceil(n / 64), pitch >= W, 1 <= attempts
__global__ __launch_bounds__(64 * kUniformWaves) void k_pick_uniform(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ samples,
                                                                     int32_t *__restrict__ binding, uint32_t p, uint32_t n, uint32_t W,
                                                                     uint32_t pitch, uint32_t attempts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pod = blockIdx.x * kUniformWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pod >= p) return;  // the whole wave
    const uint64_t *__restrict__ row = mask + (size_t)pod * pitch;
    const uint32_t u = samples[(size_t)pod * attempts];
    const uint64_t last_mask = (n & 63u) ? ((1ull << (n & 63u)) - 1ull) : ~0ull;
    int32_t *out = binding + pod;

    if (W <= kUniformChunkWords) {
        uint64_t a, b;
        load_pair(row, 0, lane, W, last_mask, a, b);
        const uint32_t incl = wave_inclusive_scan((uint32_t)__popcll(a) + (uint32_t)__popcll(b), lane);
        const uint32_t c = wave_total(incl);
        if (c == 0) {
            if (lane == 0) *out = -1;
            return;
        }
        select_in_chunk(a, b, incl, (uint32_t)(((uint64_t)u * c) >> 32), 0, lane, out);
        return;
    }

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
    const uint32_t k = (uint32_t)(((uint64_t)u * c) >> 32);
    // second pass: the chunk that holds k (k < c: there is one)
    uint32_t run = 0;
    for (uint32_t base = 0; base < W; base += kUniformChunkWords) {
        uint64_t a, b;
        load_pair(row, base, lane, W, last_mask, a, b);
        const uint32_t incl = wave_inclusive_scan((uint32_t)__popcll(a) + (uint32_t)__popcll(b), lane);
        const uint32_t tot = wave_total(incl);
        if (k < run + tot) {
            select_in_chunk(a, b, incl, k - run, base, lane, out);
            return;
        }
        run += tot;
    }
}

}  // namespace ksched
