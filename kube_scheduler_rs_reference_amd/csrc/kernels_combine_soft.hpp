// kernels_combine_soft.hpp -- k_mask_combine_soft (extension E7): narrow the caller's mask by the mask one evaluation wrote, row by row,
// unless that would leave the row empty.
//
// The contract (include/ksched.h, KSCHED_COMBINE_SOFT): per pod row, old' = dst's words [0, W) with the bits at or beyond n of the last
// word cleared, r = old' OP src with OP one of AND, AND-NOT.  If r has a set bit the row becomes r, else it becomes old'.  Words [W, pitch)
// of either buffer are neither read nor written.  src is the ctx's scratch mask, which the mask kernel of the same call has just written
// at the same pitch; dst is the caller's out_feasible.  The two never overlap.
//
// Shape: the decision needs the whole row, so a row belongs to one GROUP of lanes of one wave (1 .. 64 lanes, a power of two; 64 / group
// rows per wave: mask_combine_soft.hpp).  Lane j of the group loads the units j, j + group, ... of its row from both buffers -- a unit is
// k_mask_combine's: 16 bytes where both buffers allow it (WIDE), else 8 --, all of them before it uses any, computes r, and the group
// decides with ONE __ballot of "my r has a set bit", of which every group reads its own lanes' bits: no LDS, no atomics, no barrier.
// Then the stores: r for a row that narrows; for a row that does not, nothing -- except the row's last word where clearing the bits at or
// beyond n changes it, by the one lane that holds it.  So the kernel moves what k_mask_combine moves, or less.
// KEEP: the lane keeps its (at most kSoftKeepUnits) units in registers from the loads to the stores.  A longer row (!KEEP, a whole wave per
// row) is read twice, once to decide and once to store.
// The grid is bounded (kSoftMaxGrid) and strides over the rows; rows are counted in 64 bits and offsets are 64-bit: p * pitch words may
// exceed 2^32.  The rows of one wave differ in their decisions, so the store is predicated per group; lanes past their row's last unit
// idle.  Plain loads and stores, as in k_mask_combine: the combined mask is read next by a pick or by the next tier's call.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_combine.hpp"
#include "mask_combine_soft.hpp"

namespace ksched {

struct SoftArgs {
    uint32_t p, W, pitch;     // rows, words per row that are combined, words between consecutive rows (of dst and of src)
    uint32_t units_per_row;   // ceil(W / 2) WIDE, else W
    uint32_t units_per_lane;  // ceil(units_per_row / group)
    uint32_t group_shift;     // log2(lanes per row)
    uint32_t rows_per_pass;   // the grid stride, in rows
    uint64_t valid;           // valid_bits_word(n)
};

// a unit of the row that starts `row_off` words into the buffers; col < units_per_row, so w0 < W
template <bool WIDE>
__device__ __forceinline__ CombineUnit soft_unit(size_t row_off, uint32_t col, uint32_t W) {
    const uint32_t w0 = WIDE ? 2u * col : col;
    return CombineUnit{row_off + w0, w0, WIDE && w0 + 1u < W};
}

// what a lane knows about its row's last word, if it holds it: old' of that word, and whether old' differs from what dst holds
struct SoftLast {
    uint64_t word = 0;
    bool fix = false;
};

// d, the unit's words of dst, becomes old'; returns r
template <CombineOp OP>
__device__ __forceinline__ combine_u64x2 soft_fold(const CombineUnit &u, combine_u64x2 &d, combine_u64x2 s, const SoftArgs &a, SoftLast &last) {
    const uint32_t lw = a.W - 1u;
    if (u.w0 == lw) {
        last.fix = (d.x & ~a.valid) != 0;
        last.word = d.x &= a.valid;
    }
    if (u.pair && u.w0 + 1u == lw) {
        last.fix = (d.y & ~a.valid) != 0;
        last.word = d.y &= a.valid;
    }
    combine_u64x2 r;
    r.x = combine_apply<OP>(d.x, s.x);
    r.y = combine_apply<OP>(d.y, s.y);  // (a one-word unit: d.y = s.y = 0 gives 0 under either op)
    return r;
}

__device__ __forceinline__ void soft_store(uint64_t *__restrict__ dst, const CombineUnit &u, combine_u64x2 r) {
    if (u.pair) *reinterpret_cast<combine_u64x2 *>(dst + u.off) = r;
    else dst[u.off] = r.x;
}

// launched with plan_soft_launch's grid of kSoftBlock threads; p >= 1, W >= 1, pitch >= W; OP is kAnd or kAndNot
template <CombineOp OP, bool WIDE, bool KEEP>
__global__ __launch_bounds__(kSoftBlock) void k_mask_combine_soft(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, SoftArgs a) {
    const uint32_t t = blockIdx.x * kSoftBlock + threadIdx.x;  // (grid * block <= 2^19)
    const uint32_t group = 1u << a.group_shift, j = t & (group - 1u);
    const uint32_t first_lane = (threadIdx.x & (kSoftWave - 1u)) & ~(group - 1u);  // of the lane's group, in its wave
    const uint64_t group_bits = group == kSoftWave ? ~0ull : (1ull << group) - 1ull;
    for (uint64_t row = t >> a.group_shift; row < a.p; row += a.rows_per_pass) {  // (uniform in a group; groups of a wave may leave at different passes)
        const size_t row_off = (size_t)row * a.pitch;
        SoftLast last;
        uint64_t any = 0;
        if (KEEP) {
            combine_u64x2 d[kSoftKeepUnits], s[kSoftKeepUnits];
#pragma unroll
            for (uint32_t k = 0; k < kSoftKeepUnits; ++k) {  // every load of the row before the first use
                const uint32_t col = j + (k << a.group_shift);
                if (k < a.units_per_lane && col < a.units_per_row) combine_load(dst, src, soft_unit<WIDE>(row_off, col, a.W), d[k], s[k]);
                else d[k] = s[k] = combine_u64x2{0, 0};
            }
#pragma unroll
            for (uint32_t k = 0; k < kSoftKeepUnits; ++k) {
                const uint32_t col = j + (k << a.group_shift);
                if (k < a.units_per_lane && col < a.units_per_row) {
                    d[k] = soft_fold<OP>(soft_unit<WIDE>(row_off, col, a.W), d[k], s[k], a, last);
                    any |= d[k].x | d[k].y;
                }
            }
            const bool narrows = ((__ballot(any != 0) >> first_lane) & group_bits) != 0;
            if (narrows) {
#pragma unroll
                for (uint32_t k = 0; k < kSoftKeepUnits; ++k) {
                    const uint32_t col = j + (k << a.group_shift);
                    if (k < a.units_per_lane && col < a.units_per_row) soft_store(dst, soft_unit<WIDE>(row_off, col, a.W), d[k]);
                }
            } else if (last.fix) {
                dst[row_off + a.W - 1u] = last.word;
            }
        } else {
#pragma unroll 4
            for (uint32_t k = 0; k < a.units_per_lane; ++k) {
                const uint32_t col = j + (k << a.group_shift);
                if (col < a.units_per_row) {
                    const CombineUnit u = soft_unit<WIDE>(row_off, col, a.W);
                    combine_u64x2 d, s;
                    combine_load(dst, src, u, d, s);
                    const combine_u64x2 r = soft_fold<OP>(u, d, s, a, last);
                    any |= r.x | r.y;
                }
            }
            const bool narrows = ((__ballot(any != 0) >> first_lane) & group_bits) != 0;
            if (narrows) {
#pragma unroll 4
                for (uint32_t k = 0; k < a.units_per_lane; ++k) {  // the second read: mostly from the caches the first one filled
                    const uint32_t col = j + (k << a.group_shift);
                    if (col < a.units_per_row) {
                        const CombineUnit u = soft_unit<WIDE>(row_off, col, a.W);
                        combine_u64x2 d, s;
                        combine_load(dst, src, u, d, s);
                        soft_store(dst, u, soft_fold<OP>(u, d, s, a, last));
                    }
                }
            } else if (last.fix) {
                dst[row_off + a.W - 1u] = last.word;
            }
        }
    }
}

template <CombineOp OP>
inline void launch_mask_combine_soft(uint64_t *dst, const uint64_t *src, const SoftLaunch &l, const SoftArgs &a, hipStream_t s) {
    const dim3 grid(l.grid), block(l.block);
    if (l.vec == 2) {
        if (l.keep) hipLaunchKernelGGL((k_mask_combine_soft<OP, true, true>), grid, block, 0, s, dst, src, a);
        else hipLaunchKernelGGL((k_mask_combine_soft<OP, true, false>), grid, block, 0, s, dst, src, a);
    } else {
        if (l.keep) hipLaunchKernelGGL((k_mask_combine_soft<OP, false, true>), grid, block, 0, s, dst, src, a);
        else hipLaunchKernelGGL((k_mask_combine_soft<OP, false, false>), grid, block, 0, s, dst, src, a);
    }
}

// the soft combine of dst with src over [p] rows of W = ceil(n / 64) words, `pitch` words apart in both buffers, enqueued on `s`: the access
// width is mask_combine.hpp's, the geometry mask_combine_soft.hpp's.  The one launch path (ksched_api.hip's launch_mask;
// tools/mask_combine_bench.hip times the same call, and with `read_twice` the two-read form at rows that fit in registers, which no caller
// of the library can ask for).
inline hipError_t run_mask_combine_soft(CombineOp op, uint64_t *dst, const uint64_t *src, uint32_t p, uint32_t n, uint32_t W, uint32_t pitch, hipStream_t s,
                                        bool read_twice = false) {
    if (p == 0 || W == 0) return hipSuccess;
    SoftLaunch l = plan_soft_launch(p, W, combine_vec_words((uint64_t)(uintptr_t)dst, (uint64_t)(uintptr_t)src, pitch));
    if (read_twice) l.keep = false;
    const SoftArgs a{p, W, pitch, l.units_per_row, l.units_per_lane, l.group_shift, l.rows_per_pass, valid_bits_word(n)};
    switch (op) {
        case CombineOp::kAnd: launch_mask_combine_soft<CombineOp::kAnd>(dst, src, l, a, s); break;
        case CombineOp::kAndNot: launch_mask_combine_soft<CombineOp::kAndNot>(dst, src, l, a, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ksched
