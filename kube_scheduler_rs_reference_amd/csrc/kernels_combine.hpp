// kernels_combine.hpp -- k_mask_combine (extension E6): fold the mask one evaluation wrote into the mask the caller holds.
//
// The contract (include/ksched.h): per pod row, dst[w] = dst[w] OP src[w] for the words w < W, OP one of AND, OR, AND-NOT; the row's
// last word is then ANDed with the valid-bits word, so bits at or beyond n come out zero whatever dst held there.  Words [W, pitch) of
// either buffer are neither read nor written.  src is the ctx's scratch mask, which the mask kernel of the same call has just written
// at the same pitch; dst is the caller's out_feasible.  The two never overlap.
//
// Shape: a pure streaming kernel -- two reads and one write per word, no LDS, no atomics, no barrier, nothing shared between lanes.  A
// unit of a row is two neighbouring words as ONE 16-byte load from each buffer and one 16-byte store (WIDE, when every row of both buffers
// starts on a 16-byte boundary: combine_vec_words, mask_combine.hpp), else one word; a row of odd W ends in a one-word unit, so that the
// padding word behind it is not touched.  Neighbouring lanes take neighbouring units of a row and run on into the next row.  The grid is
// bounded (kCombineMaxGrid) and every lane strides over the units by the grid's size, TWO units per iteration, one stride apart: the four
// loads of both are issued before either store, which doubles the bytes a wave has in flight (3 - 5 % at a cache-resident mask, 7 % on the
// 8-byte path at HBM size, nothing on the 16-byte path there: DESIGN.md section 4).  The (row, column) of a lane's next unit follows from the previous one by an add and a carry (CombineLaunch::drow / dcol,
// drow2 / dcol2), so the loop divides nothing.
// Rows are counted in 64 bits and offsets are 64-bit: p * pitch words may exceed 2^32 (a 4.39 GB mask is a supported size).
//
// Plain stores: the combined mask is read next by a pick or by the next combining call, usually from the same XCD's L2 when it is small;
// a non-temporal store would need a measurement to replace them (tools/mask_combine_cost.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mask_combine.hpp"

namespace ksched {

struct CombineArgs {
    uint32_t p, W, pitch;    // rows, words per row that are combined, words between consecutive rows (of dst and of src)
    uint32_t units_per_row;  // ceil(W / 2) WIDE, else W
    uint32_t drow, dcol;     // one grid stride (grid * block units) as rows and columns: from a lane's first unit to its second
    uint32_t drow2, dcol2;   // two strides: a lane's step from one iteration to the next
    uint64_t valid;          // valid_bits_word(n)
};

typedef uint64_t combine_u64x2 __attribute__((ext_vector_type(2)));

template <CombineOp OP>
__device__ __forceinline__ uint64_t combine_apply(uint64_t d, uint64_t s) {
    if (OP == CombineOp::kAnd) return d & s;
    if (OP == CombineOp::kOr) return d | s;
    return d & ~s;
}

// one unit of a row: where it starts, and whether it is two words (WIDE and both words are the row's own) or one
struct CombineUnit {
    size_t off;
    uint32_t w0;
    bool pair;
};
template <bool WIDE>
__device__ __forceinline__ CombineUnit combine_unit(uint64_t row, uint32_t col, const CombineArgs &a) {
    const uint32_t w0 = WIDE ? 2u * col : col;  // w0 < W: col < units_per_row
    return CombineUnit{(size_t)row * a.pitch + w0, w0, WIDE && w0 + 1u < a.W};
}
__device__ __forceinline__ void combine_load(const uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, const CombineUnit &u, combine_u64x2 &d,
                                             combine_u64x2 &s) {
    if (u.pair) {
        d = *reinterpret_cast<const combine_u64x2 *>(dst + u.off);
        s = *reinterpret_cast<const combine_u64x2 *>(src + u.off);
    } else {
        d.x = dst[u.off];
        s.x = src[u.off];
        d.y = s.y = 0;
    }
}
template <CombineOp OP>
__device__ __forceinline__ void combine_store(uint64_t *__restrict__ dst, const CombineUnit &u, combine_u64x2 d, combine_u64x2 s, const CombineArgs &a) {
    const uint32_t last = a.W - 1u;
    d.x = combine_apply<OP>(d.x, s.x);
    if (u.w0 == last) d.x &= a.valid;
    if (u.pair) {
        d.y = combine_apply<OP>(d.y, s.y);
        if (u.w0 + 1u == last) d.y &= a.valid;
        *reinterpret_cast<combine_u64x2 *>(dst + u.off) = d;
    } else {
        dst[u.off] = d.x;
    }
}
__device__ __forceinline__ void combine_advance(uint64_t &row, uint32_t &col, uint32_t drow, uint32_t dcol, uint32_t units_per_row) {
    row += drow;
    col += dcol;  // (both below units_per_row <= 2^26)
    if (col >= units_per_row) {
        col -= units_per_row;
        ++row;
    }
}

// launched with plan_combine_launch's grid of kCombineBlock threads; p >= 1, W >= 1, pitch >= W
template <CombineOp OP, bool WIDE>
__global__ __launch_bounds__(kCombineBlock) void k_mask_combine(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, CombineArgs a) {
    const uint32_t t = blockIdx.x * kCombineBlock + threadIdx.x;  // (grid * block <= 2^19)
    uint64_t row0 = t / a.units_per_row, row1 = row0;
    uint32_t col0 = t - (uint32_t)row0 * a.units_per_row, col1 = col0;
    combine_advance(row1, col1, a.drow, a.dcol, a.units_per_row);  // the lane's second unit: one stride on (rows only grow: row1 >= row0)
    while (row0 < a.p) {
        const bool two = row1 < a.p;
        const CombineUnit u0 = combine_unit<WIDE>(row0, col0, a), u1 = combine_unit<WIDE>(row1, col1, a);
        combine_u64x2 d0, s0, d1, s1;
        combine_load(dst, src, u0, d0, s0);
        if (two) combine_load(dst, src, u1, d1, s1);  // in flight together with the first unit's, before either store
        combine_store<OP>(dst, u0, d0, s0, a);
        if (two) combine_store<OP>(dst, u1, d1, s1, a);
        combine_advance(row0, col0, a.drow2, a.dcol2, a.units_per_row);
        combine_advance(row1, col1, a.drow2, a.dcol2, a.units_per_row);
    }
}

template <CombineOp OP>
inline void launch_mask_combine(uint64_t *dst, const uint64_t *src, const CombineLaunch &l, const CombineArgs &a, hipStream_t s) {
    if (l.vec == 2) hipLaunchKernelGGL((k_mask_combine<OP, true>), dim3(l.grid), dim3(l.block), 0, s, dst, src, a);
    else hipLaunchKernelGGL((k_mask_combine<OP, false>), dim3(l.grid), dim3(l.block), 0, s, dst, src, a);
}

// dst = dst OP src over [p] rows of W = ceil(n / 64) words, `pitch` words apart in both buffers, enqueued on `s`: the access width and the
// geometry are mask_combine.hpp's.  The one launch path (ksched_api.hip's launch_mask; tools/mask_combine_bench.hip times the same call).
inline hipError_t run_mask_combine(CombineOp op, uint64_t *dst, const uint64_t *src, uint32_t p, uint32_t n, uint32_t W, uint32_t pitch, hipStream_t s) {
    const CombineLaunch l = plan_combine_launch(p, W, combine_vec_words((uint64_t)(uintptr_t)dst, (uint64_t)(uintptr_t)src, pitch));
    if (l.grid == 0) return hipSuccess;
    const CombineArgs a{p, W, pitch, l.units_per_row, l.drow, l.dcol, l.drow2, l.dcol2, valid_bits_word(n)};
    switch (op) {
        case CombineOp::kAnd: launch_mask_combine<CombineOp::kAnd>(dst, src, l, a, s); break;
        case CombineOp::kOr: launch_mask_combine<CombineOp::kOr>(dst, src, l, a, s); break;
        case CombineOp::kAndNot: launch_mask_combine<CombineOp::kAndNot>(dst, src, l, a, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ksched
