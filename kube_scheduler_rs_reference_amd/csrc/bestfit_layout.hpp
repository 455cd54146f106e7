// bestfit_layout.hpp -- every number the best-fit structures and launches are sized by: the sample and level arrays of the two
// orders, the row bitmaps in best-fit order, the hand-over buffer of the two-stage pick with its rotating counter sets, and the
// KSCHED_OPT_DEBUG bits the launches read.
//
// Host-only on purpose, like eval_plan.hpp and snapshot_change.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it
// and tests/cpp/bestfit_layout_tests.cpp pins every rule at its boundary without a GPU.  The buffers these layouts size are
// BestfitIndex in ksched_api.hip, which builds them (build_bestfit, build_bestfit_rows) and launches the picks over them
// (launch_bestfit_rows); the kernels are in kernels_build.hpp and kernels_direct.hpp.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "merge_sort_plan.hpp"

namespace ksched {

// The first stage appends the pods it hands over to kBfSublists lists, wave w to list w % kBfSublists: ONE list with one counter made
// 2 000 waves queue for a returning atomic on one address (~8 ns each, up to 10 us of waiting per wave at the C5 shard).
constexpr uint32_t kBfSublists = 128;

// The lane-per-pod searches (k_pick_bestfit_lanes) descend 8-ary level arrays and carry at most kBfMaxLevels of them: level k holds
// the last element of every block of 8^k entries, and the search starts in the at most eight entries above the top level.  Six
// levels therefore cover 8^7 nodes; beyond that the plan keeps best fit to one stage (plan_eval), and a snapshot with list keys,
// which needs the first stage, is unsupported.
constexpr uint32_t kBfMaxLevels = 6;
constexpr uint32_t kBfLanesMaxNodes = 1u << 21;
constexpr uint64_t bf_pow8(uint32_t k) { return k ? 8u * bf_pow8(k - 1u) : 1u; }
static_assert(kBfLanesMaxNodes == bf_pow8(kBfMaxLevels + 1u), "six levels and the eight entries above them cover 8^7 nodes");

// ---- the two orders (build_bestfit) ---------------------------------------------------------------------------------------
// Sample arrays of bf_mem and cpu_sorted for the wave-per-pod searches (wave_lower_bound_sampled): s1 = last element of every block of
// 64, s2 = of every block of 4096, in one buffer [mem s1][mem s2][cpu s1][cpu s2].  Level arrays for the lane-per-pod searches, in one
// buffer of two halves [mem level 1][mem level 2]...[cpu level 1]...; lvl_off[k - 1] = offset of level k inside one half.
struct BfOrderLayout {
    uint32_t n1 = 0, n2 = 0;  // entries of s1, s2
    bool sampled = false;     // the sampled searches apply: three rounds of 64 cover the array
    uint32_t nlev = 0, lvl_off[kBfMaxLevels] = {}, lvl_half = 0;
    uint32_t merge_passes = 0;  // merge passes of each sort behind the runs of 1024 (merge_sort_plan.hpp)

    size_t sample_elems() const { return 2 * (size_t)(n1 + n2); }
    size_t level_elems() const { return 2 * (size_t)lvl_half + 8; }
    // where the sample arrays behind the first start inside the sample buffer
    size_t mem_s2() const { return n1; }
    size_t cpu_s1() const { return (size_t)n1 + n2; }
    size_t cpu_s2() const { return 2 * (size_t)n1 + n2; }
};

inline BfOrderLayout bf_order_layout(uint32_t n) {
    BfOrderLayout l;
    l.n1 = (n + 63u) / 64u;
    l.n2 = (n + 4095u) / 4096u;
    l.sampled = n <= 64u * 64u * 64u;
    // 8-ary level arrays: level k = last element of every block of 8^k entries
    uint32_t nk = n, off = 0;
    while (nk > 8u && l.nlev < kBfMaxLevels) {
        nk = (nk + 7u) / 8u;
        l.lvl_off[l.nlev++] = off;
        off += (nk + 7u) & ~7u;  // every level starts on a 64-byte boundary and may be read in whole blocks of eight
    }
    l.lvl_half = off;
    l.merge_passes = merge_passes(n);
    return l;
}

// what ksched_set_nodes reserves of bf_mem and cpu_sorted (+8: the 8-ary searches read whole blocks of eight)
inline size_t bf_searched_elems(uint32_t n) { return (size_t)n + 8; }

// ---- the row bitmaps in best-fit order (build_bestfit_rows) ---------------------------------------------------------------
// The bitmap index's named rows (`row_cpu` of them: valid, taint, label) once more over best-fit positions, then 256 + 1 cpu
// threshold rows, row[t] = {i : cpurank[i] >= t * q}.
struct BfRowLayout {
    uint32_t Wbf = 0;     // words of a row, padded to whole 64-byte lines: k_pick_bestfit_lanes reads aligned blocks of 8 words
    uint32_t levels = 256, q = 1;
    uint32_t row_cpu0 = 0;  // the first threshold row = the number of named rows
    uint32_t rows = 0;
    size_t words() const { return (size_t)rows * Wbf; }
};

inline BfRowLayout bf_row_layout(uint32_t n, uint32_t row_cpu) {
    BfRowLayout l;
    l.Wbf = ((n + 63u) / 64u + 7u) & ~7u;
    l.q = (n + l.levels - 1u) / l.levels;
    l.row_cpu0 = row_cpu;
    l.rows = row_cpu + l.levels + 1u;
    return l;
}

// ---- the hand-over buffer of the two-stage pick (launch_bestfit_rows) -----------------------------------------------------
// uint32 words: [kBfCounterSets sets of kBfSublists counters, one per 128-byte line, in rotation][listed mask: ceil(p / 64) words of 64 bits]
// [64-byte hand-over records: kBfSublists lists of sub_cap slots]; each call zeroes the NEXT call's counters (no memset launch).
// The trace buffer (KSCHED_OPT_DEBUG bit 20) holds uint64 words: 8 per wave of the first stage, then 4 per hand-over slot.
constexpr uint32_t kBfCounterSets = 3;
struct BfHandoverLayout {
    size_t waves1 = 0;    // waves of the first stage's 64 lanes
    size_t sub_cap = 0;   // slots of one sub-list
    size_t ctr_u32 = 0, mask_u32 = 0;
    size_t slots2() const { return (size_t)kBfSublists * sub_cap; }
    size_t mask_off() const { return ctr_u32; }
    size_t rec_off() const { return ctr_u32 + mask_u32; }
    size_t total_u32() const { return ctr_u32 + mask_u32 + 16 * slots2(); }
    size_t ctr_off(uint32_t slot) const { return (size_t)slot * kBfSublists * 32; }
    size_t trace1_u64() const { return waves1 * 8; }
    size_t trace2_u64() const { return slots2() * 4; }
    size_t trace_u64() const { return trace1_u64() + trace2_u64(); }
};

inline BfHandoverLayout bf_handover_layout(uint32_t p) {
    BfHandoverLayout l;
    l.waves1 = ((size_t)p + 63) / 64;
    l.sub_cap = ((l.waves1 + kBfSublists - 1) / kBfSublists) * 64;
    l.ctr_u32 = kBfCounterSets * (size_t)kBfSublists * 32;
    l.mask_u32 = ((l.waves1 * 2 + 15) / 16) * 16;  // (records stay 64-byte aligned)
    return l;
}

// Which counter set a two-stage call uses.  The call before zeroed it (its first-stage kernel zeroes `zero()`); a buffer whose
// capacity is not the one the counters were last zeroed at is a fresh allocation: all counters once, by a memset, and set 0 again.
struct BfRotation {
    size_t zeroed_cap = 0;
    uint32_t slot = 0;
    bool fresh(size_t cap) const { return zeroed_cap != cap; }
    void zeroed(size_t cap) {  // the memset of all counters has been enqueued
        zeroed_cap = cap;
        slot = 0;
    }
    uint32_t use() const { return slot; }
    uint32_t zero() const { return (slot + 1u) % kBfCounterSets; }
    void advance() { slot = zero(); }  // (only once the kernel that zeroes the next set is on its way)
};

// ---- KSCHED_OPT_DEBUG as the best-fit launches read it --------------------------------------------------------------------
struct BfDebug {
    uint32_t lane_blocks = 2;  // bits 12-15: A/B of the hand-over point (in 64-byte blocks of 8 words); 0 = the default, 2
    bool tracing = false;      // bit 20: per-wave time stamps of both stages (tools/bestfit_ab.py --trace)
    uint32_t grid_shift = 2;   // bits 21-22: the second stage's grid covers 1 / 2^k of the lists' capacity, k = 2 by default, A/B 0 / 1 / 3
};

inline BfDebug bf_debug(uint32_t debug) {
    BfDebug d;
    const uint32_t blocks = (debug >> 12) & 15u, g = (debug >> 21) & 3u;
    d.lane_blocks = blocks ? blocks : 2u;
    d.tracing = (debug & 0x100000u) != 0u;
    d.grid_shift = g == 0u ? 2u : g == 1u ? 0u : g == 2u ? 1u : 3u;
    return d;
}

// blocks of the second stage (k_pick_bestfit_handed): one wave per block, block b takes entries b / kBfSublists, + stride, ... of sub-list b % kBfSublists
inline uint32_t bf_handed_grid(size_t sub_cap, uint32_t grid_shift) { return kBfSublists * std::max<uint32_t>(1u, (uint32_t)sub_cap >> grid_shift); }

}  // namespace ksched
