// tile_launch.hpp -- one launch of a tile kernel (k_eval_fused, k_summarize_indexed) over the per-tile bitmap index, described
// once: which predicate terms are active, how a block's LDS is carved up, the launch geometry, the kernel arguments the two
// kernels share, and the dispatch over the predicate instantiations.
//
// Host-only in the sense of eval_plan.hpp: no kernel and no ksched_ctx, so tests/cpp/tile_launch_tests.cpp compiles it with plain
// g++ (the way tests/cpp/index_tests does: the HIP headers are only read for their types) and pins every rule at its boundary
// without a GPU.  run_fused (kernels_fused.hpp) and run_summary_indexed (kernels_summary.hpp) take their numbers from here; the
// measured rules of the launch geometry live here, with their measurements.
#pragma once

#include <algorithm>
#include <type_traits>

#include "eval_request.hpp"
#include "tile_index.hpp"

//   KSCHED_FUSED_THREADS threads per block (waves x 64) of the tile kernels (a build-time variant: tools/build_variants.sh)
#ifndef KSCHED_FUSED_THREADS
#define KSCHED_FUSED_THREADS 1024
#endif

namespace ksched {

constexpr uint32_t kFusedThreads = KSCHED_FUSED_THREADS;
constexpr uint32_t kFusedWaves = kFusedThreads / 64;

// ---- the request's terms over an index layout ---------------------------------------------------------------------------
// Which predicates a tile kernel evaluates: EvalRequest's derived terms (eval_request.hpp) against the layout's label keys, taint
// groups (not the snapshot's have_taints) and list keys.
struct TileTerms {
    bool fit, sel, taint;
    bool list;      // the selector term runs over a snapshot with list keys: the LIST instantiations
    bool want_fit;  // a second, fit-only mask is written
};

inline TileTerms tile_terms(const EvalRequest &r, const IndexedLayout &l) {
    const bool sel = r.sel(l.nkeys);
    return TileTerms{r.fit(), sel, r.taint(l.ngroups != 0), sel && l.nlist > 0, r.want_fit()};
}

// ---- LDS carve-up ---------------------------------------------------------------------------------------------------------
// [rows * 128 : bitmap rows][aux block: 2 search trees + 2 cnt tables (fit)]
// per wave x 64 pods: [16 B fit record (fit)][16 B label rows 1..8 (sel)][8 B taint rows (taint)]
// [nlist * 6 KiB: the tile's list keys][per wave x 64 pods: 8 B list record]   (sel, snapshots with list keys only)
// [the tile-test pick's park of the round's draws][the operand prefetch's dump area]
constexpr uint32_t kLdsFit = 1u, kLdsSel = 2u, kLdsTaint = 4u;
constexpr uint32_t kLdsPark = 8u;      // the per-wave park of the tile-test pick (PICK == 2)
constexpr uint32_t kLdsPrefetch = 16u; // the operand prefetch's dump area: only where it still fits (it never decides whether a kernel applies)
// The summary kernel takes every record region whatever the predicates (a pod's fit and label records take its lanes' packed
// counts afterwards), no park and no prefetch.
constexpr uint32_t kLdsEveryRegion = kLdsFit | kLdsSel | kLdsTaint;

constexpr uint32_t kPickAttempts = 5;  // draws per pod the tile-test pick (PICK == 2) handles: ATTEMPTS of src/main.rs:49
constexpr uint32_t kPickParkBytes = kFusedWaves * kPickAttempts * 64u * 4u;
constexpr uint32_t kPrefetchDumpBytes = 256u;  // one dword per lane: where the operand prefetch's LDS-DMA loads land (shared by the block's waves: nobody reads it)

struct TileLds {
    uint32_t off_aux, off_fit, off_lab, off_trow, off_list, off_lrec, off_park;
    uint32_t off_pf;  // or 0xFFFFFFFF: no room, no prefetch
    uint32_t bytes;
};

constexpr uint32_t lds_want(const TileTerms &t, bool park) {
    return (t.fit ? kLdsFit : 0u) | (t.sel ? kLdsSel : 0u) | (t.taint ? kLdsTaint : 0u) | (park ? kLdsPark : 0u) | kLdsPrefetch;
}

constexpr TileLds tile_lds_layout(const IndexedLayout &l, uint32_t want) {
    constexpr uint32_t pods = kFusedWaves * 64u;  // a record per wave and pod of its round
    const bool lists = (want & kLdsSel) && l.nlist;
    uint32_t off = l.rows * 128u;
    auto take = [&off](bool on, uint32_t bytes) {  // -> where the region starts; it takes no room when it is not wanted
        const uint32_t at = off;
        if (on) off += bytes;
        return at;
    };
    TileLds d{};
    d.off_aux = take(want & kLdsFit, kAuxWords * 8u);
    d.off_fit = take(want & kLdsFit, pods * 16u);
    d.off_lab = take(want & kLdsSel, pods * 16u);
    d.off_trow = take(want & kLdsTaint, pods * 8u);
    d.off_list = take(lists, l.nlist * kListBytes);
    d.off_lrec = take(lists, pods * kListRecBytes);
    d.off_park = take(want & kLdsPark, kPickParkBytes);
    d.off_pf = (want & kLdsPrefetch) && off + kPrefetchDumpBytes <= kLdsBudget ? take(true, kPrefetchDumpBytes) : 0xFFFFFFFFu;
    d.bytes = off;
    return d;
}

// indexed_plan (tile_index.hpp) admits a layout when its rows plus lds_non_row_bytes(nlist) fit the budget: that is every region
// of this carve-up, so every indexed snapshot's summary -- and every fused form without the park -- fits.
constexpr bool lds_is_what_indexed_plan_checks(uint32_t nlist) {
    IndexedLayout l{};
    l.nlist = nlist;
    return tile_lds_layout(l, kLdsEveryRegion).bytes == lds_non_row_bytes(nlist);
}
static_assert(lds_is_what_indexed_plan_checks(0) && lds_is_what_indexed_plan_checks(1) && lds_is_what_indexed_plan_checks(kMaxListKeys),
              "tile_lds_layout and indexed_plan's LDS budget have drifted apart");

// ---- launch geometry ------------------------------------------------------------------------------------------------------
// Work split of the fused kernel: the unit is 8 pods (one phase-2 instruction).  Units are cut evenly into `chunks` pod ranges;
// the (chunk, tile) blocks are dealt to the 8 XCDs in contiguous chunk-major runs of `run` blocks.
// blocks of kFusedThreads threads a compute unit holds at once: by LDS, and by its 2048 thread slots
inline uint32_t resident_blocks_per_cu(uint32_t lds) { return std::max(1u, std::min(kLdsBudget / lds, 2048u / kFusedThreads)); }

struct FusedGeometryIn {
    uint32_t p = 0, tiles = 1;
    uint32_t lds = 0;       // tile_lds_layout(...).bytes (the tile-test pick's park included: the pick's form enters through it)
    bool pick = false;      // a sampled pick rides in the launch, in either form
    uint32_t grid_cus = 0;  // KSCHED_OPT_GRID_CUS
    int round_order = 0;    // KSCHED_OPT_ROUND_ORDER: 0 = interleaved, wave-major (default); 1 = blocked; 2 = interleaved, chunk-major
    uint32_t debug = 0;     // KSCHED_OPT_DEBUG: bits 5, 18-19 and 31
};

struct FusedGeometry {
    uint32_t units, chunks, unit_q, unit_rem;  // ceil(p / 8), pod ranges, units / chunks, units % chunks
    uint32_t u_stride, wave_major;             // FusedArgs
    uint32_t tiles_rcp, run, grid;             // floor(2^32 / tiles), (chunk, tile) pairs per XCD, blocks
    uint32_t pick_ppb, pick_waves;             // a riding pick: pods one block carries, and how many of its waves carry them
};

inline FusedGeometry fused_geometry(const FusedGeometryIn &in) {
    FusedGeometry g{};
    g.units = (in.p + 7u) / 8u;
    // chunks: as many pod ranges as keep every block resident at once (256 CUs x blocks per CU), but no
    // more than one round (64 pods) per wave needs.
    const uint32_t blocks_per_cu = resident_blocks_per_cu(in.lds);
    const uint32_t rounds = (g.units + 7u) / 8u;
    // chunks that give every wave one round; small batches whose pick rides along are cut finer (a block's time is its fill plus
    // ONE round either way, and the pick's pods spread over more CUs).  debug bits 18-19: A/B of that divisor (0: default).
    uint32_t per_block = kFusedWaves;
    if (in.pick) per_block = 4u;
    if (((in.debug >> 18) & 3u) == 1u) per_block = kFusedWaves;
    if (((in.debug >> 18) & 3u) == 2u) per_block = 4u;
    if (((in.debug >> 18) & 3u) == 3u) per_block = 1u;
    const uint32_t want = (rounds + per_block - 1u) / per_block;
    // grid_cus (KSCHED_OPT_GRID_CUS): the launch keeps to that many compute units, so that the launches of the FOLLOWING batches
    // (other streams) find free ones and fill while this one stores; 0 = the whole chip
    const uint32_t cus = in.grid_cus ? std::min(256u, in.grid_cus) : 256u;
    g.chunks = std::max(1u, std::min((cus * blocks_per_cu) / in.tiles, want));
    // Interleaved orders, launches of TWO rounds per wave (C3: 1 563 rounds over 51 x 16 waves): the launch lasts as long as its two-round waves, and
    // at the largest resident chunk count one wave in twelve has only one -- the smallest chunk count that still needs no third round (49: 784 waves x 2
    // rounds) fills fewer blocks for the same two rounds: step 18.05 -> 17.6 us (sweep of 44 .. 51 chunks, session r7i: 18.43 18.25 17.94 17.91 17.77
    // 17.6 17.8 18.05).  Longer launches are bound by their stores, not by the quantisation, and want every compute unit (session r7k, even / largest
    // chunk count: 150 k pods 23.5 / 23.3 us, 300 k 43.3 / 40.0, 400 k 55.7 / 52.4); one-round launches keep the finer cut (a riding pick's pods spread
    // wider).  profiles/r06_r7i_r7k_chunk_count.txt
    if (in.round_order != 1 && !(in.debug & 0x80000000u)) {  // (debug bit 31: the largest resident chunk count, the A/B of this rule)
        const uint32_t streams = g.chunks * kFusedWaves;
        const uint32_t per_wave = (rounds + streams - 1u) / streams;
        if (per_wave == 2u) g.chunks = std::max(1u, std::min(g.chunks, (rounds + 2u * kFusedWaves - 1u) / (2u * kFusedWaves)));
    }
    g.unit_q = g.units / g.chunks;
    g.unit_rem = g.units % g.chunks;
    // units between a wave's consecutive rounds: 8 = every wave owns a contiguous pod range (blocked); chunks * waves * 8 = the
    // launch's rounds are dealt round-robin over its (chunk, wave) streams (interleaved: the chip writes ONE moving window)
    g.u_stride = in.round_order == 1 ? 8u : g.chunks * kFusedWaves * 8u;
    g.wave_major = in.round_order == 2 ? 0u : 1u;
    g.tiles_rcp = (uint32_t)std::min<uint64_t>((1ull << 32) / in.tiles, 0xFFFFFFFFull);
    const uint32_t total = g.chunks * in.tiles;
    g.run = (total + 7u) / 8u;
    g.grid = (in.debug & 32u) ? total : g.run * 8u;  // (debug bit 5: no padding to whole runs)
    if (in.pick) {
        g.pick_ppb = (in.p + total - 1u) / total;
        g.pick_waves = std::max(1u, std::min(8u, (g.pick_ppb + 63u) / 64u));
    }
    return g;
}

struct SummaryGeometry {
    uint32_t rounds, chunks, grid;  // rounds of 64 pods in the batch, blocks per tile, blocks
};

// blocks per tile: as many as the chip holds at once (a block fills a compute unit's LDS), no more than one round per wave needs
inline SummaryGeometry summary_geometry(uint32_t p, uint32_t tiles, uint32_t lds) {
    SummaryGeometry g{};
    g.rounds = (p + 63u) / 64u;
    g.chunks = std::max(1u, std::min((256u * resident_blocks_per_cu(lds)) / tiles, (g.rounds + kFusedWaves - 1u) / kFusedWaves));
    g.grid = g.chunks * tiles;
    return g;
}

// ---- the kernel arguments both tile kernels take (FusedArgs, SummaryArgs: the same-named members) ---------------------------
template <class Args>
inline void fill_tile_args(Args &a, const IndexedSnapshot &s, const TileLds &d, const TileTerms &t, const EvalRequest &r) {
    const IndexedLayout &l = s.lay;
    a.p = r.p;
    a.tiles = l.tiles;
    a.rows = l.rows;
    a.nkeys = l.nkeys;
    a.ngroups = l.ngroups;
    a.row_zero = l.row_zero;
    a.row_valid = l.row_valid;
    a.row_cpu = l.row_cpu;
    a.row_taint = l.row_taint;
    for (int k = 0; k < 8; ++k) {
        const bool is_list = l.lab_base[k] == kLabList;  // no rows: phase 1 skips the column (list_mask8)
        a.lab_off[k] = is_list ? 0u : (l.lab_base[k] - 1u) * 128u;  // id s -> row lab_base + s - 1 (ids start at 1; keys without rows never match s != 0 below nkeys)
        a.lab_mx1[k] = is_list ? 0u : l.lab_max[k] + 1u;
    }
    a.lab_meta = s.d_lab_meta;
    a.zero64 = reinterpret_cast<const uint64_t *>(s.d_lab_meta + 64);
    a.off_aux = d.off_aux;
    a.off_fit = d.off_fit;
    a.off_lab = d.off_lab;
    a.off_trow = d.off_trow;
    a.off_list = d.off_list;
    a.off_lrec = d.off_lrec;
    a.nlist = t.list ? l.nlist : 0u;
    a.list_mask8 = 0;
    for (uint32_t j = 0; j < a.nlist; ++j) {
        a.list_col[j] = l.list_col[j];
        if (l.list_col[j] < 8u) a.list_mask8 |= 1u << l.list_col[j];
    }
    a.has_tol = r.ptol != nullptr ? 1u : 0u;
}

// ---- dispatch over the predicate instantiations ---------------------------------------------------------------------------
// f(fit, sel, taint) with the three as std::integral_constant<bool, ...>: decltype(fit)::value is a template argument
template <class F>
inline auto with_predicates(bool fit, bool sel, bool taint, F &&f) {
    auto on = [](bool b, auto &&g) { return !b ? g(std::false_type{}) : g(std::true_type{}); };
    return on(fit, [&](auto F_) { return on(sel, [&](auto S_) { return on(taint, [&](auto T_) { return f(F_, S_, T_); }); }); });
}

}  // namespace ksched
