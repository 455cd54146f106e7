// tile_launch_tests.cpp -- host-side check of the launch description of the tile kernels (csrc/tile_launch.hpp), no GPU: the LDS
// carve-up, the launch geometry of k_eval_fused and k_summarize_indexed with every measured rule at its boundary, the shared
// argument fill and the predicate dispatcher.  Every expected value is a literal, printed once by the functions the launchers had
// before the description existed (fused_lds_bytes, summary_lds_bytes, the arithmetic inside run_fused / run_summary_indexed) --
// none is computed by the code under test.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/tile_launch.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

// ---- the LDS carve-up -----------------------------------------------------------------------------------------------------
struct LdsRow {
    int fit, sel, taint, park;
    uint32_t off_aux, off_fit, off_lab, off_trow, off_list, off_lrec, off_park, off_pf, bytes;
};
struct LdsCase {
    const char *name;
    uint32_t n, nkeys;
    std::vector<uint32_t> lab_max;
    uint64_t taints;
    uint32_t rows, nlist, ngroups;
    LdsRow fused[16];
    uint32_t summary[7];  // off_aux, off_fit, off_lab, off_trow, off_list, off_lrec, bytes
};

static const LdsCase kLdsCases[] = {
    {"C3", 5000, 8, {2, 3, 4, 8, 16, 32, 64, 128}, 0, 525, 0, 0,
     {{0, 0, 0, 0, 67200u, 67200u, 67200u, 67200u, 67200u, 67200u, 67200u, 0x10680u, 67456u},
      {1, 0, 0, 0, 67200u, 100000u, 116384u, 116384u, 116384u, 116384u, 116384u, 0x1C6A0u, 116640u},
      {0, 1, 0, 0, 67200u, 67200u, 67200u, 83584u, 83584u, 83584u, 83584u, 0x14680u, 83840u},
      {1, 1, 0, 0, 67200u, 100000u, 116384u, 132768u, 132768u, 132768u, 132768u, 0x206A0u, 133024u},
      {0, 0, 1, 0, 67200u, 67200u, 67200u, 67200u, 75392u, 75392u, 75392u, 0x12680u, 75648u},
      {1, 0, 1, 0, 67200u, 100000u, 116384u, 116384u, 124576u, 124576u, 124576u, 0x1E6A0u, 124832u},
      {0, 1, 1, 0, 67200u, 67200u, 67200u, 83584u, 91776u, 91776u, 91776u, 0x16680u, 92032u},
      {1, 1, 1, 0, 67200u, 100000u, 116384u, 132768u, 140960u, 140960u, 140960u, 0x226A0u, 141216u},
      {0, 0, 0, 1, 67200u, 67200u, 67200u, 67200u, 67200u, 67200u, 67200u, 0x15680u, 87936u},
      {1, 0, 0, 1, 67200u, 100000u, 116384u, 116384u, 116384u, 116384u, 116384u, 0x216A0u, 137120u},
      {0, 1, 0, 1, 67200u, 67200u, 67200u, 83584u, 83584u, 83584u, 83584u, 0x19680u, 104320u},
      {1, 1, 0, 1, 67200u, 100000u, 116384u, 132768u, 132768u, 132768u, 132768u, 0x256A0u, 153504u},
      {0, 0, 1, 1, 67200u, 67200u, 67200u, 67200u, 75392u, 75392u, 75392u, 0x17680u, 96128u},
      {1, 0, 1, 1, 67200u, 100000u, 116384u, 116384u, 124576u, 124576u, 124576u, 0x236A0u, 145312u},
      {0, 1, 1, 1, 67200u, 67200u, 67200u, 83584u, 91776u, 91776u, 91776u, 0x1B680u, 112512u},
      {1, 1, 1, 1, 67200u, 100000u, 116384u, 132768u, 140960u, 140960u, 140960u, 0x276A0u, 161696u}},
     {67200u, 100000u, 116384u, 132768u, 140960u, 140960u, 140960u}},
    // two hostname-like keys become lists; with every region and the park the prefetch dump no longer fits
    {"two list keys", 5000, 8, {2, 3, 4, 5000, 16, 32, 64, 4000}, 0x7, 403, 2, 1,
     {{0, 0, 0, 0, 51584u, 51584u, 51584u, 51584u, 51584u, 51584u, 51584u, 0xC980u, 51840u},
      {1, 0, 0, 0, 51584u, 84384u, 100768u, 100768u, 100768u, 100768u, 100768u, 0x189A0u, 101024u},
      {0, 1, 0, 0, 51584u, 51584u, 51584u, 67968u, 67968u, 80256u, 88448u, 0x15980u, 88704u},
      {1, 1, 0, 0, 51584u, 84384u, 100768u, 117152u, 117152u, 129440u, 137632u, 0x219A0u, 137888u},
      {0, 0, 1, 0, 51584u, 51584u, 51584u, 51584u, 59776u, 59776u, 59776u, 0xE980u, 60032u},
      {1, 0, 1, 0, 51584u, 84384u, 100768u, 100768u, 108960u, 108960u, 108960u, 0x1A9A0u, 109216u},
      {0, 1, 1, 0, 51584u, 51584u, 51584u, 67968u, 76160u, 88448u, 96640u, 0x17980u, 96896u},
      {1, 1, 1, 0, 51584u, 84384u, 100768u, 117152u, 125344u, 137632u, 145824u, 0x239A0u, 146080u},
      {0, 0, 0, 1, 51584u, 51584u, 51584u, 51584u, 51584u, 51584u, 51584u, 0x11980u, 72320u},
      {1, 0, 0, 1, 51584u, 84384u, 100768u, 100768u, 100768u, 100768u, 100768u, 0x1D9A0u, 121504u},
      {0, 1, 0, 1, 51584u, 51584u, 51584u, 67968u, 67968u, 80256u, 88448u, 0x1A980u, 109184u},
      {1, 1, 0, 1, 51584u, 84384u, 100768u, 117152u, 117152u, 129440u, 137632u, 0x269A0u, 158368u},
      {0, 0, 1, 1, 51584u, 51584u, 51584u, 51584u, 59776u, 59776u, 59776u, 0x13980u, 80512u},
      {1, 0, 1, 1, 51584u, 84384u, 100768u, 100768u, 108960u, 108960u, 108960u, 0x1F9A0u, 129696u},
      {0, 1, 1, 1, 51584u, 51584u, 51584u, 67968u, 76160u, 88448u, 96640u, 0x1C980u, 117376u},
      {1, 1, 1, 1, 51584u, 84384u, 100768u, 117152u, 125344u, 137632u, 145824u, 0xFFFFFFFFu, 166304u}},
     {51584u, 84384u, 100768u, 117152u, 125344u, 137632u, 145824u}},
    {"ten taint groups", 3000, 3, {5, 7, 2}, 1ull << 39, 437, 0, 10,
     {{0, 0, 0, 0, 55936u, 55936u, 55936u, 55936u, 55936u, 55936u, 55936u, 0xDA80u, 56192u},
      {1, 0, 0, 0, 55936u, 88736u, 105120u, 105120u, 105120u, 105120u, 105120u, 0x19AA0u, 105376u},
      {0, 1, 0, 0, 55936u, 55936u, 55936u, 72320u, 72320u, 72320u, 72320u, 0x11A80u, 72576u},
      {1, 1, 0, 0, 55936u, 88736u, 105120u, 121504u, 121504u, 121504u, 121504u, 0x1DAA0u, 121760u},
      {0, 0, 1, 0, 55936u, 55936u, 55936u, 55936u, 64128u, 64128u, 64128u, 0xFA80u, 64384u},
      {1, 0, 1, 0, 55936u, 88736u, 105120u, 105120u, 113312u, 113312u, 113312u, 0x1BAA0u, 113568u},
      {0, 1, 1, 0, 55936u, 55936u, 55936u, 72320u, 80512u, 80512u, 80512u, 0x13A80u, 80768u},
      {1, 1, 1, 0, 55936u, 88736u, 105120u, 121504u, 129696u, 129696u, 129696u, 0x1FAA0u, 129952u},
      {0, 0, 0, 1, 55936u, 55936u, 55936u, 55936u, 55936u, 55936u, 55936u, 0x12A80u, 76672u},
      {1, 0, 0, 1, 55936u, 88736u, 105120u, 105120u, 105120u, 105120u, 105120u, 0x1EAA0u, 125856u},
      {0, 1, 0, 1, 55936u, 55936u, 55936u, 72320u, 72320u, 72320u, 72320u, 0x16A80u, 93056u},
      {1, 1, 0, 1, 55936u, 88736u, 105120u, 121504u, 121504u, 121504u, 121504u, 0x22AA0u, 142240u},
      {0, 0, 1, 1, 55936u, 55936u, 55936u, 55936u, 64128u, 64128u, 64128u, 0x14A80u, 84864u},
      {1, 0, 1, 1, 55936u, 88736u, 105120u, 105120u, 113312u, 113312u, 113312u, 0x20AA0u, 134048u},
      {0, 1, 1, 1, 55936u, 55936u, 55936u, 72320u, 80512u, 80512u, 80512u, 0x18A80u, 101248u},
      {1, 1, 1, 1, 55936u, 88736u, 105120u, 121504u, 129696u, 129696u, 129696u, 0x24AA0u, 150432u}},
     {55936u, 88736u, 105120u, 121504u, 129696u, 129696u, 129696u}},
    // the largest layout indexed_plan admits here: with every region 96 bytes stay free, fewer than the prefetch dump's 256 --
    // no dump (off_pf = 0xFFFFFFFF), the total as without it, and the forms with the park exceed the budget
    {"96 bytes free", 2000, 1, {426}, 0x1, 703, 0, 1,
     {{0, 0, 0, 0, 89984u, 89984u, 89984u, 89984u, 89984u, 89984u, 89984u, 0x15F80u, 90240u},
      {1, 0, 0, 0, 89984u, 122784u, 139168u, 139168u, 139168u, 139168u, 139168u, 0x21FA0u, 139424u},
      {0, 1, 0, 0, 89984u, 89984u, 89984u, 106368u, 106368u, 106368u, 106368u, 0x19F80u, 106624u},
      {1, 1, 0, 0, 89984u, 122784u, 139168u, 155552u, 155552u, 155552u, 155552u, 0x25FA0u, 155808u},
      {0, 0, 1, 0, 89984u, 89984u, 89984u, 89984u, 98176u, 98176u, 98176u, 0x17F80u, 98432u},
      {1, 0, 1, 0, 89984u, 122784u, 139168u, 139168u, 147360u, 147360u, 147360u, 0x23FA0u, 147616u},
      {0, 1, 1, 0, 89984u, 89984u, 89984u, 106368u, 114560u, 114560u, 114560u, 0x1BF80u, 114816u},
      {1, 1, 1, 0, 89984u, 122784u, 139168u, 155552u, 163744u, 163744u, 163744u, 0xFFFFFFFFu, 163744u},
      {0, 0, 0, 1, 89984u, 89984u, 89984u, 89984u, 89984u, 89984u, 89984u, 0x1AF80u, 110720u},
      {1, 0, 0, 1, 89984u, 122784u, 139168u, 139168u, 139168u, 139168u, 139168u, 0x26FA0u, 159904u},
      {0, 1, 0, 1, 89984u, 89984u, 89984u, 106368u, 106368u, 106368u, 106368u, 0x1EF80u, 127104u},
      {1, 1, 0, 1, 89984u, 122784u, 139168u, 155552u, 155552u, 155552u, 155552u, 0xFFFFFFFFu, 176032u},
      {0, 0, 1, 1, 89984u, 89984u, 89984u, 89984u, 98176u, 98176u, 98176u, 0x1CF80u, 118912u},
      {1, 0, 1, 1, 89984u, 122784u, 139168u, 139168u, 147360u, 147360u, 147360u, 0xFFFFFFFFu, 167840u},
      {0, 1, 1, 1, 89984u, 89984u, 89984u, 106368u, 114560u, 114560u, 114560u, 0x20F80u, 135296u},
      {1, 1, 1, 1, 89984u, 122784u, 139168u, 155552u, 163744u, 163744u, 163744u, 0xFFFFFFFFu, 184224u}},
     {89984u, 122784u, 139168u, 155552u, 163744u, 163744u, 163744u}},
};

static void test_lds_layout() {
    for (const LdsCase &c : kLdsCases) {
        IndexedLayout l;
        const char *why = "";
        CHECK(indexed_plan(l, c.n, c.nkeys, c.lab_max.data(), c.taints, &why));
        CHECK(l.rows == c.rows && l.nlist == c.nlist && l.ngroups == c.ngroups);
        for (const LdsRow &e : c.fused) {
            const TileTerms t{e.fit != 0, e.sel != 0, e.taint != 0, false, false};
            const TileLds d = tile_lds_layout(l, lds_want(t, e.park != 0));
            const bool same = d.off_aux == e.off_aux && d.off_fit == e.off_fit && d.off_lab == e.off_lab && d.off_trow == e.off_trow &&
                              d.off_list == e.off_list && d.off_lrec == e.off_lrec && d.off_park == e.off_park && d.off_pf == e.off_pf &&
                              d.bytes == e.bytes;
            if (!same) std::printf("  %s: fit %d sel %d taint %d park %d\n", c.name, e.fit, e.sel, e.taint, e.park);
            CHECK(same);
        }
        const TileLds d = tile_lds_layout(l, kLdsEveryRegion);
        CHECK(d.off_aux == c.summary[0] && d.off_fit == c.summary[1] && d.off_lab == c.summary[2] && d.off_trow == c.summary[3] &&
              d.off_list == c.summary[4] && d.off_lrec == c.summary[5] && d.bytes == c.summary[6]);
        CHECK(d.off_pf == 0xFFFFFFFFu && d.off_park == d.bytes);  // the summary kernel has neither
    }
    // whatever indexed_plan admits, every region fits: a sweep over node counts, key counts, cardinalities up to one value per
    // node (list keys, and refusals beyond two of them) and taint widths
    uint32_t admitted = 0, refused = 0, with_lists = 0, tight = 0;
    const uint32_t cards[] = {1u, 2u, 7u, 64u, 128u, 300u, 426u, 427u, 442u, 443u, 1000u, 5000u, 50000u, 1u << 20};
    for (uint32_t n : {1u, 1000u, 1024u, 1025u, 5000u, 50200u})
        for (uint32_t nkeys : {0u, 1u, 2u, 3u, 8u, 9u, 19u, 32u})
            for (uint32_t big : cards)          // cardinality of the keys below
                for (uint32_t nbig = 0; nbig <= std::min(nkeys, 3u); ++nbig)
                    for (uint32_t small : {1u, 5u, 20u, 33u})
                        for (uint32_t bits : {0u, 1u, 4u, 5u, 16u, 39u, 64u}) {
                            uint32_t lab_max[kIdxMaxKeys] = {};
                            for (uint32_t k = 0; k < nkeys; ++k) lab_max[k] = k < nbig ? big : small;
                            const uint64_t taints = bits == 0 ? 0ull : bits == 64 ? ~0ull : ((1ull << bits) - 1ull);
                            IndexedLayout l;
                            const char *why = nullptr;
                            if (!indexed_plan(l, n, nkeys, lab_max, taints, &why)) {
                                ++refused;
                                CHECK(why != nullptr);
                                continue;
                            }
                            ++admitted;
                            with_lists += l.nlist > 0;
                            const uint32_t every = tile_lds_layout(l, kLdsEveryRegion).bytes;
                            CHECK(every <= kLdsBudget);
                            CHECK(every == l.rows * 128u + lds_non_row_bytes(l.nlist));
                            tight += every + kPrefetchDumpBytes > kLdsBudget;
                            // the fused forms without the park are subsets of it (plus the dump, where it fits)
                            for (uint32_t m = 0; m < 8; ++m) {
                                const TileTerms t{(m & 1u) != 0, (m & 2u) != 0, (m & 4u) != 0, false, false};
                                const TileLds d = tile_lds_layout(l, lds_want(t, false));
                                CHECK(d.bytes <= kLdsBudget);
                                CHECK(d.off_pf == 0xFFFFFFFFu || d.off_pf + kPrefetchDumpBytes == d.bytes);
                            }
                        }
    CHECK(admitted > 1000 && refused > 100 && with_lists > 100 && tight > 0);
}

// ---- the fused kernel's geometry ------------------------------------------------------------------------------------------
struct GeoCase {
    uint32_t p, tiles, lds;
    bool pick;
    uint32_t grid_cus;
    int order;
    uint32_t debug;
    uint32_t units, chunks, unit_q, unit_rem, u_stride, wave_major, tiles_rcp, run, grid, pick_ppb, pick_waves;
};

constexpr uint32_t kC3Lds = 153504u;  // C3 with the tile-test pick riding: fit + selector + park + dump (the table above)
constexpr uint32_t kBit31 = 0x80000000u;

static const GeoCase kGeoCases[] = {
    // C3, the tile-test pick riding (profiles/r06_r7i_r7k_chunk_count.txt): 49 chunks with the rule, 51 without; grid 248
    {100000, 5, kC3Lds, true, 0, 0, 0, 12500, 49, 255, 5, 6272, 1, 858993459u, 31, 248, 409, 7},
    {100000, 5, kC3Lds, true, 0, 0, kBit31, 12500, 51, 245, 5, 6528, 1, 858993459u, 32, 256, 393, 7},
    {100000, 5, kC3Lds, true, 0, 1, 0, 12500, 51, 245, 5, 8, 1, 858993459u, 32, 256, 393, 7},       // blocked: the rule is off
    {100000, 5, kC3Lds, true, 0, 2, 0, 12500, 49, 255, 5, 6272, 0, 858993459u, 31, 248, 409, 7},    // interleaved, chunk-major
    // the rule's edges at 5 tiles (51 resident chunks = 816 streams): one round per wave, two (cut / nothing to cut), three
    {52224, 5, kC3Lds, true, 0, 0, 0, 6528, 51, 128, 0, 6528, 1, 858993459u, 32, 256, 205, 4},
    {52225, 5, kC3Lds, true, 0, 0, 0, 6529, 26, 251, 3, 3328, 1, 858993459u, 17, 136, 402, 7},
    {52225, 5, kC3Lds, true, 0, 0, kBit31, 6529, 51, 128, 1, 6528, 1, 858993459u, 32, 256, 205, 4},
    {104448, 5, kC3Lds, true, 0, 0, 0, 13056, 51, 256, 0, 6528, 1, 858993459u, 32, 256, 410, 7},
    {104449, 5, kC3Lds, true, 0, 0, 0, 13057, 51, 256, 1, 6528, 1, 858993459u, 32, 256, 410, 7},
    {104449, 5, kC3Lds, true, 0, 0, kBit31, 13057, 51, 256, 1, 6528, 1, 858993459u, 32, 256, 410, 7},
    // ... and at 50 tiles (5 resident chunks = 80 streams)
    {5120, 50, kC3Lds, true, 0, 0, 0, 640, 5, 128, 0, 640, 1, 85899345u, 32, 256, 21, 1},
    {5121, 50, kC3Lds, true, 0, 0, 0, 641, 3, 213, 2, 384, 1, 85899345u, 19, 152, 35, 1},
    {5121, 50, kC3Lds, true, 0, 0, kBit31, 641, 5, 128, 1, 640, 1, 85899345u, 32, 256, 21, 1},
    {10240, 50, kC3Lds, true, 0, 0, 0, 1280, 5, 256, 0, 640, 1, 85899345u, 32, 256, 41, 1},
    {10241, 50, kC3Lds, true, 0, 0, 0, 1281, 5, 256, 1, 640, 1, 85899345u, 32, 256, 41, 1},
    {10241, 50, kC3Lds, true, 0, 0, kBit31, 1281, 5, 256, 1, 640, 1, 85899345u, 32, 256, 41, 1},
    // per_block: 16 rounds per block, 4 when a pick rides; debug bits 18-19 = 1: 16, 2: 4, 3: 1 whatever the pick
    {4096, 5, kC3Lds, false, 0, 0, 0, 512, 4, 128, 0, 512, 1, 858993459u, 3, 24, 0, 0},
    {4096, 5, kC3Lds, true, 0, 0, 0, 512, 16, 32, 0, 2048, 1, 858993459u, 10, 80, 52, 1},
    {4096, 5, kC3Lds, false, 0, 0, 1u << 18, 512, 4, 128, 0, 512, 1, 858993459u, 3, 24, 0, 0},
    {4096, 5, kC3Lds, true, 0, 0, 1u << 18, 512, 4, 128, 0, 512, 1, 858993459u, 3, 24, 205, 4},
    {4096, 5, kC3Lds, false, 0, 0, 2u << 18, 512, 16, 32, 0, 2048, 1, 858993459u, 10, 80, 0, 0},
    {4096, 5, kC3Lds, true, 0, 0, 2u << 18, 512, 16, 32, 0, 2048, 1, 858993459u, 10, 80, 52, 1},
    {4096, 5, kC3Lds, false, 0, 0, 3u << 18, 512, 51, 10, 2, 6528, 1, 858993459u, 32, 256, 0, 0},
    {4096, 5, kC3Lds, true, 0, 0, 3u << 18, 512, 51, 10, 2, 6528, 1, 858993459u, 32, 256, 17, 1},
    // two blocks per compute unit up to half the LDS budget
    {100000, 5, 81920, false, 0, 0, 0, 12500, 98, 127, 54, 12544, 1, 858993459u, 62, 496, 0, 0},
    {100000, 5, 81921, false, 0, 0, 0, 12500, 49, 255, 5, 6272, 1, 858993459u, 31, 248, 0, 0},
    // grid_cus: 0 = the whole chip, clamped to 256
    {100000, 5, kC3Lds, false, 64, 0, 0, 12500, 12, 1041, 8, 1536, 1, 858993459u, 8, 64, 0, 0},
    {100000, 5, kC3Lds, false, 256, 0, 0, 12500, 49, 255, 5, 6272, 1, 858993459u, 31, 248, 0, 0},
    {100000, 5, kC3Lds, false, 300, 0, 0, 12500, 49, 255, 5, 6272, 1, 858993459u, 31, 248, 0, 0},
    // debug bit 5: the grid is not padded to whole runs
    {100000, 5, kC3Lds, true, 0, 0, 32u, 12500, 49, 255, 5, 6272, 1, 858993459u, 31, 245, 409, 7},
    // tiles_rcp: one tile clamps to 0xFFFFFFFF; three tiles: floor(2^32 / 3) * 3 is one short of 2^32
    {1000, 1, kC3Lds, true, 0, 0, 0, 125, 4, 31, 1, 512, 1, 4294967295u, 1, 8, 250, 4},
    {1000, 3, kC3Lds, true, 0, 0, 0, 125, 4, 31, 1, 512, 1, 1431655765u, 2, 16, 84, 2},
    // pick_waves: ceil(pick_ppb / 64) clamped to 1 .. 8
    {1, 1, kC3Lds, true, 1, 0, 0, 1, 1, 1, 0, 128, 1, 4294967295u, 1, 8, 1, 1},
    {64, 1, kC3Lds, true, 1, 0, 0, 8, 1, 8, 0, 128, 1, 4294967295u, 1, 8, 64, 1},
    {65, 1, kC3Lds, true, 1, 0, 0, 9, 1, 9, 0, 128, 1, 4294967295u, 1, 8, 65, 2},
    {5000, 1, kC3Lds, true, 1, 0, 0, 625, 1, 625, 0, 128, 1, 4294967295u, 1, 8, 5000, 8},
    {1u << 20, 1, kC3Lds, true, 1, 0, 0, 131072, 1, 131072, 0, 128, 1, 4294967295u, 1, 8, 1048576, 8},
    {1u << 20, 64, kC3Lds, true, 0, 0, 0, 131072, 4, 32768, 0, 512, 1, 67108864u, 32, 256, 4096, 8},
};

static void test_fused_geometry() {
    for (const GeoCase &c : kGeoCases) {
        const FusedGeometry g = fused_geometry({c.p, c.tiles, c.lds, c.pick, c.grid_cus, c.order, c.debug});
        const bool same = g.units == c.units && g.chunks == c.chunks && g.unit_q == c.unit_q && g.unit_rem == c.unit_rem && g.u_stride == c.u_stride &&
                          g.wave_major == c.wave_major && g.tiles_rcp == c.tiles_rcp && g.run == c.run && g.grid == c.grid && g.pick_ppb == c.pick_ppb &&
                          g.pick_waves == c.pick_waves;
        if (!same)
            std::printf("  p %u tiles %u lds %u pick %d cus %u order %d debug 0x%x: chunks %u grid %u u_stride %u\n", c.p, c.tiles, c.lds, c.pick, c.grid_cus,
                        c.order, c.debug, g.chunks, g.grid, g.u_stride);
        CHECK(same);
    }
    CHECK((uint64_t)1431655765u * 3u == (1ull << 32) - 1u);
}

// ---- the summary kernel's geometry -----------------------------------------------------------------------------------------
static void test_summary_geometry() {
    struct { uint32_t p, tiles, lds, rounds, chunks, grid; } cases[] = {
        {1, 1, 140960, 1, 1, 1},           {1, 50, 140960, 1, 1, 50},          {1024, 5, 140960, 16, 1, 5},       {1025, 5, 140960, 17, 2, 10},
        {1025, 50, 81920, 17, 2, 100},     {100000, 1, 140960, 1563, 98, 98},  {100000, 5, 140960, 1563, 51, 255}, {100000, 5, 81920, 1563, 98, 490},
        {100000, 50, 140960, 1563, 5, 250}, {100000, 50, 81920, 1563, 10, 500}, {1u << 20, 1, 140960, 16384, 256, 256}, {1u << 20, 1, 81920, 16384, 512, 512},
        {1u << 20, 5, 140960, 16384, 51, 255}, {1u << 20, 5, 81920, 16384, 102, 510}, {1u << 20, 50, 140960, 16384, 5, 250},
    };
    for (const auto &c : cases) {
        const SummaryGeometry g = summary_geometry(c.p, c.tiles, c.lds);
        CHECK(g.rounds == c.rounds && g.chunks == c.chunks && g.grid == c.grid);
    }
}

// ---- the argument fill and the derived terms --------------------------------------------------------------------------------
// stand-ins with the members FusedArgs and SummaryArgs share (the kernels' own structs live next to the kernels)
struct ArgsLike {
    uint32_t p, tiles, rows, nkeys, ngroups, row_zero, row_valid, row_cpu, row_taint;
    uint32_t lab_off[8], lab_mx1[8];
    const uint32_t *lab_meta;
    const uint64_t *zero64;
    uint32_t off_aux, off_fit, off_lab, off_trow, off_list, off_lrec, nlist, list_mask8;
    uint32_t list_col[kMaxListKeys];
    uint32_t has_tol;
};

static void test_fill_and_terms() {
    IndexedSnapshot s;
    const uint32_t lab_max[8] = {2, 3, 4, 5000, 16, 32, 64, 4000};
    const char *why = "";
    CHECK(indexed_plan(s.lay, 5000, 8, lab_max, 0x7, &why));
    const IndexedLayout &l = s.lay;
    CHECK(l.nlist == 2 && l.list_col[0] == 3 && l.list_col[1] == 7);
    uint32_t meta[72] = {};
    s.d_lab_meta = meta;  // (never followed: only its address goes into the arguments)
    uint32_t sel_ids[1] = {};
    uint64_t tol[1] = {};
    EvalRequest r;
    r.p = 777;
    r.flags = KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT;
    r.psel = sel_ids;
    r.ptol = tol;
    TileTerms t = tile_terms(r, l);
    CHECK(t.fit && t.sel && t.taint && t.list && !t.want_fit);
    const TileLds d = tile_lds_layout(l, lds_want(t, false));
    ArgsLike a{};
    fill_tile_args(a, s, d, t, r);
    CHECK(a.p == 777 && a.tiles == 5 && a.rows == 403 && a.nkeys == 8 && a.ngroups == 1 && a.row_zero == 0 && a.row_valid == 1 && a.row_taint == 2);
    CHECK(a.row_cpu == 403 - 2 * kFitRows);
    // rows: zero, valid, 16 taint rows, then the keys with rows in column order, each with its all-zero row
    const uint32_t base[8] = {18, 21, 25, kLabList, 30, 47, 80, kLabList};
    for (int k = 0; k < 8; ++k) {
        CHECK(l.lab_base[k] == base[k]);
        CHECK(a.lab_off[k] == (base[k] == kLabList ? 0u : (base[k] - 1u) * 128u));
        CHECK(a.lab_mx1[k] == (base[k] == kLabList ? 0u : lab_max[k] + 1u));
    }
    CHECK(a.lab_meta == meta && a.zero64 == reinterpret_cast<const uint64_t *>(meta + 64));
    CHECK(a.off_aux == 51584u && a.off_fit == 84384u && a.off_lab == 100768u && a.off_trow == 117152u && a.off_list == 125344u && a.off_lrec == 137632u);
    CHECK(a.nlist == 2 && a.list_col[0] == 3 && a.list_col[1] == 7 && a.list_mask8 == ((1u << 3) | (1u << 7)) && a.has_tol == 1);
    // no selectors given: the selector term is off, and with it the lists; no tolerations: has_tol 0
    r.psel = nullptr;
    r.ptol = nullptr;
    r.flags |= KSCHED_WANT_FIT_MASK;
    uint64_t fit_mask[1];
    r.out_fit = fit_mask;
    t = tile_terms(r, l);
    CHECK(t.fit && !t.sel && t.taint && !t.list && t.want_fit);
    ArgsLike b{};
    fill_tile_args(b, s, tile_lds_layout(l, kLdsEveryRegion), t, r);
    CHECK(b.nlist == 0 && b.list_mask8 == 0 && b.has_tol == 0 && b.off_lrec == 137632u);
    // a layout without taint groups: the taint flag alone does not make the term
    IndexedLayout plain;
    CHECK(indexed_plan(plain, 5000, 0, lab_max, 0, &why));
    r.flags = KSCHED_SEL | KSCHED_TAINT;
    r.psel = sel_ids;
    t = tile_terms(r, plain);
    CHECK(!t.fit && !t.sel && !t.taint && !t.list);  // (no label keys either)
}

// ---- the predicate dispatcher ----------------------------------------------------------------------------------------------
static void test_with_predicates() {
    for (int m = 0; m < 8; ++m) {
        const bool fit = m & 4, sel = m & 2, taint = m & 1;
        const int got = with_predicates(fit, sel, taint, [](auto F, auto S, auto T) {
            constexpr int v = (decltype(F)::value ? 4 : 0) + (decltype(S)::value ? 2 : 0) + (decltype(T)::value ? 1 : 0);  // compile-time constants
            return v;
        });
        CHECK(got == m);
    }
    int calls = 0;
    with_predicates(false, true, false, [&](auto, auto S, auto T) { calls += decltype(S)::value && !decltype(T)::value; });  // a void callee
    CHECK(calls == 1);
}

int main() {
    test_lds_layout();
    test_fused_geometry();
    test_summary_geometry();
    test_fill_and_terms();
    test_with_predicates();
    std::printf("tile_launch_tests: %d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
