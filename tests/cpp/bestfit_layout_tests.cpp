// bestfit_layout_tests.cpp -- host-side check of the numbers the best-fit structures and launches are sized by
// (csrc/bestfit_layout.hpp), no GPU and no HIP: the sample and level arrays of the two orders, the merge passes, the row bitmaps,
// the hand-over buffer, the rotation of its counter sets and the debug bits.  The literals were computed from the expressions
// ksched_api.hip had written inline before the header existed; the ref_* functions below restate those expressions verbatim and
// are swept against the header.
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/bestfit_layout.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

// ---- the inline expressions as they stood (build_bestfit, build_bestfit_rows, launch_bestfit_rows) ----------------------------

constexpr uint32_t kRefSublists = 128;

struct RefHandover {
    size_t waves1, sub_cap, ctr_u32, mask_u32, reserve, recs, trace, trace2;
    size_t count[3];
};
static RefHandover ref_handover(uint32_t p) {
    RefHandover r;
    const size_t waves1 = ((size_t)p + 63) / 64, sub_cap = ((waves1 + kRefSublists - 1) / kRefSublists) * 64;
    const size_t ctr_u32 = 3 * (size_t)kRefSublists * 32, mask_u32 = ((waves1 * 2 + 15) / 16) * 16;
    r.waves1 = waves1;
    r.sub_cap = sub_cap;
    r.ctr_u32 = ctr_u32;
    r.mask_u32 = mask_u32;
    r.reserve = ctr_u32 + mask_u32 + 16 * (size_t)kRefSublists * sub_cap;
    r.recs = ctr_u32 + mask_u32;
    r.trace = waves1 * 8 + (size_t)kRefSublists * sub_cap * 4;
    r.trace2 = waves1 * 8;
    for (uint32_t slot = 0; slot < 3; ++slot) r.count[slot] = (size_t)slot * kRefSublists * 32;
    return r;
}

struct RefOrder {
    uint32_t n1, n2, nlev, lvl_off[6], lvl_half, nk, passes;
    size_t samples, levels, mem_s2, cpu_s1, cpu_s2;
    bool sampled;
};
static RefOrder ref_order(uint32_t n) {
    RefOrder r{};
    const uint32_t n1 = (n + 63u) / 64u, n2 = (n + 4095u) / 4096u;
    r.n1 = n1;
    r.n2 = n2;
    r.samples = 2 * (size_t)(n1 + n2);
    uint32_t nk = n, off = 0;
    r.nlev = 0;
    while (nk > 8u && r.nlev < 6u) {
        nk = (nk + 7u) / 8u;
        r.lvl_off[r.nlev++] = off;
        off += (nk + 7u) & ~7u;
    }
    r.lvl_half = off;
    r.nk = nk;
    r.levels = 2 * (size_t)off + 8;
    r.sampled = n <= 64u * 64u * 64u;
    r.mem_s2 = (size_t)n1;           // q.mem_s2 = q.mem_s1 + n1
    r.cpu_s1 = r.mem_s2 + n2;        // q.cpu_s1 = q.mem_s2 + n2
    r.cpu_s2 = r.cpu_s1 + n1;        // q.cpu_s2 = q.cpu_s1 + n1
    uint32_t passes = 0;
    for (uint64_t run = 1024; run < n; run <<= 1) ++passes;
    r.passes = passes;
    return r;
}

struct RefRows {
    uint32_t Wbf, q, levels, rows;
};
static RefRows ref_rows(uint32_t n, uint32_t row_cpu) {
    const uint32_t Wbf = ((n + 63u) / 64u + 7u) & ~7u, named = row_cpu;
    const uint32_t levels = 256u, q = (n + levels - 1u) / levels;
    const uint32_t rows = named + levels + 1u;
    return RefRows{Wbf, q, levels, rows};
}

static uint32_t ref_lane_blocks(uint32_t opt_debug) { return ((opt_debug >> 12) & 15u) ? ((opt_debug >> 12) & 15u) : 2u; }
static bool ref_tracing(uint32_t opt_debug) { return (opt_debug & 0x100000u) != 0u; }
static uint32_t ref_grid(uint32_t opt_debug, size_t sub_cap) {
    const uint32_t gshift = ((opt_debug >> 21) & 3u) == 0u ? 2u : ((opt_debug >> 21) & 3u) == 1u ? 0u : ((opt_debug >> 21) & 3u) == 2u ? 1u : 3u;
    const uint32_t per_list = std::max<uint32_t>(1u, (uint32_t)sub_cap >> gshift);
    return kRefSublists * per_list;
}

// ---- pinned literals ----------------------------------------------------------------------------------------------------------

static void handover_cases() {
    CHECK(kBfSublists == 128u && kBfCounterSets == 3u);
    struct Row {
        uint32_t p;
        size_t waves1, sub_cap, mask, rec_off, total, trace;
    };
    const Row rows[] = {
        {1, 1, 64, 16, 12304, 143376, 32776},           {512, 8, 64, 16, 12304, 143376, 32832},
        {513, 9, 64, 32, 12320, 143392, 32840},         {8192, 128, 64, 256, 12544, 143616, 33792},
        {8193, 129, 128, 272, 12560, 274704, 66568},    {24576, 384, 192, 768, 13056, 406272, 101376},
        {125000, 1954, 1024, 3920, 16208, 2113360, 539920},
    };
    for (const Row &w : rows) {
        const BfHandoverLayout h = bf_handover_layout(w.p);
        CHECK(h.waves1 == w.waves1);
        CHECK(h.sub_cap == w.sub_cap);
        CHECK(h.ctr_u32 == 12288u);
        CHECK(h.mask_u32 == w.mask);
        CHECK(h.mask_off() == 12288u);
        CHECK(h.rec_off() == w.rec_off);
        CHECK(h.total_u32() == w.total);
        CHECK(h.trace_u64() == w.trace);
        CHECK(h.trace1_u64() == w.waves1 * 8);
        CHECK(h.trace1_u64() + h.trace2_u64() == h.trace_u64());
        CHECK(h.ctr_off(0) == 0u && h.ctr_off(1) == 4096u && h.ctr_off(2) == 8192u);
        CHECK(h.rec_off() % 16 == 0);  // the 64-byte records stay aligned
    }
}

// entries above the top one of `nlev` level arrays, where the lane-per-pod searches start: at most eight, or the levels do not cover n
static uint32_t top_entries(uint32_t n, uint32_t nlev) {
    for (uint32_t k = 0; k < nlev; ++k) n = (n + 7u) / 8u;
    return n;
}

static void order_cases() {
    struct Row {
        uint32_t n, nlev;
        std::vector<uint32_t> off;
        uint32_t half;
        size_t elems;
        uint32_t n1, n2;
    };
    const Row rows[] = {
        {8, 0, {}, 0, 8, 1, 1},
        {9, 1, {0}, 8, 24, 1, 1},
        {64, 1, {0}, 8, 24, 1, 1},
        {65, 2, {0, 16}, 24, 56, 2, 1},
        {512, 2, {0, 64}, 72, 152, 8, 1},
        {513, 3, {0, 72, 88}, 96, 200, 9, 1},
        {5000, 4, {0, 632, 712, 728}, 736, 1480, 79, 2},
        {262144, 5, {0, 32768, 36864, 37376, 37440}, 37448, 74904, 4096, 64},
        {262145, 6, {0, 32776, 36880, 37400, 37472, 37488}, 37496, 75000, 4097, 65},
    };
    for (const Row &w : rows) {
        const BfOrderLayout o = bf_order_layout(w.n);
        CHECK(o.nlev == w.nlev && o.lvl_half == w.half && o.level_elems() == w.elems && o.n1 == w.n1 && o.n2 == w.n2);
        for (uint32_t k = 0; k < kBfMaxLevels; ++k) CHECK(o.lvl_off[k] == (k < w.off.size() ? w.off[k] : 0u));
        CHECK(o.sample_elems() == 2 * (size_t)(w.n1 + w.n2));
        CHECK(top_entries(w.n, o.nlev) <= 8u);
    }
    const BfOrderLayout big = bf_order_layout(2097152u);
    CHECK(big.nlev == 6u && big.lvl_half == 299592u && big.level_elems() == 599192u);
    // the sampled searches: three rounds of 64
    CHECK(bf_order_layout(262144u).sampled && !bf_order_layout(262145u).sampled);
    // one constant, three spellings: six levels cover n = 8^7 and not one node more
    CHECK(kBfMaxLevels == 6u && kBfLanesMaxNodes == 2097152u);
    CHECK(bf_order_layout(kBfLanesMaxNodes).nlev == 6u && top_entries(kBfLanesMaxNodes, 6) == 8u);
    CHECK(bf_order_layout(kBfLanesMaxNodes + 1u).nlev == 6u && top_entries(kBfLanesMaxNodes + 1u, 6) == 9u);
    // merge passes behind the runs of 1024
    const uint32_t passes[][2] = {{1, 0}, {1024, 0}, {1025, 1}, {2048, 1}, {2049, 2}, {70001, 7}, {2097152, 11}};
    for (auto &w : passes) CHECK(bf_order_layout(w[0]).merge_passes == w[1]);
    CHECK(bf_order_layout(0).merge_passes == 0u && bf_order_layout(0).nlev == 0u && bf_order_layout(0).level_elems() == 8u);
    CHECK(bf_searched_elems(0) == 8u && bf_searched_elems(70001) == 70009u && bf_searched_elems(0xFFFFFFFFu) == 0x100000007ull);
}

static void row_cases() {
    const uint32_t rows[][4] = {{1, 8, 1, 297}, {512, 8, 2, 297}, {513, 16, 3, 297}, {700, 16, 3, 297}, {70001, 1096, 274, 297}};
    for (auto &w : rows) {
        const BfRowLayout l = bf_row_layout(w[0], 40);
        CHECK(l.Wbf == w[1] && l.q == w[2] && l.rows == w[3] && l.levels == 256u && l.row_cpu0 == 40u);
        CHECK(l.words() == (size_t)w[3] * w[1]);
        CHECK(l.Wbf % 8 == 0 && (size_t)l.Wbf * 64 >= w[0]);
        CHECK((uint64_t)l.q * l.levels >= w[0]);  // threshold row `levels` is empty
    }
    CHECK(bf_row_layout(5000, 0).rows == 257u && bf_row_layout(5000, 703).rows == 960u);
}

static void rotation_cases() {
    BfRotation r;
    // a fresh capacity zeroes all counters and starts at slot 0
    CHECK(r.fresh(143376));
    r.zeroed(143376);
    CHECK(!r.fresh(143376) && r.use() == 0u && r.zero() == 1u);
    // calls use sets 0, 1, 2, 0 and zero sets 1, 2, 0, 1; an unchanged capacity never zeroes
    const uint32_t use[] = {0, 1, 2, 0}, zero[] = {1, 2, 0, 1};
    for (int i = 0; i < 4; ++i) {
        CHECK(!r.fresh(143376));
        CHECK(r.use() == use[i] && r.zero() == zero[i]);
        r.advance();
    }
    CHECK(r.use() == 1u);
    // asking does not advance: a call that fails before `advance` (launch_bestfit_two_stages calls it only behind the first stage's
    // launch check) finds the same sets again
    for (int i = 0; i < 3; ++i) CHECK(!r.fresh(143376) && r.use() == 1u && r.zero() == 2u);
    r.advance();
    CHECK(r.use() == 2u && r.zero() == 0u);
    r.advance();
    r.advance();
    CHECK(r.use() == 1u);
    // a grown capacity zeroes again and restarts at 0
    CHECK(r.fresh(274704));
    r.zeroed(274704);
    CHECK(!r.fresh(274704) && r.use() == 0u && r.zero() == 1u);
    r.advance();
    r.advance();
    CHECK(r.use() == 2u && r.zero() == 0u);
    CHECK(BfRotation{}.fresh(143376));  // the first call of a context
}

static void debug_cases() {
    for (uint32_t v = 0; v < 16; ++v) {
        const BfDebug d = bf_debug(v << 12);
        CHECK(d.lane_blocks == (v ? v : 2u));
        CHECK(!d.tracing && d.grid_shift == 2u);
    }
    const uint32_t shift[4] = {2, 0, 1, 3};
    const uint32_t grid64[4] = {2048, 8192, 4096, 1024}, grid1024[4] = {32768, 131072, 65536, 16384};
    for (uint32_t v = 0; v < 4; ++v) {
        const BfDebug d = bf_debug(v << 21);
        CHECK(d.grid_shift == shift[v] && d.lane_blocks == 2u && !d.tracing);
        CHECK(bf_handed_grid(64, d.grid_shift) == grid64[v]);
        CHECK(bf_handed_grid(1024, d.grid_shift) == grid1024[v]);
    }
    CHECK(bf_debug(1u << 20).tracing && bf_debug(1u << 20).lane_blocks == 2u && bf_debug(1u << 20).grid_shift == 2u);
    CHECK(!bf_debug(~(1u << 20)).tracing);
    CHECK(bf_debug(0x400u).lane_blocks == 2u);  // (bit 10 is the plan's: best fit in one stage)
    CHECK(bf_handed_grid(0, 2) == 128u);        // never an empty grid
    const BfDebug all = bf_debug(0xFFFFFFFFu);
    CHECK(all.lane_blocks == 15u && all.tracing && all.grid_shift == 3u);
}

// ---- the sweep: header against the restated expressions ---------------------------------------------------------------------

static unsigned long long g_rows = 0, g_diff = 0;
#define SAME(a, b)                 \
    do {                           \
        ++g_rows;                  \
        if (!((a) == (b))) ++g_diff; \
    } while (0)

static void sweep_p(uint32_t p) {
    const RefHandover r = ref_handover(p);
    const BfHandoverLayout h = bf_handover_layout(p);
    SAME(h.waves1, r.waves1);
    SAME(h.sub_cap, r.sub_cap);
    SAME(h.ctr_u32, r.ctr_u32);
    SAME(h.mask_u32, r.mask_u32);
    SAME(h.mask_off(), r.ctr_u32);
    SAME(h.rec_off(), r.recs);
    SAME(h.total_u32(), r.reserve);
    SAME(h.trace_u64(), r.trace);
    SAME(h.trace1_u64(), r.trace2);
    SAME(h.slots2(), (size_t)kRefSublists * r.sub_cap);
    for (uint32_t slot = 0; slot < 3; ++slot) SAME(h.ctr_off(slot), r.count[slot]);
    for (uint32_t g = 0; g < 4; ++g) SAME(bf_handed_grid(h.sub_cap, bf_debug(g << 21).grid_shift), ref_grid(g << 21, r.sub_cap));
}

static void sweep_n(uint32_t n) {
    const RefOrder r = ref_order(n);
    const BfOrderLayout o = bf_order_layout(n);
    SAME(o.n1, r.n1);
    SAME(o.n2, r.n2);
    SAME(o.sample_elems(), r.samples);
    SAME(o.sampled, r.sampled);
    SAME(o.mem_s2(), r.mem_s2);
    SAME(o.cpu_s1(), r.cpu_s1);
    SAME(o.cpu_s2(), r.cpu_s2);
    SAME(o.nlev, r.nlev);
    for (uint32_t k = 0; k < 6; ++k) SAME(o.lvl_off[k], r.lvl_off[k]);
    SAME(o.lvl_half, r.lvl_half);
    SAME(o.level_elems(), r.levels);
    SAME(o.merge_passes, r.passes);
    SAME(top_entries(n, o.nlev) <= 8u, n <= kBfLanesMaxNodes);
    SAME(bf_searched_elems(n), (size_t)n + 8);
    for (uint32_t row_cpu : {0u, 40u, 703u}) {
        const RefRows w = ref_rows(n, row_cpu);
        const BfRowLayout l = bf_row_layout(n, row_cpu);
        SAME(l.Wbf, w.Wbf);
        SAME(l.q, w.q);
        SAME(l.levels, w.levels);
        SAME(l.rows, w.rows);
        SAME(l.row_cpu0, row_cpu);
        SAME(l.words(), (size_t)w.rows * w.Wbf);
    }
}

static void sweep() {
    // every value up to 70000, plus -2 .. +2 around every power of 8 (and with them of 64) up to 2^22
    std::set<uint32_t> extra;
    for (uint32_t e = 0; e <= 22; e += 3)
        for (int d = -2; d <= 2; ++d) {
            const long long v = (1ll << e) + d;
            if (v > 70000) extra.insert((uint32_t)v);
        }
    for (int d = -2; d <= 2; ++d) extra.insert((uint32_t)((1ll << 22) + d));  // (and 2^22 itself, the upper end)
    for (uint32_t v = 0; v <= 70000; ++v) {
        sweep_p(v);
        sweep_n(v);
    }
    for (uint32_t v : extra) {
        sweep_p(v);
        sweep_n(v);
    }
    for (uint32_t dbg = 0; dbg < (1u << 23); dbg += 0x1000u) {  // every value of bits 12 .. 22
        const BfDebug d = bf_debug(dbg);
        SAME(d.lane_blocks, ref_lane_blocks(dbg));
        SAME(d.tracing, ref_tracing(dbg));
        SAME(bf_handed_grid(1024, d.grid_shift), ref_grid(dbg, 1024));
    }
    std::printf("sweep: %llu rows compared, %llu differences\n", g_rows, g_diff);
    CHECK(g_diff == 0);
    CHECK(g_rows > 3000000ull);
}

int main() {
    handover_cases();
    order_cases();
    row_cases();
    rotation_cases();
    debug_cases();
    sweep();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
