// snapshot_change_tests.cpp -- host-side check of the pure parts of a node-snapshot change (csrc/snapshot_change.hpp), no GPU and no
// HIP: which rows of an update count, whether the index layout survives a label update, where the staging fields lie, what a change
// makes stale.  The expectations restate the rules as the entry points had them written out by hand before the header existed; they
// are written out here, not computed by the header.
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/snapshot_change.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

using U32s = std::vector<uint32_t>;

// ---- last_wins ----------------------------------------------------------------------------------------------------------------

// the naive restatement: a map from node to the last row that names it, read in key order; the tiles as a map's keys
static void last_wins_naive(const U32s &node, U32s &keep, U32s &tiles) {
    std::map<uint32_t, uint32_t> last;
    for (uint32_t i = 0; i < node.size(); ++i) last[node[i]] = i;
    std::map<uint32_t, bool> t;
    keep.clear();
    tiles.clear();
    for (auto &kv : last) {
        keep.push_back(kv.second);
        t[kv.first / 1024u] = true;
    }
    for (auto &kv : t) tiles.push_back(kv.first);
}

static void last_wins_cases() {
    U32s keep{7, 7}, tiles{9};  // (whatever they held is replaced)
    last_wins(nullptr, 0, keep, tiles);
    CHECK(keep.empty() && tiles.empty());
    const uint32_t one[] = {5000};
    last_wins(one, 1, keep, tiles);
    CHECK(keep == U32s{0} && tiles == U32s{4});
    const uint32_t twice[] = {9, 3, 9};  // the last row of node 9 wins; ascending by node: 3 (row 1), 9 (row 2)
    last_wins(twice, 3, keep, tiles);
    CHECK((keep == U32s{1, 2}) && tiles == U32s{0});
    const uint32_t many[] = {2050, 1, 2050, 1, 1, 2050, 7, 1};  // node 1: row 7, node 7: row 6, node 2050: row 5
    last_wins(many, 8, keep, tiles);
    CHECK((keep == U32s{7, 6, 5}) && (tiles == U32s{0, 2}));
    const uint32_t edge[] = {1024, 1023};  // the last node of tile 0 and the first of tile 1
    last_wins(edge, 2, keep, tiles);
    CHECK((keep == U32s{1, 0}) && (tiles == U32s{0, 1}));
    const uint32_t same_tile[] = {1023, 0};
    last_wins(same_tile, 2, keep, tiles);
    CHECK((keep == U32s{1, 0}) && tiles == U32s{0});
    const U32s all_one(100, 4096u);  // every row on one node
    last_wins(all_one.data(), 100, keep, tiles);
    CHECK(keep == U32s{99} && tiles == U32s{4});
    std::mt19937 rng(20240607u);
    for (int round = 0; round < 400; ++round) {
        const uint32_t count = 1u + rng() % 300u, span = 1u + rng() % (round % 2 ? 40u : 9000u);
        U32s node(count), k2, t2;
        for (auto &x : node) x = rng() % span;
        last_wins(node.data(), count, keep, tiles);
        last_wins_naive(node, k2, t2);
        CHECK(keep == k2 && tiles == t2);
    }
}

// ---- does the planned layout hold? ------------------------------------------------------------------------------------------

struct Plan {
    uint32_t lab_max[KSCHED_MAX_KEYS] = {};
    uint64_t taints = 0;
};

// one row (keep = {0}) of two keys over a plan of maxima {5, 9} and taint bits 0x3
static bool holds_one(Plan &p, bool built, uint32_t ngroups, uint32_t id0, uint32_t id1, const uint64_t *taint) {
    const uint32_t keep[] = {0}, lab[] = {id0, id1};
    return label_layout_holds(p.lab_max, &p.taints, built, ngroups, 2, 1, keep, 1, lab, taint);
}
static Plan plan59() {
    Plan p;
    p.lab_max[0] = 5;
    p.lab_max[1] = 9;
    p.taints = 0x3;
    return p;
}

static void layout_cases() {
    Plan p = plan59();
    CHECK(holds_one(p, true, 1, 5, 9, nullptr));  // ids equal to their keys' maxima
    CHECK(p.lab_max[0] == 5 && p.lab_max[1] == 9 && p.taints == 0x3);
    p = plan59();
    CHECK(!holds_one(p, true, 1, 6, 9, nullptr));  // maximum + 1 on the first key
    CHECK(p.lab_max[0] == 6 && p.lab_max[1] == 9);
    p = plan59();
    CHECK(!holds_one(p, true, 1, 0, 10, nullptr));  // ... on the second
    CHECK(p.lab_max[0] == 5 && p.lab_max[1] == 10);
    p = plan59();
    CHECK(!holds_one(p, false, 1, 0, 0, nullptr));  // no index built: never
    uint64_t t = 0;
    CHECK(!holds_one(p, false, 16, 0, 0, &t));
    // taint groups of 4 bits: bit 4 * ngroups - 1 is covered, bit 4 * ngroups is not
    for (uint32_t g = 1; g < 16; ++g) {
        p = plan59();
        t = 1ull << (4 * g - 1);
        CHECK(holds_one(p, true, g, 0, 0, &t));
        CHECK(p.taints == (0x3ull | t));  // the union of the planned and the new bits
        p = plan59();
        t = 1ull << (4 * g);
        CHECK(!holds_one(p, true, g, 0, 0, &t));
        CHECK(p.taints == (0x3ull | t));
    }
    for (uint32_t g : {16u, 17u, 64u}) {  // 16 or more groups cover every bit
        p = plan59();
        t = 1ull << 63;
        CHECK(holds_one(p, true, g, 0, 0, &t));
    }
    p = plan59();
    t = 1ull << 63;
    CHECK(!holds_one(p, true, 15, 0, 0, &t));
    p = plan59();  // planned bits outside the groups count too, once the update brings taints (ngroups 0: no taint rows)
    t = 0;
    CHECK(!holds_one(p, true, 0, 0, 0, &t));
    CHECK(holds_one(p, true, 0, 0, 0, nullptr));  // ... and not when it brings none
    // several rows, [nkeys][count] with only the kept rows read: row 1 (dropped) carries ids and bits beyond the plan
    p = plan59();
    const uint32_t keep[] = {2, 0}, lab[] = {1, 99, 5, /* key 1 */ 2, 99, 9};
    const uint64_t taints[] = {0x1, 0xF0, 0x2};
    CHECK(label_layout_holds(p.lab_max, &p.taints, true, 1, 2, 3, keep, 2, lab, taints));
    CHECK(p.lab_max[0] == 5 && p.lab_max[1] == 9 && p.taints == 0x3);
    const uint32_t keep_all[] = {0, 1, 2};
    CHECK(!label_layout_holds(p.lab_max, &p.taints, true, 1, 2, 3, keep_all, 3, lab, taints));
    CHECK(p.lab_max[0] == 99 && p.lab_max[1] == 99 && p.taints == 0xF3);  // merged: the union
}

// ---- staging layouts ----------------------------------------------------------------------------------------------------------
// The three field orders, as the entry points declare them (ksched_api.hip), against the offsets those entry points computed by hand
// before StageLayout existed.

static size_t round8(size_t x) { return (x + 7) & ~(size_t)7; }

static void stage_cases() {
    const size_t kMetaWords = 72;
    for (size_t n : {0, 1, 2, 3, 7, 8, 1023, 1024, 1025, 5000})
        for (size_t nkeys : {0, 1, 2, 3, 7, 8, 16})
            for (int have_taints = 0; have_taints < 2; ++have_taints)
                for (size_t meta : {(size_t)0, kMetaWords}) {
                    // ksched_set_nodes: [cpu i64 n][mem i64 n][ids u32 n_keys x n][taints u64 n][meta words]
                    StageLayout f;
                    const size_t o_cpu = f.add<int64_t>(n), o_mem = f.add<int64_t>(n), o_lab = f.add<uint32_t>(n * nkeys);
                    const size_t o_taint = f.add<uint64_t>(have_taints ? n : 0), o_meta = f.add<uint32_t>(meta);
                    const size_t b_col = n * 8, b_lab = n * nkeys * 4, b_taint = have_taints ? b_col : 0;
                    if (n > 0) CHECK(o_cpu == 0 && o_mem == b_col);
                    if (b_lab) CHECK(o_lab == 2 * b_col);
                    // By hand the taint column lay at 2 * b_col + b_lab, which is 4 mod 8 when n * n_keys is odd (it was only ever
                    // the source of a memcpy); as a typed field it is rounded up to 8, and the meta words follow it.
                    const size_t hand_taint = 2 * b_col + b_lab, pad = b_taint ? round8(hand_taint) - hand_taint : 0;
                    if (b_taint) CHECK(o_taint == hand_taint + pad && o_taint % 8 == 0 && ((n * nkeys) % 2 || pad == 0));
                    if (meta) CHECK(o_meta == hand_taint + pad + b_taint);
                    CHECK(f.total == hand_taint + pad + b_taint + meta * 4);
                    CHECK(o_cpu % 8 == 0 && o_mem % 8 == 0);
                }
    for (size_t m : {1, 2, 3, 16, 17, 255, 256, 1001})
        for (size_t nkeys : {0, 1, 2, 3, 8, 16})
            for (int have_taints = 0; have_taints < 2; ++have_taints)
                for (size_t ntiles : {1, 2, 5})
                    for (size_t meta : {(size_t)0, kMetaWords}) {
                        // ksched_update_node_labels: [taints u64 m][node u32 m][ids u32 nkeys x m][tiles u32], copied; then [meta words]
                        StageLayout f;
                        const size_t o_taint = f.add<uint64_t>(have_taints ? m : 0), o_idx = f.add<uint32_t>(m), o_lab = f.add<uint32_t>(nkeys * m);
                        const size_t o_tiles = f.add<uint32_t>(ntiles), b_dev = f.total, o_meta = f.add<uint32_t>(meta);
                        const size_t b_taint = have_taints ? m * 8 : 0, b_idx = m * 4, b_lab = nkeys * m * 4, b_tiles = ntiles * 4;
                        if (have_taints) CHECK(o_taint == 0);
                        CHECK(o_idx == b_taint);
                        if (nkeys) CHECK(o_lab == b_taint + b_idx);
                        CHECK(o_tiles == b_taint + b_idx + b_lab);
                        CHECK(b_dev == b_taint + b_idx + b_lab + b_tiles);
                        if (meta) CHECK(o_meta == b_dev);
                        CHECK(f.total == b_dev + meta * 4);
                    }
    for (size_t m : {17, 18, 19, 255, 256, 1001, 100000})
        for (size_t ntiles : {1, 2, 17, 98}) {
            // ksched_update_nodes beyond the inline size: [node u32 m][cpu i64 m][mem i64 m][tiles u32]
            StageLayout f;
            const size_t o_idx = f.add<uint32_t>(m), o_cpu = f.add<int64_t>(m), o_mem = f.add<int64_t>(m), o_tiles = f.add<uint32_t>(ntiles);
            const size_t b_idx = (m * 4 + 7) & ~(size_t)7, b_val = m * 8;
            CHECK(o_idx == 0 && o_cpu == b_idx && o_mem == b_idx + b_val && o_tiles == b_idx + 2 * b_val);
            CHECK(f.total == b_idx + 2 * b_val + ntiles * 4);
            CHECK(o_cpu % 8 == 0 && o_mem % 8 == 0);
        }
    // an empty field takes no room and no padding; alignment follows the type
    StageLayout f;
    CHECK(f.add<uint8_t>(3) == 0 && f.add<uint64_t>(0) == 3 && f.total == 3);
    CHECK(f.add<uint16_t>(1) == 4 && f.add<uint32_t>(1) == 8 && f.add<uint64_t>(1) == 16 && f.total == 24);
}

// ---- what a change makes stale ------------------------------------------------------------------------------------------------

static void stale_cases() {
    // what each call set by hand: ksched_update_nodes and the applies bf_dirty, ksched_update_node_labels bf_rows_dirty,
    // ksched_set_nodes bf_dirty (and bf_rows_built = false), the lazy best-fit rebuild neither
    CHECK(stale_order(Stale::kAvailable) && !stale_rows_only(Stale::kAvailable));
    CHECK(!stale_order(Stale::kLabels) && stale_rows_only(Stale::kLabels));
    CHECK(stale_order(Stale::kEverything) && !stale_rows_only(Stale::kEverything));
    CHECK(!stale_order(Stale::kNothing) && !stale_rows_only(Stale::kNothing));
}

int main() {
    last_wins_cases();
    layout_cases();
    stage_cases();
    stale_cases();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
