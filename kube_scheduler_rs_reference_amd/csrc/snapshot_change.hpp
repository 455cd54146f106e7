// snapshot_change.hpp -- the pure parts of a node-snapshot change: which rows of an update count, whether the index layout survives
// new labels, where the fields of a staging block lie, and what a change makes stale.
//
// Host-only on purpose, like eval_plan.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/snapshot_change_tests.cpp pins every rule at its boundary without a GPU.  The protocol that uses them -- begin,
// stage / upload, commit -- is SnapshotChange in ksched_api.hip.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/ksched.h"

namespace ksched {

constexpr uint32_t kChangeTileNodes = 1024;  // == kTileNodes (tile_index.hpp needs HIP; ksched_api.hip asserts the two agree)

// A node listed twice takes its last row (the patch kernels' threads are unordered): `keep` = the row numbers of the last occurrence
// of every node index, ascending by node; `tiles` = the kChangeTileNodes-node tiles they touch, ascending and unique.  One row -- the
// watch-event case -- is not sorted (std::stable_sort would ask for a buffer); `keep` is sorted and thinned in place.
inline void last_wins(const uint32_t *node_index, uint32_t count, std::vector<uint32_t> &keep, std::vector<uint32_t> &tiles) {
    keep.resize(count);
    std::iota(keep.begin(), keep.end(), 0u);
    if (count > 1) std::stable_sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) { return node_index[a] < node_index[b]; });
    uint32_t m = 0;
    for (uint32_t i = 0; i < count; ++i)
        if (i + 1 == count || node_index[keep[i + 1]] != node_index[keep[i]]) keep[m++] = keep[i];
    keep.resize(m);
    tiles.clear();
    for (uint32_t i : keep)
        if (tiles.empty() || tiles.back() != node_index[i] / kChangeTileNodes) tiles.push_back(node_index[i] / kChangeTileNodes);
}

// Does the planned index layout still hold for the new labels and taints of a label update?  Every new id at most its key's planned
// maximum, every new taint bit inside the planned taint groups (4 bits each; 16 or more cover every bit); without a built index it
// never holds.  `lab_max` [KSCHED_MAX_KEYS] and `all_taints` come in as planned and leave as the union of the planned and the new:
// what a re-plan is made for.  `lab` is [nkeys][count] and `taints` [count] (or nullptr), read at the `m` kept rows.
inline bool label_layout_holds(uint32_t *lab_max, uint64_t *all_taints, bool index_built, uint32_t ngroups, uint32_t nkeys, uint32_t count,
                               const uint32_t *keep, uint32_t m, const uint32_t *lab, const uint64_t *taints) {
    bool holds = index_built;
    for (uint32_t k = 0; k < nkeys; ++k)
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t id = lab[(size_t)k * count + keep[j]];
            if (id > lab_max[k]) {
                lab_max[k] = id;
                holds = false;
            }
        }
    if (taints) {
        for (uint32_t j = 0; j < m; ++j) *all_taints |= taints[keep[j]];
        const uint32_t groups = index_built ? ngroups : 0u;
        const uint64_t covered = groups >= 16u ? ~0ull : (1ull << (4u * groups)) - 1ull;
        if (*all_taints & ~covered) holds = false;
    }
    return holds;
}

// The fields of one staging block, in the order they are added: add<T>(count) gives the field's offset, aligned to T; an empty field
// takes no room and no padding.  A call declares its fields once; the host pointers (pinned block) and the device pointers come from
// the same offsets.  (tests/cpp/snapshot_change_tests.cpp restates the three calls' field orders.)
struct StageLayout {
    size_t total = 0;
    template <class T>
    size_t add(size_t count) {
        if (count == 0) return total;
        total = (total + alignof(T) - 1) & ~(alignof(T) - 1);
        const size_t off = total;
        total += count * sizeof(T);
        return off;
    }
};
// What a committed change makes stale, in rising order.  The best-fit structures are rebuilt lazily (ensure_bestfit): their ORDER reads
// `available` only, their row bitmaps read labels and taints too, in that order.  kEverything is ksched_set_nodes: a new snapshot.
enum class Stale { kNothing, kLabels, kAvailable, kEverything };
inline bool stale_order(Stale s) { return s >= Stale::kAvailable; }     // BestfitIndex::order_stale: the order, and the rows with it
inline bool stale_rows_only(Stale s) { return s == Stale::kLabels; }    // BestfitIndex::rows_stale

}  // namespace ksched
