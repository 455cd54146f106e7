// apply_plan.hpp -- what one ksched_apply_bindings_device / _sharded / _sharded_local call does, decided in one place: which flag
// words are refused, what happens to the per-node scratch, which passes each rank launches in which order over which grid, and
// which all-gathers join the ranks.  DESIGN.md section 7a has the table.
//
// Host-only on purpose, like eval_plan.hpp and pipe_plan.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/apply_plan_tests.cpp enumerates every combination of flags, communicator, sizes, status_out and index without a GPU.
// apply_begin .. apply_run (ksched_api.hip) fill the argument structs and execute the plan; ApplyState there holds the buffers and
// the ApplyScratch below.
//
// The facts are scalars: the flags, whether the call has a communicator and its size, the snapshot's node count, and per rank its
// row count, whether it passed status_out and whether its snapshot has a bitmap index.
//
// The call has three phases, because the collectives sit between them and the one-process form takes each phase through every rank
// before the collective that joins them:
//   phase 0   claim                                     | all-gather of the claims, n words per rank
//   phase 1   claim merge, accumulate -- or keys, sort  | all-gather of the split sums, 8 * n words per rank
//   phase 2   commit (local / gathered / admit), re-index of the dirty tiles, status
// A pass that has nothing to do is not launched; a rank with no rows still joins both collectives, commits what the others sent and
// re-indexes.  Over an empty snapshot (n = 0) only the rank's accumulate pass (or, with KSCHED_APPLY_WHILE_FIT, its keys pass) is
// launched -- every pod is UNBOUND or BAD_NODE, which those passes write -- and no claim, collective, commit, re-index or status pass.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/ksched.h"
#include "merge_sort_plan.hpp"

namespace ksched {

constexpr uint32_t kApplyTileNodes = 1024;           // nodes of a bitmap tile: the commit runs a block per tile, a thread per node
constexpr uint32_t kApplyIdleClaim = 0xFFFFFFFFu;    // an unclaimed node; global pod indexes stay below it

// ---- the flag verdict: what needs no handle -------------------------------------------------------------------------------
// Unknown bits, and WHILE_FIT with another admission rule or with RELEASE (nothing is admitted there): KSCHED_E_INVAL.
inline int apply_flags_check(uint32_t flags) {
    if (flags & ~(uint32_t)(KSCHED_APPLY_FIRST_PER_NODE | KSCHED_APPLY_RELEASE | KSCHED_APPLY_WHILE_FIT)) return KSCHED_E_INVAL;
    if ((flags & KSCHED_APPLY_WHILE_FIT) && (flags & (KSCHED_APPLY_FIRST_PER_NODE | KSCHED_APPLY_RELEASE))) return KSCHED_E_INVAL;
    return KSCHED_OK;
}
// ... and with a communicator WHILE_FIT is unsupported: admission needs every rank's requests per node, in pod order; the per-node
// exchange of claims and sums cannot carry that.
inline int apply_flags_verdict(uint32_t flags, bool comm) {
    if (int rc = apply_flags_check(flags)) return rc;
    if (comm && (flags & KSCHED_APPLY_WHILE_FIT)) return KSCHED_E_UNSUPPORTED;
    return KSCHED_OK;
}
// a rank's global pod indexes row_lo .. row_lo + count - 1 stay below the idle claim
inline bool apply_rows_in_range(uint32_t row_lo, uint32_t count) { return (uint64_t)row_lo + count <= (uint64_t)kApplyIdleClaim; }

// ---- the scratch step -------------------------------------------------------------------------------------------------
// The per-node scratch (acc, claim, ovf, dirty) is idle between calls: every call leaves it as it found it, so it is allocated and
// memset once per snapshot size.  `n` = nodes it holds in its idle state (0 = not yet, or a failed call left it unknown); `gen` = the
// generation of the latest call: tile t is dirty for call g when dirty[t] == dirty[tiles] == g, and 0 is every entry's initial value.
struct ApplyScratch {
    uint32_t n = 0, gen = 0;
    void invalidate() { n = 0; }
};
struct ApplyScratchStep {
    bool allocate = false;  // reserve the four buffers for `cap` nodes and memset acc (0), claim (0xFF) and dirty (0); ovf needs none
    uint32_t cap = 0, cap_tiles = 0;
    size_t acc_elems = 0, claim_elems = 0, ovf_elems = 0, dirty_elems = 0;  // what is reserved (uint64, uint32, uint8, uint32)
    size_t acc_bytes = 0, claim_bytes = 0, dirty_bytes = 0;                 // what is memset
    ApplyScratch next;      // once everything is enqueued; next.gen is this call's generation
};
inline ApplyScratchStep plan_apply_scratch(ApplyScratch s, uint32_t n) {
    ApplyScratchStep st;
    st.next = s;
    if (s.n == 0 || n > s.n) {  // (an empty snapshot needs the scratch too: the accumulate pass writes dirty[0])
        st.allocate = true;
        st.cap = std::max<uint32_t>(n, 1024u);
        st.cap_tiles = (st.cap + kApplyTileNodes - 1u) / kApplyTileNodes;
        st.acc_elems = (size_t)st.cap * 4;
        st.claim_elems = st.ovf_elems = st.cap;
        st.dirty_elems = st.cap_tiles + 1u;
        st.acc_bytes = (size_t)st.cap * 32;
        st.claim_bytes = (size_t)st.cap * 4;
        st.dirty_bytes = (size_t)(st.cap_tiles + 1u) * 4;
        st.next.n = st.cap;
        st.next.gen = 0;
    }
    if (++st.next.gen == 0) st.next.gen = 1;
    return st;
}

// ---- the passes of one rank -----------------------------------------------------------------------------------------------
enum class ApplyPass : uint8_t {
    kClaim,           // k_apply_claim           a lane per pod, blocks of 256
    kClaimMerge,      // k_apply_claim_merge     a lane per node, blocks of 256
    kAccumulate,      // k_apply_accumulate      a lane per pod, blocks of 256
    kKeys,            // k_apply_keys            a lane per pod, blocks of 256
    kSort,            // ApplyRankPlan::sort     (grid: that of its first step)
    kCommitLocal,     // k_apply_commit          a block of kApplyTileNodes per tile
    kCommitGathered,  // k_apply_commit_gathered a block of kApplyTileNodes per tile
    kCommitAdmit,     // k_apply_admit           a wave per node, four to a block of 256
    kReindex,         // k_build_tile_fit over the dirty tiles (launch_build_fit sizes it; grid here: the tiles)
    kStatus,          // k_apply_status          a lane per pod, blocks of 256
};
struct ApplyLaunch {
    ApplyPass pass;
    uint32_t grid;
};
// threads of a block of the pass's kernel (kSort and kReindex size their own launches)
constexpr uint32_t apply_pass_block(ApplyPass pass) {
    return pass == ApplyPass::kCommitLocal || pass == ApplyPass::kCommitGathered ? kApplyTileNodes : 256u;
}

constexpr uint32_t apply_pod_grid(uint32_t p) { return std::min<uint32_t>((p + 255u) / 256u, 2048u); }

struct ApplyFacts {
    uint32_t flags = 0;
    bool comm = false;
    uint32_t nranks = 1;
    uint32_t n = 0;  // nodes of the snapshot (every rank holds a replica)
};
struct ApplyRankFacts {
    uint32_t rows = 0;     // the rank's pods
    bool status = false;   // status_out given
    bool indexed = false;  // the rank's snapshot has a bitmap index
};

constexpr int kApplyPhases = 3, kApplyMaxLaunches = 6;
struct ApplyRankPlan {
    bool admit = false;    // KSCHED_APPLY_WHILE_FIT: keys, sort and admit in place of accumulate, commit and status
    bool refused = false;  // ... with more rows than the sort takes (kSortMaxRecords): KSCHED_E_INVAL before anything changes
    // the sort's two sets hold `admit_rows` records each; when they do not, they are regrown to admit_cap -- BEFORE the change begins, so
    // that a failed allocation leaves the snapshot as it was
    size_t admit_rows = 0, admit_cap = 0;
    uint32_t tiles = 0;
    size_t gather_elems = 0;  // with a communicator, uint64 elements of the receive buffer: [nranks][n][4] (the claims [nranks][n] uint32 fit)
    // the launches in order; phase f is launch[phase_end[f - 1] .. phase_end[f])
    ApplyLaunch launch[kApplyMaxLaunches];
    uint8_t phase_end[kApplyPhases] = {};
    SortPlan sort;  // of the kSort pass, if there is one
    const ApplyLaunch *begin(int phase) const { return launch + (phase ? phase_end[phase - 1] : 0); }
    const ApplyLaunch *end(int phase) const { return launch + phase_end[phase]; }
};

inline ApplyRankPlan plan_apply_rank(const ApplyFacts &f, const ApplyRankFacts &r) {
    ApplyRankPlan pl;
    const uint32_t n = f.n, p = r.rows;
    const bool fpn = (f.flags & KSCHED_APPLY_FIRST_PER_NODE) != 0u;
    pl.admit = (f.flags & KSCHED_APPLY_WHILE_FIT) != 0u;
    pl.tiles = (n + kApplyTileNodes - 1u) / kApplyTileNodes;
    if (f.comm) pl.gather_elems = (size_t)f.nranks * n * 4;
    if (pl.admit) {
        pl.refused = p > kSortMaxRecords;
        if (pl.refused) return pl;
        pl.admit_rows = p;
        pl.admit_cap = std::max<size_t>((size_t)p + p / 4, 1024);
    }
    uint8_t k = 0;
    auto add = [&](ApplyPass pass, uint32_t grid) { pl.launch[k++] = ApplyLaunch{pass, grid}; };
    // phase 0
    if (fpn && p > 0 && n > 0) add(ApplyPass::kClaim, apply_pod_grid(p));
    pl.phase_end[0] = k;
    // phase 1
    if (pl.admit) {
        if (p > 0) {
            add(ApplyPass::kKeys, apply_pod_grid(p));
            if (n > 0) {  // (else every pod is UNBOUND or BAD_NODE: final)
                pl.sort = plan_merge_sort(p, false, SortInto::kScratch);
                add(ApplyPass::kSort, pl.sort.steps[0].grid);
            }
        }
    } else {
        if (f.comm && fpn && n > 0) add(ApplyPass::kClaimMerge, std::min<uint32_t>((n + 255u) / 256u, 1024u));
        if (p > 0) add(ApplyPass::kAccumulate, apply_pod_grid(p));
    }
    pl.phase_end[1] = k;
    // phase 2
    if (pl.tiles > 0) {
        if (pl.admit) {
            if (p > 0) add(ApplyPass::kCommitAdmit, (n + 3u) / 4u);
        } else if (f.comm) add(ApplyPass::kCommitGathered, pl.tiles);
        else add(ApplyPass::kCommitLocal, pl.tiles);
        // only the dirty tiles are re-indexed: every tile's block reads its generation and the clean ones exit
        if (r.indexed) add(ApplyPass::kReindex, pl.tiles);
        // (every status but OVERFLOW is final after the accumulate pass; with no node, all of them)
        if (!pl.admit && r.status && p > 0) add(ApplyPass::kStatus, apply_pod_grid(p));
    }
    pl.phase_end[2] = k;
    return pl;
}

// ---- the collectives of the call, in 32-bit words per rank (0: not run) -------------------------------------------------------
struct ApplyGathers {
    size_t claims_words = 0;  // behind phase 0: every rank's claim[n]
    size_t sums_words = 0;    // behind phase 1: every rank's acc[n][4] split sums, 8 words per node
};
inline ApplyGathers plan_apply_gathers(const ApplyFacts &f) {
    ApplyGathers g;
    if (f.comm && (f.flags & KSCHED_APPLY_FIRST_PER_NODE) && f.n > 0) g.claims_words = f.n;
    if (f.comm && f.n > 0) g.sums_words = (size_t)f.n * 8;
    return g;
}

}  // namespace ksched
