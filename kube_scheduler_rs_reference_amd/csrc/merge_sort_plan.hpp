// merge_sort_plan.hpp -- the passes and buffers of one device merge sort (kernels_build.hpp: k_sort_runs + k_merge_pass), said once:
// how many merge passes n records take, which kernel each step launches over which grid with which run length, which buffer it
// reads and which it writes, and where the sorted keys and indices end up.
//
// Host-only on purpose, like eval_plan.hpp and pipe_plan.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/merge_sort_plan_tests.cpp executes every plan on the CPU, with the set a pass does not write poisoned, without a GPU.
// launch_merge_sort (ksched_api.hip) walks a plan over a SortScratch and takes no decision of its own; the two users are the
// best-fit orders (bestfit_sort: the snapshot's columns -> the arrays the pick kernels read) and KSCHED_APPLY_WHILE_FIT
// (plan_apply_rank in apply_plan.hpp: the keys k_apply_keys left in set 1 -> whichever set the last pass writes).
//
// Buffers are identities, not pointers.  Step 0 (k_sort_runs) sorts every run of kSortRun records from the source into set 0; merge
// pass i = 1 .. passes merges runs of kSortRun << (i - 1) from the set pass i - 1 wrote into set i & 1 -- except that a sort with a
// caller-named destination lands its LAST step's first key and indices there (the second key of that step still goes to set
// passes & 1: nobody reads it, but the kernel writes it).  So every step reads one buffer and writes another, and every step but
// the first reads what the step before it wrote.
#pragma once

#include <cstdint>

namespace ksched {

constexpr uint32_t kSortRun = 1024;                // records k_sort_runs sorts per block, in LDS
constexpr uint32_t kSortMaxRecords = 1u << 31;     // the merge passes index records with 32 bits and double `run` without wrapping up to here
constexpr uint32_t kSortMaxSteps = 22;             // the runs + ceil(log2(2^31 / 1024)) = 21 merge passes

// merge passes behind the runs of kSortRun: ceil(log2(n / kSortRun)), 0 up to one run
constexpr uint32_t merge_passes(uint64_t n) {
    uint32_t passes = 0;
    for (uint64_t run = kSortRun; run < n; run <<= 1) ++passes;
    return passes;
}

enum class SortBuf : uint8_t {
    kNone,     // (a second key that is absent)
    kColumns,  // the caller's input columns, read by step 0 only; idx = position
    kSet0,
    kSet1,     // the scratch's two sets of (k0, k1, idx)
    kDest,     // the caller's destination arrays (k0, idx)
};
enum class SortKernel : uint8_t { kRuns, kMerge };
enum class SortInto : uint8_t {
    kDest,     // from the caller's columns into the caller's destination arrays (best fit)
    kScratch,  // from the first key in set 1 (idx = position), staying in the scratch (the admit)
};

constexpr SortBuf sort_set(uint32_t i) { return (i & 1u) ? SortBuf::kSet1 : SortBuf::kSet0; }

struct SortStep {
    SortKernel kernel = SortKernel::kRuns;
    uint32_t run = 0;    // kMerge: records of one input run (SortArgs::run); kRuns: 0
    uint32_t grid = 0;   // blocks, of kSortRun threads (kRuns) or 256 (kMerge)
    SortBuf in = SortBuf::kNone;      // k0_in and, with a second key, k1_in; idx_in too unless kRuns (idx = position)
    SortBuf out = SortBuf::kNone;     // k0_out and idx_out
    SortBuf k1_out = SortBuf::kNone;  // kNone without a second key; else always a scratch set
};

struct SortPlan {
    bool refused = false;  // more than kSortMaxRecords records: nothing may be launched
    uint32_t n = 0;
    bool second_key = false;
    uint32_t passes = 0;
    uint32_t nsteps = 0;   // 1 + passes
    SortStep steps[kSortMaxSteps];
    SortBuf landing = SortBuf::kNone;  // where the sorted first keys and indices are once the last step has run
};

inline SortPlan plan_merge_sort(uint32_t n, bool second_key, SortInto into) {
    SortPlan pl;
    pl.n = n;
    pl.second_key = second_key;
    if (n > kSortMaxRecords) {
        pl.refused = true;
        return pl;
    }
    pl.passes = merge_passes(n);
    pl.nsteps = 1u + pl.passes;
    for (uint32_t i = 0; i <= pl.passes; ++i) {
        SortStep &st = pl.steps[i];
        const bool last = i == pl.passes;
        if (i == 0) {
            st.kernel = SortKernel::kRuns;
            st.grid = (n + kSortRun - 1u) / kSortRun;
            st.in = into == SortInto::kDest ? SortBuf::kColumns : SortBuf::kSet1;
        } else {
            st.kernel = SortKernel::kMerge;
            st.run = kSortRun << (i - 1u);
            st.grid = (n + 255u) / 256u;
            st.in = sort_set(i - 1u);
        }
        st.out = last && into == SortInto::kDest ? SortBuf::kDest : sort_set(i);
        st.k1_out = second_key ? sort_set(i) : SortBuf::kNone;
    }
    pl.landing = pl.steps[pl.passes].out;
    return pl;
}

// ---- identities -> addresses: the pointer members of a step's SortArgs (kernels_build.hpp), from the arrays behind the names ------
struct SortBuffers {
    int64_t *set_k0[2] = {}, *set_k1[2] = {};  // set_k1: only a sort with a second key touches it
    uint32_t *set_idx[2] = {};
    const int64_t *col_k0 = nullptr, *col_k1 = nullptr;  // SortInto::kDest
    int64_t *dst_k0 = nullptr;
    uint32_t *dst_idx = nullptr;
};
struct SortPtrs {
    const int64_t *k0_in = nullptr, *k1_in = nullptr;  // k1_in == nullptr: the records have no second key
    const uint32_t *idx_in = nullptr;                  // nullptr: idx = position (the runs)
    int64_t *k0_out = nullptr, *k1_out = nullptr;
    uint32_t *idx_out = nullptr;
};
inline SortPtrs sort_step_ptrs(const SortPlan &pl, const SortStep &st, const SortBuffers &b) {
    SortPtrs q;
    if (st.in == SortBuf::kColumns) {
        q.k0_in = b.col_k0;
        q.k1_in = pl.second_key ? b.col_k1 : nullptr;
    } else {
        const int i = st.in == SortBuf::kSet1;
        q.k0_in = b.set_k0[i];
        q.k1_in = pl.second_key ? b.set_k1[i] : nullptr;
        if (st.kernel == SortKernel::kMerge) q.idx_in = b.set_idx[i];
    }
    const int o = st.out == SortBuf::kSet1;
    q.k0_out = st.out == SortBuf::kDest ? b.dst_k0 : b.set_k0[o];
    q.idx_out = st.out == SortBuf::kDest ? b.dst_idx : b.set_idx[o];
    if (st.k1_out != SortBuf::kNone) q.k1_out = b.set_k1[st.k1_out == SortBuf::kSet1];
    return q;
}

}  // namespace ksched
