// merge_sort_plan_tests.cpp -- host-side check of the device merge sort's plan (csrc/merge_sort_plan.hpp), no GPU and no HIP.
//
// (a) The shape of every plan: pass count, no step reads what it writes, every step reads what the step before it wrote, the caller's
//     columns are never written, the landing place is the last step's output.
// (b) Every plan up to 4097 records executed on the CPU over an emulation of the two kernels' contracts (k_sort_runs: every run of 1024
//     sorted; k_merge_pass: neighbouring runs merged by ranking), with everything of the scratch a step does not write poisoned when it
//     runs, against std::sort on (k0, k1, idx).
// (c) The two drivers ksched_api.hip had before the header (bestfit_sort, apply_admit_sort), transcribed literally: the same kernel,
//     run, grid and buffers step by step.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/merge_sort_plan.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static const uint32_t kSizes[] = {0u, 1u, 1023u, 1024u, 1025u, 2048u, 2049u, 4096u, 4097u, 50000u, 1u << 31};

// ceil(log2(n / 1024)) clamped at 0, without the header's loop: the smallest k with 1024 * 2^k >= n
static uint32_t passes_expected(uint64_t n) {
    uint32_t k = 0;
    while ((1024ull << k) < n) ++k;
    return k;
}

// ---- (a) -----------------------------------------------------------------------------------------------------------
static void check_shape(uint32_t n, bool second_key, SortInto into) {
    const SortPlan pl = plan_merge_sort(n, second_key, into);
    CHECK(!pl.refused);
    CHECK(pl.n == n && pl.second_key == second_key);
    CHECK(pl.passes == passes_expected(n));
    CHECK(pl.nsteps == pl.passes + 1u && pl.nsteps <= kSortMaxSteps);
    for (uint32_t i = 0; i < pl.nsteps; ++i) {
        const SortStep &st = pl.steps[i];
        CHECK((st.kernel == SortKernel::kRuns) == (i == 0));
        CHECK(st.run == (i == 0 ? 0u : 1024u << (i - 1u)));
        CHECK(st.grid == (i == 0 ? (uint32_t)(((uint64_t)n + 1023u) / 1024u) : (uint32_t)(((uint64_t)n + 255u) / 256u)));
        CHECK(st.in != st.out && st.in != st.k1_out);                         // no step reads a buffer it writes
        CHECK(st.out != SortBuf::kColumns && st.k1_out != SortBuf::kColumns);  // the caller's columns are never an output
        CHECK(st.in != SortBuf::kNone && st.in != SortBuf::kDest && st.out != SortBuf::kNone);
        CHECK((st.k1_out != SortBuf::kNone) == second_key);
        CHECK(st.k1_out == SortBuf::kNone || st.k1_out == SortBuf::kSet0 || st.k1_out == SortBuf::kSet1);
        if (i == 0) {
            CHECK(st.in == (into == SortInto::kDest ? SortBuf::kColumns : SortBuf::kSet1));  // the admit's keys start in set 1
        } else {  // every step reads what the previous one wrote
            CHECK(st.in == pl.steps[i - 1].out);
            if (second_key) CHECK(st.in == pl.steps[i - 1].k1_out);
        }
        if (i + 1 < pl.nsteps) CHECK(st.out == SortBuf::kSet0 || st.out == SortBuf::kSet1);  // (only the last step may land outside)
    }
    CHECK(pl.landing == pl.steps[pl.nsteps - 1].out);
    if (into == SortInto::kDest) CHECK(pl.landing == SortBuf::kDest);
    else CHECK(pl.landing == ((pl.passes & 1u) ? SortBuf::kSet1 : SortBuf::kSet0));
    // best fit's final second key is the scratch set nobody reads: not the one the last step reads
    if (second_key) CHECK(pl.steps[pl.nsteps - 1].k1_out == ((pl.passes & 1u) ? SortBuf::kSet1 : SortBuf::kSet0));
}

// ---- (b) the kernels' contracts on the CPU ---------------------------------------------------------------------------------
using Rec = std::tuple<int64_t, int64_t, uint32_t>;
constexpr int64_t kPoisonKey = INT64_MIN + 7;
constexpr uint32_t kPoisonIdx = 0xDEADBEEFu;

struct Arrays {
    std::vector<int64_t> set_k0[2], set_k1[2], col_k0, col_k1, dst_k0;
    std::vector<uint32_t> set_idx[2], dst_idx;
    explicit Arrays(uint32_t n) {
        for (int b = 0; b < 2; ++b) {
            set_k0[b].assign(n, kPoisonKey);
            set_k1[b].assign(n, kPoisonKey);
            set_idx[b].assign(n, kPoisonIdx);
        }
        col_k0.assign(n, 0);
        col_k1.assign(n, 0);
        dst_k0.assign(n, kPoisonKey);
        dst_idx.assign(n, kPoisonIdx);
    }
    SortBuffers buffers() {
        SortBuffers b;
        for (int i = 0; i < 2; ++i) {
            b.set_k0[i] = set_k0[i].data();
            b.set_k1[i] = set_k1[i].data();
            b.set_idx[i] = set_idx[i].data();
        }
        b.col_k0 = col_k0.data();
        b.col_k1 = col_k1.data();
        b.dst_k0 = dst_k0.data();
        b.dst_idx = dst_idx.data();
        return b;
    }
};

// one step: read the inputs as the kernel would, poison every scratch array the step does not write, then write
static void emulate_step(const SortPlan &pl, const SortStep &st, Arrays &a) {
    const SortBuffers b = a.buffers();
    const SortPtrs q = sort_step_ptrs(pl, st, b);
    const uint32_t n = pl.n;
    std::vector<Rec> in(n), out(n);
    for (uint32_t g = 0; g < n; ++g) in[g] = Rec(q.k0_in[g], q.k1_in ? q.k1_in[g] : 0, q.idx_in ? q.idx_in[g] : g);
    if (st.kernel == SortKernel::kRuns) {
        CHECK(q.idx_in == nullptr);
        out = in;
        for (uint32_t lo = 0; lo < n; lo += 1024u) std::sort(out.begin() + lo, out.begin() + std::min(n, lo + 1024u));
    } else {
        CHECK(q.idx_in != nullptr && st.run >= 1024u);
        const uint64_t span = 2ull * st.run;
        for (uint32_t g = 0; g < n; ++g) {  // by ranking: the place in the own run plus the records of the sibling run that come before
            const uint32_t base = (uint32_t)((g / span) * span), off = g - base;
            const bool in_a = off < st.run;
            const uint32_t b_lo = (uint32_t)std::min<uint64_t>(n, (uint64_t)base + st.run), b_hi = (uint32_t)std::min<uint64_t>(n, base + span);
            const uint32_t s_lo = in_a ? b_lo : base, s_hi = in_a ? b_hi : b_lo;
            const uint32_t before = (uint32_t)(std::lower_bound(in.begin() + s_lo, in.begin() + s_hi, in[g]) - (in.begin() + s_lo));
            out[base + (in_a ? off : off - st.run) + before] = in[g];
        }
    }
    for (int i = 0; i < 2; ++i) {
        if (q.k0_out != b.set_k0[i]) std::fill(a.set_k0[i].begin(), a.set_k0[i].end(), kPoisonKey);
        if (q.k1_out != b.set_k1[i]) std::fill(a.set_k1[i].begin(), a.set_k1[i].end(), kPoisonKey);
        if (q.idx_out != b.set_idx[i]) std::fill(a.set_idx[i].begin(), a.set_idx[i].end(), kPoisonIdx);
    }
    for (uint32_t g = 0; g < n; ++g) {
        q.k0_out[g] = std::get<0>(out[g]);
        if (q.k1_out) q.k1_out[g] = std::get<1>(out[g]);
        q.idx_out[g] = std::get<2>(out[g]);
    }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

static void check_execution(uint32_t n, bool second_key, SortInto into) {
    const SortPlan pl = plan_merge_sort(n, second_key, into);
    Arrays a(n);
    std::vector<Rec> expect(n);
    for (uint32_t g = 0; g < n; ++g) {  // tied k0, tied (k0, k1), distinct idx
        const int64_t k0 = (int64_t)(rnd() % 7u) - 3, k1 = second_key ? (int64_t)(rnd() % 3u) : 0;
        expect[g] = Rec(k0, k1, g);
        if (into == SortInto::kDest) {
            a.col_k0[g] = k0;
            a.col_k1[g] = k1;
        } else {
            a.set_k0[1][g] = k0;  // where k_apply_keys leaves them
        }
    }
    const std::vector<int64_t> col_k0 = a.col_k0, col_k1 = a.col_k1;
    std::sort(expect.begin(), expect.end());
    for (uint32_t i = 0; i < pl.nsteps; ++i) emulate_step(pl, pl.steps[i], a);
    const std::vector<int64_t> &k0 = pl.landing == SortBuf::kDest ? a.dst_k0 : a.set_k0[pl.landing == SortBuf::kSet1];
    const std::vector<uint32_t> &idx = pl.landing == SortBuf::kDest ? a.dst_idx : a.set_idx[pl.landing == SortBuf::kSet1];
    bool same = true;
    for (uint32_t g = 0; g < n; ++g) same = same && k0[g] == std::get<0>(expect[g]) && idx[g] == std::get<2>(expect[g]);
    CHECK(same);
    CHECK(a.col_k0 == col_k0 && a.col_k1 == col_k1);
}

// ---- (c) the drivers as they were, over pointers that are names ----------------------------------------------------------------
struct Launch {
    bool merge;
    uint32_t n, run, grid, block;
    const void *k0_in, *k1_in, *idx_in, *k0_out, *k1_out, *idx_out;
    bool operator==(const Launch &o) const {
        return merge == o.merge && n == o.n && run == o.run && grid == o.grid && block == o.block && k0_in == o.k0_in && k1_in == o.k1_in &&
               idx_in == o.idx_in && k0_out == o.k0_out && k1_out == o.k1_out && idx_out == o.idx_out;
    }
};
struct OldSortArgs {  // SortArgs of kernels_build.hpp
    const int64_t *k0_in, *k1_in;
    const uint32_t *idx_in;
    int64_t *k0_out, *k1_out;
    uint32_t *idx_out;
    uint32_t n, run;
};
static std::vector<Launch> g_log;
static void old_launch(bool merge, uint32_t grid, uint32_t block, const OldSortArgs &a) {
    g_log.push_back(Launch{merge, a.n, a.run, grid, block, a.k0_in, a.k1_in, a.idx_in, a.k0_out, a.k1_out, a.idx_out});
}
// one element per array is enough to give it an address
struct Names {
    int64_t srt_k0[2], srt_k1[2], col_k0, col_k1, dst_k0;
    uint32_t srt_idx[2], dst_idx;
    SortBuffers buffers() {
        SortBuffers b;
        for (int i = 0; i < 2; ++i) {
            b.set_k0[i] = &srt_k0[i];
            b.set_k1[i] = &srt_k1[i];
            b.set_idx[i] = &srt_idx[i];
        }
        b.col_k0 = &col_k0;
        b.col_k1 = &col_k1;
        b.dst_k0 = &dst_k0;
        b.dst_idx = &dst_idx;
        return b;
    }
};

// bestfit_sort as it was; returns false where it refused
static bool old_bestfit_sort(Names &bi, uint32_t n, const int64_t *k0, const int64_t *k1, int64_t *dst_k0, uint32_t *dst_idx) {
    uint32_t passes = 0;
    for (uint64_t run = 1024; run < n; run <<= 1) ++passes;  // (bf_order_layout's loop, as it was)
    if (n > (1u << 31)) return false;
    auto out_of = [&](uint32_t i, OldSortArgs &q) {
        q.k0_out = i == passes ? dst_k0 : &bi.srt_k0[i & 1];
        q.k1_out = k1 ? &bi.srt_k1[i & 1] : nullptr;
        q.idx_out = i == passes ? dst_idx : &bi.srt_idx[i & 1];
    };
    OldSortArgs q{};
    q.n = n;
    q.k0_in = k0;
    q.k1_in = k1;
    out_of(0, q);
    old_launch(false, (n + 1023u) / 1024u, 1024, q);
    for (uint32_t i = 1; i <= passes; ++i) {
        OldSortArgs m{};
        m.n = n;
        m.run = 1024u << (i - 1u);
        m.k0_in = q.k0_out;
        m.k1_in = q.k1_out;
        m.idx_in = q.idx_out;
        out_of(i, m);
        old_launch(true, (n + 255u) / 256u, 256, m);
        q = m;
    }
    return true;
}

// the sort of apply_admit_sort as it was, behind its k_apply_keys launch (keys = admit_k0[1]); admit_scratch_ready refused p > 2^31
// before it.  Returns where the last pass landed.
static bool old_admit_sort(Names &c, uint32_t p, const int64_t **w_k0, const uint32_t **w_idx) {
    if (p > (1u << 31)) return false;
    int64_t *keys = &c.srt_k0[1];
    OldSortArgs q{};
    q.n = p;
    q.k0_in = keys;
    q.k0_out = &c.srt_k0[0];
    q.idx_out = &c.srt_idx[0];
    old_launch(false, (p + 1023u) / 1024u, 1024, q);
    uint32_t set = 0;
    for (uint64_t run = 1024; run < p; run <<= 1) {
        OldSortArgs m{};
        m.n = p;
        m.run = (uint32_t)run;
        m.k0_in = &c.srt_k0[set];
        m.idx_in = &c.srt_idx[set];
        set ^= 1u;
        m.k0_out = &c.srt_k0[set];
        m.idx_out = &c.srt_idx[set];
        old_launch(true, (p + 255u) / 256u, 256, m);
    }
    *w_k0 = &c.srt_k0[set];
    *w_idx = &c.srt_idx[set];
    return true;
}

static std::vector<Launch> new_launches(const SortPlan &pl, const SortBuffers &b) {
    std::vector<Launch> v;
    for (uint32_t i = 0; i < pl.nsteps; ++i) {
        const SortStep &st = pl.steps[i];
        const SortPtrs q = sort_step_ptrs(pl, st, b);
        const bool merge = st.kernel == SortKernel::kMerge;
        v.push_back(Launch{merge, pl.n, st.run, st.grid, merge ? 256u : kSortRun, q.k0_in, q.k1_in, q.idx_in, q.k0_out, q.k1_out, q.idx_out});
    }
    return v;
}

static void check_against_old(uint32_t n) {
    Names nm{};
    const SortBuffers b = nm.buffers();
    for (int second = 0; second < 2; ++second) {
        g_log.clear();
        const bool ran = old_bestfit_sort(nm, n, &nm.col_k0, second ? &nm.col_k1 : nullptr, &nm.dst_k0, &nm.dst_idx);
        const SortPlan pl = plan_merge_sort(n, second != 0, SortInto::kDest);
        CHECK(ran == !pl.refused);
        if (ran) CHECK(new_launches(pl, b) == g_log);
        else CHECK(pl.nsteps == 0);
    }
    g_log.clear();
    const int64_t *w_k0 = nullptr;
    const uint32_t *w_idx = nullptr;
    const bool ran = old_admit_sort(nm, n, &w_k0, &w_idx);
    const SortPlan pl = plan_merge_sort(n, false, SortInto::kScratch);
    CHECK(ran == !pl.refused);
    if (ran) {
        CHECK(new_launches(pl, b) == g_log);
        CHECK(pl.landing == SortBuf::kSet0 || pl.landing == SortBuf::kSet1);
        CHECK(w_k0 == b.set_k0[pl.landing == SortBuf::kSet1] && w_idx == b.set_idx[pl.landing == SortBuf::kSet1]);
    } else CHECK(pl.nsteps == 0);
}

int main() {
    int plans = 0, executed = 0;
    for (uint32_t n : kSizes)
        for (int into = 0; into < 2; ++into)
            for (int second = 0; second < 2; ++second) {
                if (into == 1 && second) continue;  // (the admit has no second key; the plan would take one all the same, see below)
                check_shape(n, second != 0, into ? SortInto::kScratch : SortInto::kDest);
                ++plans;
                if (n <= 4097u) {
                    check_execution(n, second != 0, into ? SortInto::kScratch : SortInto::kDest);
                    ++executed;
                }
            }
    for (uint32_t n : kSizes) check_shape(n, true, SortInto::kScratch);  // a second key that stays in the scratch: the same shape
    // every size of a pass boundary's neighbourhood, executed
    for (uint32_t n = 1; n <= 4200u; n += (n % 1024u >= 1020u || n % 1024u <= 4u) ? 1u : 53u) {
        check_execution(n, true, SortInto::kDest);
        check_execution(n, false, SortInto::kScratch);
        executed += 2;
    }
    // the refusal: 2^31 records are taken, one more is not, and nothing is planned then
    for (int into = 0; into < 2; ++into)
        for (int second = 0; second < 2; ++second) {
            const SortPlan pl = plan_merge_sort((1u << 31) + 1u, second != 0, into ? SortInto::kScratch : SortInto::kDest);
            CHECK(pl.refused && pl.nsteps == 0 && pl.landing == SortBuf::kNone);
            CHECK(!plan_merge_sort(1u << 31, second != 0, into ? SortInto::kScratch : SortInto::kDest).refused);
        }
    CHECK(merge_passes(1u << 31) == 21u && merge_passes(50000u) == 6u && kSortMaxSteps == 22u);
    for (uint32_t n : kSizes) check_against_old(n);
    check_against_old((1u << 31) + 1u);
    for (uint32_t n = 0; n <= 70000u; n += 7u) check_against_old(n);
    std::printf("%d plans shaped, %d executed, %d failed check(s)\n", plans, executed, g_fail);
    return g_fail ? 1 : 0;
}
