// apply_plan_tests.cpp -- host-side check of what an apply call does (csrc/apply_plan.hpp), no GPU and no HIP.
//
// (a) The five functions that decided a call between them before the header (apply_begin, apply_admit_sort, apply_accumulate,
//     apply_finish, apply_run, with apply_scratch_ready, admit_scratch_ready, apply_flags_check and sharded_check), transcribed literally
//     over a fake ctx that logs every allocation, memset, launch and collective.  Every combination of flags 0 .. 15 x communicator x
//     nranks {1, 3} x n {0, 1, 1024, 1025} x rows {0, 1, 1025} x status_out x index x three states the scratch may be in runs through
//     them and through an executor of the plan shaped as ksched_api.hip's: the same verdict and the same log, line by line.
// (b) The scratch step by itself: the first call, a smaller snapshot (kept), a larger one (reallocated, the generation restarts),
//     invalidate() and the generation's wrap past 0.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/apply_plan.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

using Log = std::vector<std::string>;
static void note(Log &log, const char *fmt, ...) {
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    log.emplace_back(buf);
}

// a DevBuf that allocates nothing: reserve() grows to exactly n, as DevBuf does, and says so
struct FakeBuf {
    size_t cap = 0;
    void reserve(Log &log, int rank, const char *name, size_t n) {
        if (n <= cap) return;
        cap = n;
        note(log, "r%d malloc %s %zu", rank, name, n);
    }
};

// ---- (a) the code as it was ----------------------------------------------------------------------------------------------
constexpr int kOldTileNodes = 1024;
constexpr uint32_t kOldUnclaimed = 0xFFFFFFFFu;
struct OldCtx {
    int rank = 0;
    uint32_t n = 0;
    bool idx_built = false;
    FakeBuf apply_acc, apply_claim, apply_ovf, apply_dirty, apply_gath, admit_k0[2], admit_idx[2];
    uint32_t apply_n = 0, apply_gen = 0;
    Log *log = nullptr;
};
struct OldComm {
    int nranks = 1, rank = 0;
};
struct OldApplyArgs {
    bool status = false;
    uint32_t p = 0, n = 0, tiles = 0, gen = 0, first_per_node = 0, release = 0;
};
struct OldAdmitArgs {
    uint32_t p = 0, n = 0, tiles = 0, gen = 0;
    int keys_set = -1, sorted_set = -1;  // which admit set the keys are written to and which the admit reads
};
struct OldCall {
    OldCtx *c = nullptr;
    OldComm *q = nullptr;
    uint32_t count = 0;
    OldApplyArgs a{};
    bool admit = false;
    OldAdmitArgs w{};
};
static void old_launch(OldCtx *c, const char *kernel, uint32_t grid, uint32_t block, uint32_t gen) {
    note(*c->log, "r%d %s <<<%u, %u>>> gen %u", c->rank, kernel, grid, block, gen);
}
static uint32_t old_pod_grid(uint32_t p) { return std::min<uint32_t>((p + 255u) / 256u, 2048u); }

static void old_apply_scratch_ready(OldCtx *c) {
    const uint32_t n = c->n;
    if (c->apply_n == 0 || n > c->apply_n) {
        c->apply_n = 0;
        const uint32_t cap = std::max<uint32_t>(n, 1024u), cap_tiles = (cap + kOldTileNodes - 1) / kOldTileNodes;
        c->apply_acc.reserve(*c->log, c->rank, "acc", (size_t)cap * 4);
        c->apply_claim.reserve(*c->log, c->rank, "claim", cap);
        c->apply_ovf.reserve(*c->log, c->rank, "ovf", cap);
        c->apply_dirty.reserve(*c->log, c->rank, "dirty", cap_tiles + 1u);
        note(*c->log, "r%d memset acc 0x00 %zu", c->rank, (size_t)cap * 32);
        note(*c->log, "r%d memset claim 0xFF %zu", c->rank, (size_t)cap * 4);
        note(*c->log, "r%d memset dirty 0x00 %zu", c->rank, (size_t)(cap_tiles + 1u) * 4);
        c->apply_n = cap;
        c->apply_gen = 0;
    }
    if (++c->apply_gen == 0) c->apply_gen = 1;
}
static int old_apply_flags_check(uint32_t flags) {
    if (flags & ~(KSCHED_APPLY_FIRST_PER_NODE | KSCHED_APPLY_RELEASE | KSCHED_APPLY_WHILE_FIT)) return KSCHED_E_INVAL;
    if ((flags & KSCHED_APPLY_WHILE_FIT) && (flags & (KSCHED_APPLY_FIRST_PER_NODE | KSCHED_APPLY_RELEASE))) return KSCHED_E_INVAL;
    return KSCHED_OK;
}
static int old_admit_scratch_ready(OldCtx *c, uint32_t p) {
    if (p > (1u << 31)) return KSCHED_E_INVAL;
    if (p <= c->admit_k0[0].cap && p <= c->admit_k0[1].cap && p <= c->admit_idx[0].cap && p <= c->admit_idx[1].cap) return KSCHED_OK;
    const size_t cap = std::max<size_t>((size_t)p + p / 4, 1024);
    for (int i = 0; i < 2; ++i) {
        c->admit_k0[i].reserve(*c->log, c->rank, i ? "admit_k0[1]" : "admit_k0[0]", cap);
        c->admit_idx[i].reserve(*c->log, c->rank, i ? "admit_idx[1]" : "admit_idx[0]", cap);
    }
    return KSCHED_OK;
}
// (the parts of sharded_check that need no handle)
static int old_sharded_check(uint32_t count, uint32_t row_lo, uint32_t flags) {
    if (int rc = old_apply_flags_check(flags)) return rc;
    if (flags & KSCHED_APPLY_WHILE_FIT) return KSCHED_E_UNSUPPORTED;
    if ((uint64_t)row_lo + count > (uint64_t)kOldUnclaimed) return KSCHED_E_INVAL;
    return KSCHED_OK;
}
static int old_apply_begin(OldCall &x, uint32_t flags, bool status_out) {
    OldCtx *c = x.c;
    x.admit = (flags & KSCHED_APPLY_WHILE_FIT) != 0u;
    if (x.admit)
        if (int rc = old_admit_scratch_ready(c, x.count)) return rc;
    note(*c->log, "r%d change begins", c->rank);
    old_apply_scratch_ready(c);
    const uint32_t n = c->n;
    OldApplyArgs &a = x.a;
    a.status = status_out;
    a.p = x.count;
    a.n = n;
    a.tiles = (n + kOldTileNodes - 1) / kOldTileNodes;
    a.gen = c->apply_gen;
    a.first_per_node = (flags & KSCHED_APPLY_FIRST_PER_NODE) ? 1u : 0u;
    a.release = (flags & KSCHED_APPLY_RELEASE) ? 1u : 0u;
    if (x.q) c->apply_gath.reserve(*c->log, c->rank, "gath", (size_t)x.q->nranks * n * 4);
    if (a.first_per_node && a.p > 0 && n > 0) old_launch(c, "k_apply_claim", old_pod_grid(a.p), 256, a.gen);
    if (x.admit) {
        OldAdmitArgs &w = x.w;
        w.p = a.p;
        w.n = n;
        w.tiles = a.tiles;
        w.gen = a.gen;
    }
    return KSCHED_OK;
}
static int old_apply_admit_sort(OldCall &x) {
    OldCtx *c = x.c;
    OldAdmitArgs &w = x.w;
    const uint32_t p = w.p;
    if (p == 0) return KSCHED_OK;
    w.keys_set = 1;
    old_launch(c, "k_apply_keys", old_pod_grid(p), 256, w.gen);
    if (w.n == 0) return KSCHED_OK;
    note(*c->log, "r%d k_sort_runs <<<%u, 1024>>> run 0 in set 1 out set 0", c->rank, (p + 1023u) / 1024u);
    uint32_t set = 0;
    for (uint64_t run = 1024; run < p; run <<= 1) {
        const uint32_t in = set;
        set ^= 1u;
        note(*c->log, "r%d k_merge_pass <<<%u, 256>>> run %u in set %u out set %u", c->rank, (p + 255u) / 256u, (uint32_t)run, in, set);
    }
    w.sorted_set = (int)set;
    return KSCHED_OK;
}
static int old_apply_accumulate(OldCall &x) {
    OldCtx *c = x.c;
    if (x.q && x.a.first_per_node && x.a.n > 0)
        old_launch(c, "k_apply_claim_merge", std::min<uint32_t>((x.a.n + 255u) / 256u, 1024u), 256, x.a.gen);
    if (x.a.p > 0) old_launch(c, "k_apply_accumulate", old_pod_grid(x.a.p), 256, x.a.gen);
    return KSCHED_OK;
}
static int old_apply_finish(OldCall &x) {
    OldCtx *c = x.c;
    if (x.a.tiles > 0) {
        if (x.admit) {
            if (x.w.p > 0) {
                old_launch(c, "k_apply_admit", (x.w.n + 3u) / 4u, 256, x.w.gen);
                note(*c->log, "r%d admit reads set %d", c->rank, x.w.sorted_set);
            }
        } else if (x.q) old_launch(c, "k_apply_commit_gathered", x.a.tiles, kOldTileNodes, x.a.gen);
        else old_launch(c, "k_apply_commit", x.a.tiles, kOldTileNodes, x.a.gen);
        if (c->idx_built) note(*c->log, "r%d re-index of the dirty tiles", c->rank);
        if (!x.admit && x.a.status && x.a.p > 0) old_launch(c, "k_apply_status", old_pod_grid(x.a.p), 256, x.a.gen);
    }
    note(*c->log, "r%d change commits", c->rank);
    return KSCHED_OK;
}
static int old_apply_run(OldCall *v, int k, uint32_t flags, const bool *status_out, Log &log) {
    for (int i = 0; i < k; ++i)
        if (int rc = old_apply_begin(v[i], flags, status_out[i])) return rc;
    const uint32_t n = v[0].a.n;
    const bool comm = v[0].q != nullptr;
    if (comm && (flags & KSCHED_APPLY_FIRST_PER_NODE) && n > 0) note(log, "allgather claims %zu", (size_t)n);
    for (int i = 0; i < k; ++i)
        if (int rc = v[i].admit ? old_apply_admit_sort(v[i]) : old_apply_accumulate(v[i])) return rc;
    if (comm && n > 0) note(log, "allgather sums %zu", (size_t)n * 8);
    int rc = KSCHED_OK;
    for (int i = 0; i < k && !rc; ++i) rc = old_apply_finish(v[i]);
    return rc;
}

// ---- the executor of the plan, shaped as ksched_api.hip's (ApplyState, apply_begin, apply_launch, apply_finish, apply_run) -------------
struct NewCtx {
    int rank = 0;
    uint32_t n = 0;
    bool idx_built = false;
    FakeBuf acc, claim, ovf, dirty, gath, sort_k0[2], sort_idx[2];
    ApplyScratch scratch;
    Log *log = nullptr;
};
struct NewCall {
    NewCtx *c = nullptr;
    bool comm = false;
    uint32_t count = 0;
    ApplyRankPlan plan;
    uint32_t gen = 0;
    int sorted_set = -1;
};
static const char *kernel_of(ApplyPass p) {
    switch (p) {
    case ApplyPass::kClaim: return "k_apply_claim";
    case ApplyPass::kClaimMerge: return "k_apply_claim_merge";
    case ApplyPass::kAccumulate: return "k_apply_accumulate";
    case ApplyPass::kKeys: return "k_apply_keys";
    case ApplyPass::kCommitLocal: return "k_apply_commit";
    case ApplyPass::kCommitGathered: return "k_apply_commit_gathered";
    case ApplyPass::kCommitAdmit: return "k_apply_admit";
    case ApplyPass::kStatus: return "k_apply_status";
    default: return "?";
    }
}
static int set_of(SortBuf b) { return b == SortBuf::kSet0 ? 0 : b == SortBuf::kSet1 ? 1 : -1; }
static void new_launch(NewCall &x, int phase) {
    NewCtx *c = x.c;
    for (const ApplyLaunch *l = x.plan.begin(phase); l != x.plan.end(phase); ++l) {
        if (l->pass == ApplyPass::kSort) {
            const SortPlan &s = x.plan.sort;
            CHECK(!s.refused && !s.second_key && l->grid == s.steps[0].grid);
            for (uint32_t i = 0; i < s.nsteps; ++i)
                note(*c->log, "r%d %s <<<%u, %u>>> run %u in set %d out set %d", c->rank, s.steps[i].kernel == SortKernel::kRuns ? "k_sort_runs" : "k_merge_pass",
                     s.steps[i].grid, s.steps[i].kernel == SortKernel::kRuns ? 1024u : 256u, s.steps[i].run, set_of(s.steps[i].in), set_of(s.steps[i].out));
            x.sorted_set = set_of(s.landing);
        } else if (l->pass == ApplyPass::kReindex) {
            CHECK(l->grid == x.plan.tiles);
            note(*c->log, "r%d re-index of the dirty tiles", c->rank);
        } else {
            note(*c->log, "r%d %s <<<%u, %u>>> gen %u", c->rank, kernel_of(l->pass), l->grid, apply_pass_block(l->pass), x.gen);
            if (l->pass == ApplyPass::kCommitAdmit) note(*c->log, "r%d admit reads set %d", c->rank, x.sorted_set);
        }
    }
}
static int new_apply_begin(NewCall &x, const ApplyFacts &f, bool status_out) {
    NewCtx *c = x.c;
    x.plan = plan_apply_rank(f, ApplyRankFacts{x.count, status_out, c->idx_built});
    if (x.plan.refused) return KSCHED_E_INVAL;
    if (x.plan.admit) {
        const size_t p = x.plan.admit_rows;
        if (!(p <= c->sort_k0[0].cap && p <= c->sort_k0[1].cap && p <= c->sort_idx[0].cap && p <= c->sort_idx[1].cap))  // SortScratch::holds
            for (int b = 0; b < 2; ++b) {                                                                            // SortScratch::reserve, no second key
                c->sort_k0[b].reserve(*c->log, c->rank, b ? "admit_k0[1]" : "admit_k0[0]", x.plan.admit_cap);
                c->sort_idx[b].reserve(*c->log, c->rank, b ? "admit_idx[1]" : "admit_idx[0]", x.plan.admit_cap);
            }
    }
    note(*c->log, "r%d change begins", c->rank);
    const ApplyScratchStep st = plan_apply_scratch(c->scratch, c->n);  // ApplyState::ready
    if (st.allocate) {
        c->acc.reserve(*c->log, c->rank, "acc", st.acc_elems);
        c->claim.reserve(*c->log, c->rank, "claim", st.claim_elems);
        c->ovf.reserve(*c->log, c->rank, "ovf", st.ovf_elems);
        c->dirty.reserve(*c->log, c->rank, "dirty", st.dirty_elems);
        note(*c->log, "r%d memset acc 0x00 %zu", c->rank, st.acc_bytes);
        note(*c->log, "r%d memset claim 0xFF %zu", c->rank, st.claim_bytes);
        note(*c->log, "r%d memset dirty 0x00 %zu", c->rank, st.dirty_bytes);
    }
    c->scratch = st.next;
    x.gen = c->scratch.gen;
    if (x.comm) c->gath.reserve(*c->log, c->rank, "gath", x.plan.gather_elems);
    new_launch(x, 0);
    return KSCHED_OK;
}
static int new_apply_run(NewCall *v, int k, const ApplyFacts &f, const bool *status_out, Log &log) {
    const ApplyGathers g = plan_apply_gathers(f);
    for (int i = 0; i < k; ++i)
        if (int rc = new_apply_begin(v[i], f, status_out[i])) return rc;
    if (g.claims_words) note(log, "allgather claims %zu", g.claims_words);
    for (int i = 0; i < k; ++i) new_launch(v[i], 1);
    if (g.sums_words) note(log, "allgather sums %zu", g.sums_words);
    for (int i = 0; i < k; ++i) {
        new_launch(v[i], 2);
        note(log, "r%d change commits", v[i].c->rank);
    }
    return KSCHED_OK;
}

// the states a ctx's scratch may be in when the call arrives: {apply_n, apply_gen, capacity of the admit's sets}
struct Before {
    uint32_t apply_n, apply_gen;
    size_t admit_cap;
};
static const Before kBefore[] = {{0, 0, 0}, {1024, 5, 1024}, {2048, 0xFFFFFFFFu, 2000}};
static const uint32_t kRows[] = {0u, 1u, 1025u}, kNodes[] = {0u, 1u, 1024u, 1025u};

static long check_against_old() {
    long combos = 0;
    for (uint32_t flags = 0; flags < 16; ++flags)
        for (int comm = 0; comm < 2; ++comm)
            for (int nranks : {1, 3})
                for (uint32_t n : kNodes)
                    for (int ri = 0; ri < 3; ++ri)
                        for (int status = 0; status < 2; ++status)
                            for (int index = 0; index < 2; ++index)
                                for (const Before &bf : kBefore) {
                                    ++combos;
                                    // the verdict: every entry point asks it before it takes a lock
                                    const int old_verdict = comm ? old_sharded_check(kRows[ri], 0, flags) : old_apply_flags_check(flags);
                                    CHECK(apply_flags_verdict(flags, comm != 0) == old_verdict);
                                    CHECK(apply_flags_check(flags) == old_apply_flags_check(flags));
                                    if (old_verdict != KSCHED_OK) continue;
                                    // rank 0 has the enumerated rows, status_out and index; the others of a clique the next ones round
                                    const int k = comm ? nranks : 1;
                                    Log old_log, new_log;
                                    OldCtx oc[3];
                                    NewCtx nc[3];
                                    OldComm oq[3];
                                    OldCall ov[3];
                                    NewCall nv[3];
                                    bool st[3];
                                    for (int i = 0; i < k; ++i) {
                                        const uint32_t rows = kRows[(ri + i) % 3];
                                        st[i] = ((status + i) & 1) != 0;
                                        const bool built = ((index + i) & 1) != 0;
                                        oc[i].rank = nc[i].rank = i;
                                        oc[i].n = nc[i].n = n;
                                        oc[i].idx_built = nc[i].idx_built = built;
                                        oc[i].log = &old_log;
                                        nc[i].log = &new_log;
                                        oc[i].apply_n = nc[i].scratch.n = bf.apply_n;
                                        oc[i].apply_gen = nc[i].scratch.gen = bf.apply_gen;
                                        if (bf.apply_n) {  // (what the call that left that state reserved)
                                            const size_t tiles = (bf.apply_n + 1023u) / 1024u;
                                            oc[i].apply_acc.cap = nc[i].acc.cap = (size_t)bf.apply_n * 4;
                                            oc[i].apply_claim.cap = nc[i].claim.cap = oc[i].apply_ovf.cap = nc[i].ovf.cap = bf.apply_n;
                                            oc[i].apply_dirty.cap = nc[i].dirty.cap = tiles + 1;
                                        }
                                        for (int b = 0; b < 2; ++b)
                                            oc[i].admit_k0[b].cap = oc[i].admit_idx[b].cap = nc[i].sort_k0[b].cap = nc[i].sort_idx[b].cap = bf.admit_cap;
                                        oq[i].nranks = nranks;
                                        oq[i].rank = i;
                                        ov[i].c = &oc[i];
                                        ov[i].q = comm ? &oq[i] : nullptr;
                                        ov[i].count = nv[i].count = rows;
                                        nv[i].c = &nc[i];
                                        nv[i].comm = comm != 0;
                                    }
                                    ApplyFacts f;
                                    f.flags = flags;
                                    f.comm = comm != 0;
                                    f.nranks = comm ? (uint32_t)nranks : 1u;
                                    f.n = n;
                                    const int old_rc = old_apply_run(ov, k, flags, st, old_log);
                                    const int new_rc = new_apply_run(nv, k, f, st, new_log);
                                    CHECK(old_rc == new_rc);
                                    const bool same = old_log == new_log;
                                    CHECK(same);
                                    if (!same && g_fail < 4) {
                                        std::printf("flags %u comm %d nranks %d n %u rows %u status %d index %d\n", flags, comm, nranks, n, kRows[ri], status, index);
                                        for (const std::string &l : old_log) std::printf("  old: %s\n", l.c_str());
                                        for (const std::string &l : new_log) std::printf("  new: %s\n", l.c_str());
                                    }
                                    for (int i = 0; i < k; ++i) {
                                        CHECK(oc[i].apply_n == nc[i].scratch.n && oc[i].apply_gen == nc[i].scratch.gen);
                                        CHECK(nv[i].plan.tiles == ov[i].a.tiles);
                                    }
                                }
    return combos;
}

// ---- the answers the table of DESIGN.md section 7a states, written out ----------------------------------------------------------
static std::vector<ApplyPass> passes_of(const ApplyRankPlan &pl, int phase) {
    std::vector<ApplyPass> v;
    for (const ApplyLaunch *l = pl.begin(phase); l != pl.end(phase); ++l) v.push_back(l->pass);
    return v;
}
static void check_named_cases() {
    using P = ApplyPass;
    ApplyFacts f;
    f.n = 1025;
    // a FIRST_PER_NODE sharded call, a rank with an empty shard: no claim, no accumulate, no status -- but the claim merge, the gathered
    // commit and the re-index, and both collectives
    f.flags = KSCHED_APPLY_FIRST_PER_NODE;
    f.comm = true;
    f.nranks = 3;
    ApplyRankPlan pl = plan_apply_rank(f, ApplyRankFacts{0, true, true});
    CHECK(passes_of(pl, 0).empty());
    CHECK(passes_of(pl, 1) == std::vector<P>{P::kClaimMerge});
    CHECK((passes_of(pl, 2) == std::vector<P>{P::kCommitGathered, P::kReindex}));
    CHECK(pl.launch[0].grid == 5u && pl.launch[1].grid == 2u && pl.tiles == 2u && pl.gather_elems == 3u * 1025u * 4u);
    CHECK(plan_apply_gathers(f).claims_words == 1025u && plan_apply_gathers(f).sums_words == 8200u);
    // ... and a rank with rows
    pl = plan_apply_rank(f, ApplyRankFacts{1025, true, false});
    CHECK(passes_of(pl, 0) == std::vector<P>{P::kClaim});
    CHECK((passes_of(pl, 1) == std::vector<P>{P::kClaimMerge, P::kAccumulate}));
    CHECK((passes_of(pl, 2) == std::vector<P>{P::kCommitGathered, P::kStatus}));
    // over an empty snapshot only the pass that reports every pod UNBOUND or BAD_NODE runs: accumulate, or WHILE_FIT's keys
    f = ApplyFacts{};
    pl = plan_apply_rank(f, ApplyRankFacts{1025, true, true});
    CHECK(passes_of(pl, 0).empty() && passes_of(pl, 2).empty());
    CHECK(passes_of(pl, 1) == std::vector<P>{P::kAccumulate});
    f.flags = KSCHED_APPLY_WHILE_FIT;
    pl = plan_apply_rank(f, ApplyRankFacts{1025, true, true});
    CHECK(passes_of(pl, 1) == std::vector<P>{P::kKeys} && passes_of(pl, 2).empty());
    // WHILE_FIT over nodes: keys, sort, admit, re-index; 1025 pods take one merge pass and land in set 1
    f.n = 1024;
    pl = plan_apply_rank(f, ApplyRankFacts{1025, true, true});
    CHECK((passes_of(pl, 1) == std::vector<P>{P::kKeys, P::kSort}));
    CHECK((passes_of(pl, 2) == std::vector<P>{P::kCommitAdmit, P::kReindex}));
    CHECK(pl.sort.passes == 1u && pl.sort.landing == SortBuf::kSet1 && pl.admit_cap == 1281u && pl.launch[2].grid == 256u);
    // more pods than the sort takes
    pl = plan_apply_rank(f, ApplyRankFacts{(1u << 31) + 1u, false, false});
    CHECK(pl.refused && pl.phase_end[2] == 0);
    CHECK(!plan_apply_rank(f, ApplyRankFacts{1u << 31, false, false}).refused);
    f.flags = 0;
    CHECK(!plan_apply_rank(f, ApplyRankFacts{(1u << 31) + 1u, false, false}).refused);
    // the bound of the global pod indexes
    for (uint64_t lo : {0ull, 1ull, 0x7FFFFFFFull, 0xFFFFFFFEull, 0xFFFFFFFFull})
        for (uint64_t cnt : {0ull, 1ull, 2ull, 0x80000000ull, 0xFFFFFFFFull}) {
            CHECK(apply_rows_in_range((uint32_t)lo, (uint32_t)cnt) == (old_sharded_check((uint32_t)cnt, (uint32_t)lo, 0) == KSCHED_OK));
            CHECK(apply_rows_in_range((uint32_t)lo, (uint32_t)cnt) == (lo + cnt <= 0xFFFFFFFFull));
        }
}

// ---- (b) the scratch step ---------------------------------------------------------------------------------------------------
static void check_scratch_step() {
    ApplyScratch s;
    // the first call: allocated for max(n, 1024) nodes, generation 1
    ApplyScratchStep st = plan_apply_scratch(s, 5000);
    CHECK(st.allocate && st.cap == 5000u && st.cap_tiles == 5u);
    CHECK(st.acc_elems == 20000u && st.claim_elems == 5000u && st.ovf_elems == 5000u && st.dirty_elems == 6u);
    CHECK(st.acc_bytes == 160000u && st.claim_bytes == 20000u && st.dirty_bytes == 24u);
    CHECK(st.next.n == 5000u && st.next.gen == 1u);
    s = st.next;
    // a smaller snapshot: kept, the next generation
    st = plan_apply_scratch(s, 100);
    CHECK(!st.allocate && st.next.n == 5000u && st.next.gen == 2u);
    s = st.next;
    st = plan_apply_scratch(s, 5000);
    CHECK(!st.allocate && st.next.n == 5000u && st.next.gen == 3u);
    s = st.next;
    // a larger one: reallocated, the generation restarts
    st = plan_apply_scratch(s, 5001);
    CHECK(st.allocate && st.cap == 5001u && st.cap_tiles == 5u && st.next.n == 5001u && st.next.gen == 1u);
    s = st.next;
    // a change that stopped halfway: the next call allocates and memsets again, whatever the size
    s.invalidate();
    CHECK(s.n == 0u);
    st = plan_apply_scratch(s, 10);
    CHECK(st.allocate && st.cap == 1024u && st.cap_tiles == 1u && st.dirty_bytes == 8u && st.next.n == 1024u && st.next.gen == 1u);
    // an empty snapshot needs the scratch too
    st = plan_apply_scratch(ApplyScratch{}, 0);
    CHECK(st.allocate && st.cap == 1024u && st.next.gen == 1u);
    // the generation never takes 0, the initial value of every tile's entry
    s = ApplyScratch{};
    s.n = 1024;
    s.gen = 0xFFFFFFFEu;
    st = plan_apply_scratch(s, 1024);
    CHECK(!st.allocate && st.next.gen == 0xFFFFFFFFu);
    st = plan_apply_scratch(st.next, 1024);
    CHECK(!st.allocate && st.next.gen == 1u && st.next.n == 1024u);
}

int main() {
    const long combos = check_against_old();
    check_named_cases();
    check_scratch_step();
    std::printf("%ld combinations against the functions as they were, %d failed check(s)\n", combos, g_fail);
    return g_fail ? 1 : 0;
}
