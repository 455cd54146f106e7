// selterms_plan_tests.cpp -- host-side check of the rules of a tagged call with a term count (extension E10, KSCHED_SEL_TERMS:
// csrc/sel_terms.hpp, csrc/eval_plan.hpp), no GPU and no HIP: the constants and what they leave alone; every refusal and every accepted
// combination of check_selterms_args at its boundary; where entry (term, key, pod) lies and how many columns the host forms copy;
// selterms_row against seltag_row (one term IS the tagged row, T terms are the OR of T tagged rows, a zero term, a NEVER term, the case in
// which AND-of-ORs and OR-of-ANDs differ, padding bits); the launch geometry walked on the CPU as the two kernels walk it (every word below
// W of every row stored exactly once by ONE launch, no padding word ever, every key of every term read by exactly one pass of the wide
// kernel, eight keys at most by the other); the plan with the field; and that a request without the field gets the plan it got before the
// field existed (plan_eval_as_it_was below).  The expectations are written out here, not computed by the header.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/eval_plan.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/mask_combine_soft.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/sel_ops.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/sel_tags.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/sel_terms.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static bool is(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

static const uint32_t kTagged = 0x40000u, kField = 0x00F00000u;
static const uint32_t kExists = 0x4000u, kGt = 0x8000u, kLt = 0x10000u, kAny = 0x1C000u;
static const uint32_t kAnd = 0x200u, kOr = 0x400u, kAndNot = 0x800u, kSoft = 0x2000u;
static const uint32_t kNever = 0xFFFFFFFFu;
static const uint32_t kPicks[] = {0u, KSCHED_PICK_SAMPLED, KSCHED_PICK_BESTFIT, KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD, KSCHED_PICK_PACK};
enum : uint32_t { EQ = 0, NE = 1, EX = 2, AB = 3, GT = 4, LT = 5 };

static uint32_t ent(uint32_t tag, uint32_t id) { return (tag << 29) | id; }
static uint32_t terms(uint32_t t) { return t << 20; }

// ---- the constants ---------------------------------------------------------------------------------------------------------------------
static void the_field() {
    CHECK(KSCHED_SEL_TERMS_SHIFT == 20u && KSCHED_SEL_TERMS_MASK == kField && KSCHED_MAX_TERMS == 15u);
    CHECK(KSCHED_SEL_TERMS(1) == 0x100000u && KSCHED_SEL_TERMS(3) == 0x300000u && KSCHED_SEL_TERMS(15) == kField);
    // four adjacent bits outside every known flag and outside the values callers probe with as unknown
    CHECK(!(kField & (0x1FFu | 0xE00u | 0x2000u | 0x1C000u | kTagged | 0x1000u | 0x20000u | 0x80000u)));
    CHECK((KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_ANY | KSCHED_WANT_FIT_MASK) == 0x1FFu && KSCHED_COMBINE_ANY == 0xE00u && KSCHED_COMBINE_SOFT == 0x2000u);
    CHECK(KSCHED_SELOP_ANY == kAny && KSCHED_SELOP_TAGGED == kTagged && KSCHED_ABI_VERSION == 7u);
    for (uint32_t rest : {0u, 0x1FFu, 0xE00u, 0x2000u, 0x1000u, 0x20000u, 0x80000u, 0x1C000u, kTagged, 0xFF000000u}) {
        CHECK(sel_terms(rest) == 0u);
        for (uint32_t t = 1; t <= 15u; ++t) {
            const uint32_t w = rest | terms(t);
            CHECK(sel_terms(w) == t);
            // the field changes neither the operator of a word, nor its tagged reading, nor its combine op, nor its modifier
            CHECK(sel_op(w) == sel_op(rest) && sel_tagged(w) == sel_tagged(rest) && combine_op(w) == combine_op(rest) && combine_soft(w) == combine_soft(rest));
        }
    }
}

// ---- the refusals -----------------------------------------------------------------------------------------------------------------------
static void the_argument_rules() {
    const uint32_t ok = KSCHED_SEL | kTagged;
    for (uint32_t t : {1u, 2u, 14u, 15u}) {
        const uint32_t f = ok | terms(t);
        // accepted: a tagged call with the field; a combine op, the modifier and a pick beside them change nothing here
        CHECK(check_selterms_args(f, true, false) == KSCHED_OK);
        for (uint32_t comb : {kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
            for (uint32_t pick : kPicks) CHECK(check_selterms_args(f | comb | pick, true, false) == KSCHED_OK);
        // where it is not accepted (ksched_pipe_submit)
        CHECK(check_selterms_args(f, false, false) == KSCHED_E_INVAL);
        // the field without KSCHED_SELOP_TAGGED: a plain call, an operator call, no selector term at all
        CHECK(check_selterms_args(terms(t), true, false) == KSCHED_E_INVAL);
        CHECK(check_selterms_args(KSCHED_SEL | terms(t), true, false) == KSCHED_E_INVAL);
        CHECK(check_selterms_args(KSCHED_FIT | KSCHED_SEL | terms(t), true, false) == KSCHED_E_INVAL);
        for (uint32_t op : {kExists, kGt, kLt}) CHECK(check_selterms_args(KSCHED_SEL | op | terms(t), true, false) == KSCHED_E_INVAL);
        // ... hence without KSCHED_SEL, or beside an operator flag
        CHECK(check_selterms_args(kTagged | terms(t), true, false) == KSCHED_E_INVAL);
        for (uint32_t op : {kExists, kGt, kLt}) CHECK(check_selterms_args(f | op, true, false) == KSCHED_E_INVAL);
        // fit, taints and a fit mask
        CHECK(check_selterms_args(f | KSCHED_FIT, true, false) == KSCHED_E_INVAL);
        CHECK(check_selterms_args(f | KSCHED_TAINT, true, false) == KSCHED_E_INVAL);
        CHECK(check_selterms_args(f | KSCHED_WANT_FIT_MASK, true, false) == KSCHED_E_INVAL);
        CHECK(check_selterms_args(f | KSCHED_WANT_FIT_MASK, true, true) == KSCHED_E_INVAL);
        CHECK(check_selterms_args(f, true, true) == KSCHED_E_INVAL);
    }
    // field 0: whatever the rest says, this rule has nothing to say (the other rules are asked about the rest)
    for (uint32_t rest : {0u, ok, ok | KSCHED_FIT, KSCHED_SEL | kGt | kLt, kTagged, 0x80000u, 0x1000u})
        for (int accepted = 0; accepted < 2; ++accepted)
            for (int fit = 0; fit < 2; ++fit) CHECK(check_selterms_args(rest, accepted, fit) == KSCHED_OK);
    // a tagged call's own answer does not change
    CHECK(check_seltag_args(ok, true, false) == KSCHED_OK && check_seltag_args(ok | terms(3), true, false) == KSCHED_OK);
}

// ---- the layout -------------------------------------------------------------------------------------------------------------------------
static void the_layout() {
    CHECK(selterms_index(0, 0, 0, 8, 100) == 0u && selterms_index(0, 3, 7, 8, 100) == 307u);
    CHECK(selterms_index(1, 0, 0, 8, 100) == 800u && selterms_index(2, 5, 99, 8, 100) == (2u * 8u + 5u) * 100u + 99u);
    CHECK(selterms_index(1, 2, 3, 9, 120) == (9u + 2u) * 120u + 3u);  // ksched_eval_begin: sel_stride entries between columns
    CHECK(selterms_index(14, 31, 0xFFFFFFFEu, 32, 0xFFFFFFFFull) == (14ull * 32ull + 31ull) * 0xFFFFFFFFull + 0xFFFFFFFEull);  // 64-bit
    CHECK(selterms_columns(0, 8) == 8u && selterms_columns(1, 8) == 8u && selterms_columns(3, 8) == 24u && selterms_columns(15, 32) == 480u && selterms_columns(4, 0) == 0u);
}

// ---- one pod's row ----------------------------------------------------------------------------------------------------------------------
static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static void the_row_rule() {
    // by hand: two keys, four nodes.  zone = (1, 2, 1, 0), disk = (5, 5, 6, 6)
    const uint32_t lab[8] = {1, 2, 1, 0, 5, 5, 6, 6};
    uint64_t row = 0;
    {  // two terms that each pass a different node: (zone = 2) | (zone Absent): nodes 1 and 3
        const uint32_t sel[4] = {ent(EQ, 2), 0, ent(AB, 0), 0};  // [term][key][pod], p = 1
        selterms_row(lab, sel, 2, 2, 4, 1, 0, &row);
        CHECK(row == 0xAull);
    }
    {  // (zone = 1 & disk = 5) | (zone = 2 & disk = 6): node 0 alone -- where AND of ORs, (zone in {1, 2}) & (disk in {5, 6}), says nodes 0, 1, 2
        const uint32_t sel[4] = {ent(EQ, 1), ent(EQ, 5), ent(EQ, 2), ent(EQ, 6)};
        selterms_row(lab, sel, 2, 2, 4, 1, 0, &row);
        CHECK(row == 0x1ull);
    }
    {  // an all-zero term passes everywhere, wherever it stands; a NEVER term adds nothing
        const uint32_t a[6] = {0, 0, ent(EQ, 2), 0, kNever, 0}, b[6] = {ent(EQ, 2), 0, 0, kNever, 0, 0}, c[4] = {ent(EQ, 2), 0, 0, kNever};
        selterms_row(lab, a, 2, 3, 4, 1, 0, &row);
        CHECK(row == 0xFull);
        selterms_row(lab, b, 2, 3, 4, 1, 0, &row);
        CHECK(row == 0xFull);
        selterms_row(lab, c, 2, 2, 4, 1, 0, &row);
        CHECK(row == 0x2ull);
        const uint32_t d[4] = {kNever, 0, 0, ent(7, 3)};
        selterms_row(lab, d, 2, 2, 4, 1, 0, &row);
        CHECK(row == 0ull);
    }
    selterms_row(lab, nullptr, 2, 3, 4, 1, 0, &row);
    CHECK(row == 0xFull);  // no selectors: every node
    selterms_row(lab, lab, 0, 3, 4, 1, 0, &row);
    CHECK(row == 0xFull);  // no keys: every node
    // against seltag_row: T = 1 IS the tagged row; T terms are the OR of the T tagged rows; bits at or beyond n stay zero (NE, ABSENT)
    uint32_t seed = 0xE10u;
    unsigned differs_from_every_term = 0, and_of_ors_differs = 0;
    for (uint32_t n : {1u, 63u, 64u, 65u, 130u})
        for (uint32_t nkeys : {1u, 2u, 9u})
            for (uint32_t T : {1u, 2u, 3u, 15u}) {
                const uint32_t p = 5, W = (n + 63u) / 64u;
                std::vector<uint32_t> l((size_t)nkeys * n), s((size_t)T * nkeys * p);
                for (auto &v : l) v = lcg(seed) >> 29;  // ids 0 .. 7
                for (auto &e : s) {
                    const uint32_t r = lcg(seed) >> 24;
                    e = r < 100u ? 0u : r < 110u ? kNever : ent((r >> 1) % 6u, (lcg(seed) >> 29));
                }
                for (uint32_t pod = 0; pod < p; ++pod) {
                    std::vector<uint64_t> got(W), want(W, 0), one(W), ors((size_t)nkeys * W, 0), aoo(W, ~0ull);
                    bool equals_a_term = false;
                    selterms_row(l.data(), s.data(), nkeys, T, n, p, pod, got.data());
                    for (uint32_t t = 0; t < T; ++t) {
                        seltag_row(l.data(), s.data() + (size_t)t * nkeys * p, nkeys, n, p, pod, one.data());
                        for (uint32_t w = 0; w < W; ++w) want[w] |= one[w];
                        // the per-key (wrong) formula: OR over the terms key by key, then AND over the keys
                        for (uint32_t k = 0; k < nkeys; ++k) {
                            std::vector<uint32_t> only((size_t)nkeys * p, 0);
                            only[(size_t)k * p + pod] = s[((size_t)t * nkeys + k) * p + pod];
                            std::vector<uint64_t> r(W);
                            seltag_row(l.data(), only.data(), nkeys, n, p, pod, r.data());
                            for (uint32_t w = 0; w < W; ++w) ors[(size_t)k * W + w] |= r[w];
                        }
                    }
                    for (uint32_t t = 0; t < T; ++t) {
                        seltag_row(l.data(), s.data() + (size_t)t * nkeys * p, nkeys, n, p, pod, one.data());
                        equals_a_term = equals_a_term || one == want;
                    }
                    for (uint32_t k = 0; k < nkeys; ++k)
                        for (uint32_t w = 0; w < W; ++w) aoo[w] &= ors[(size_t)k * W + w];
                    CHECK(got == want);
                    if (n & 63u) CHECK(!(got[W - 1] >> (n & 63u)));
                    differs_from_every_term += !equals_a_term;
                    and_of_ors_differs += aoo != want;
                    if (T == 1) CHECK(equals_a_term);
                }
            }
    CHECK(differs_from_every_term > 20 && and_of_ors_differs > 20);  // the cases tell an OR of ANDs from one term and from an AND of ORs
}

// ---- the launch plan ----------------------------------------------------------------------------------------------------------------------
// every thread block walks as the kernels do; `seen` counts the stores into every word of a [p][pitch] buffer, `read` the loads of every
// selector entry's column (term, key) per pod tile
static void walk(uint32_t p, uint32_t W, uint32_t pitch, uint32_t nkeys, uint32_t T) {
    const SeltermsLaunch l = plan_selterms_launch(p, W, nkeys, T);
    const SelopLaunch o = plan_selop_launch(p, W, nkeys);  // the same geometry over columns and pod tiles, not restated
    CHECK(l.block == 256u && l.gx == o.gx && l.gy == o.gy && l.pod_tiles == o.pod_tiles && l.pod_tiles_per_block == o.pod_tiles_per_block);
    CHECK(l.gx == (W + 15u) / 16u && l.gy >= 1u && l.gy <= 2048u && l.pod_tiles == (p + 63u) / 64u);
    CHECK((uint64_t)l.gy * l.pod_tiles_per_block >= l.pod_tiles && (uint64_t)(l.gy - 1u) * l.pod_tiles_per_block < l.pod_tiles);
    CHECK(l.key_passes == (nkeys == 0 ? 1u : (nkeys + 7u) / 8u) && l.wide == (nkeys > 8u) && l.terms == (nkeys == 0 ? 1u : T));
    // the keys of a term: the narrow kernel reads keys [0, min(8, nkeys)) -- all of them, it runs only where nkeys <= 8 --; the wide one
    // reads keys [8 * pass, ...) in pass `pass`: every key by exactly one pass
    std::vector<uint8_t> key_seen(nkeys, 0);
    if (!l.wide) {
        for (uint32_t k = 0; k < 8u; ++k)
            if (k < nkeys) ++key_seen[k];
    } else {
        for (uint32_t pass = 0; pass < l.key_passes; ++pass) {
            const uint32_t key0 = pass * 8u;
            CHECK(key0 < nkeys);
            const uint32_t nk = nkeys - key0 < 8u ? nkeys - key0 : 8u;
            for (uint32_t k = 0; k < 8u; ++k)
                if (k < nk) ++key_seen[key0 + k];
        }
    }
    for (uint8_t s : key_seen) CHECK(s == 1);
    std::vector<uint8_t> seen((size_t)p * pitch, 0);
    for (uint32_t by = 0; by < l.gy; ++by)
        for (uint32_t bx = 0; bx < l.gx; ++bx)
            for (uint32_t wave = 0; wave < 4u; ++wave) {
                const uint32_t w0 = (bx * 4u + wave) * 4u;
                if (w0 >= W) continue;
                for (uint32_t t = 0; t < l.pod_tiles_per_block; ++t) {
                    const uint64_t first = (uint64_t)(by * l.pod_tiles_per_block + t) * 64u;
                    if (first >= p) break;
                    const uint32_t jmax = p - (uint32_t)first < 64u ? p - (uint32_t)first : 64u;
                    for (uint32_t lane = 0; lane < jmax; ++lane)  // ONE store per word, after all terms (and all passes) of the tile
                        for (uint32_t c = 0; c < 4u; ++c)
                            if (w0 + c < W) ++seen[((size_t)first + lane) * pitch + w0 + c];
                }
            }
    bool once = true, padding_alone = true;
    for (uint32_t r = 0; r < p; ++r)
        for (uint32_t w = 0; w < pitch; ++w) {
            const uint8_t s = seen[(size_t)r * pitch + w];
            if (w < W ? s != 1 : s != 0) (w < W ? once : padding_alone) = false;
        }
    CHECK(once);
    CHECK(padding_alone);
}

static void the_launch() {
    for (uint32_t p : {1u, 63u, 64u, 65u, 129u, 4097u})
        for (uint32_t W : {1u, 3u, 4u, 5u, 15u, 16u, 17u, 33u, 65u})  // each side of a wave's four columns and a block's sixteen
            for (uint32_t extra : {0u, 1u, 15u})
                for (uint32_t nkeys : {0u, 1u, 8u, 9u, 16u, 17u, 32u})
                    for (uint32_t T : {1u, 2u, 15u}) walk(p, W, W + extra, nkeys, T);
    SeltermsLaunch l = plan_selterms_launch(100000, 79, 8, 4);  // C3: 5 column blocks, 391 block rows of 4 tiles, one launch, the narrow kernel
    CHECK(l.gx == 5 && l.pod_tiles == 1563 && l.gy == 391 && l.pod_tiles_per_block == 4 && l.key_passes == 1 && !l.wide && l.terms == 4);
    l = plan_selterms_launch(64, 16, 32, 15);
    CHECK(l.gx == 1 && l.gy == 1 && l.pod_tiles_per_block == 1 && l.key_passes == 4 && l.wide && l.terms == 15);
    l = plan_selterms_launch(64, 16, 9, 2);
    CHECK(l.key_passes == 2 && l.wide);
    l = plan_selterms_launch(64, 16, 8, 2);
    CHECK(l.key_passes == 1 && !l.wide);
    l = plan_selterms_launch(64, 16, 0, 7);
    CHECK(l.key_passes == 1 && !l.wide && l.terms == 1);  // no keys: nothing to OR
    l = plan_selterms_launch(0, 5, 8, 2);
    CHECK(l.gx == 0 && l.gy == 0);  // nothing to launch
    l = plan_selterms_launch(5, 0, 8, 2);
    CHECK(l.gx == 0 && l.gy == 0);
    // the geometry the standing legs rely on (tests/apply_paths_worker.py case_sizes and the walks): 3000 pods over 50 000 and 60 000 nodes
    // with three terms -- 47 tiles, two a block, 24 block rows: 48 slots, so the last block breaks at `first >= p`; the narrow kernel --; a
    // walk's 2000 pods over 4097 nodes with ten keys: the wide kernel, two key passes, one tile a block; and the sizes case's one-node step
    l = plan_selterms_launch(3000, 782, 8, 3);
    CHECK(l.gx == 49 && l.pod_tiles == 47 && l.pod_tiles_per_block == 2 && l.gy == 24 && l.key_passes == 1 && !l.wide && l.terms == 3);
    l = plan_selterms_launch(3000, 938, 8, 3);
    CHECK(l.gx == 59 && l.pod_tiles == 47 && l.pod_tiles_per_block == 2 && l.gy == 24 && l.key_passes == 1 && !l.wide && l.terms == 3);
    l = plan_selterms_launch(2000, 65, 10, 3);
    CHECK(l.gx == 5 && l.pod_tiles == 32 && l.gy == 32 && l.pod_tiles_per_block == 1 && l.key_passes == 2 && l.wide && l.terms == 3);
    l = plan_selterms_launch(3000, 1, 8, 3);
    CHECK(l.gx == 1 && l.pod_tiles == 47 && l.gy == 47 && l.pod_tiles_per_block == 1 && l.key_passes == 1 && !l.wide && l.terms == 3);
    walk(3000, 782, 784, 8, 3);
    walk(2000, 65, 65, 10, 3);
    walk(3000, 1, 1, 8, 3);
    walk(2048u * 64u + 1u, 1, 1, 8, 2);  // one pod more than 2048 block rows of one tile: two tiles a block
    walk(3u * 2048u * 64u + 65u, 3, 4, 9, 3);
}

// ---- the plan with the field ----------------------------------------------------------------------------------------------------------------
static EvalFacts step(uint32_t flags, bool have_feas) {
    EvalFacts f;
    f.p = 100000;
    f.n = 5000;
    f.attempts = flags & KSCHED_PICK_DRAWS ? 5 : 0;
    f.flags = flags;
    f.nkeys = 8;
    f.have_feas = have_feas;
    f.have_psel = flags & KSCHED_SEL;
    f.tiles = 5;
    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = true;
    f.bf_rows_built = true;
    f.fused_waves = 16;
    f.combine = combine_op(flags);
    f.soft = combine_soft(flags);
    f.selop = sel_op(flags);
    f.seltag = sel_tagged(flags);
    f.terms = sel_terms(flags);
    return f;
}

static void the_plan_with_the_field() {
    CHECK(EvalFacts().terms == 0u && EvalPlan().terms == 0u);
    unsigned plans = 0;
    for (uint32_t T : {0u, 1u, 2u, 15u})
        for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
            for (uint32_t pick : kPicks)
                for (int have_feas = 0; have_feas < 2; ++have_feas)
                    for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
                        for (int can = 0; can < 2; ++can)
                            for (int from_mask = 0; from_mask < 2; ++from_mask)
                                for (int fused_pick = 0; fused_pick <= 3; ++fused_pick) {
                                    if (comb && !have_feas) continue;   // (check_combine_args refuses a combining call without its mask)
                                    if (!pick && !have_feas) continue;  // (check_eval_args refuses a call with nothing to write)
                                    EvalFacts f = step(KSCHED_SEL | kTagged | terms(T) | comb | pick, have_feas);
                                    f.opt_kernel = opt;
                                    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = can;
                                    f.opt_pick_from_mask = from_mask;
                                    f.opt_fused_pick = fused_pick;
                                    const EvalPlan pl = plan_eval(f);
                                    EvalFacts g = f;  // the same call without the field: the tagged call's plan
                                    g.terms = 0;
                                    g.flags &= ~kField;
                                    const EvalPlan tg = plan_eval(g);
                                    ++plans;
                                    CHECK(pl.error == KSCHED_OK && pl.why == PlanError::kNone && pl.seltag && pl.selop == SelOp::kNone);
                                    // the terms kernel whenever the field is not 0, one term included; the tagged kernel without it
                                    CHECK(pl.terms == T);
                                    CHECK(pl.mask == (T ? MaskKernel::kSelTerms : MaskKernel::kSelTag));
                                    CHECK(is(pl.last_kernel, T ? "selterms" : "seltag"));
                                    CHECK(tg.mask == MaskKernel::kSelTag && tg.terms == 0u && is(tg.last_kernel, "seltag"));
                                    // everything around the kernel is the tagged call's plan
                                    CHECK(pl.combine == tg.combine && pl.soft == tg.soft && pl.scratch_mask == tg.scratch_mask && pl.sampled == tg.sampled &&
                                          pl.bestfit == tg.bestfit && pl.ranked == tg.ranked && is(pl.last_pick, tg.last_pick));
                                    CHECK(pl.combine == combine_op(comb) && pl.soft == ((comb & kSoft) != 0) && pl.scratch_mask == (comb != 0 || !have_feas));
                                    CHECK(!pl.pick_rides() && !pl.bestfit_rows() && pl.pick_from_mask() == (pick != 0));
                                }
    CHECK(plans > 3000);
    // the field reaches a plan only through a tagged call (check_selterms_args refuses every other word): without `seltag` it is not looked at
    EvalFacts f = step(KSCHED_FIT | KSCHED_SEL, true);
    f.terms = 3;
    CHECK(plan_eval(f).terms == 0u && plan_eval(f).mask != MaskKernel::kSelTerms);
    f = step(KSCHED_SEL | kGt, true);
    f.terms = 3;
    CHECK(plan_eval(f).terms == 0u && plan_eval(f).mask == MaskKernel::kSelOp);
}

// ---- without the field: today's plans -------------------------------------------------------------------------------------------------------
// plan_eval as it was before EvalFacts and EvalPlan had the terms field (the parent's function, word for word)
static EvalPlan plan_eval_as_it_was(const EvalFacts &f) {
    EvalPlan plan;
    const uint32_t p = f.p, flags = f.flags;
    const bool pick_s = flags & KSCHED_PICK_SAMPLED, pick_b = flags & KSCHED_PICK_BESTFIT;
    const bool want_mask = f.have_feas || f.have_fit;
    const bool can_fused = f.fused_applicable;
    const int kern = choose_kernel(f.opt_kernel, can_fused);
    if (f.selop != SelOp::kNone || f.seltag) {
        if (f.selop != SelOp::kNone) {
            plan.selop = f.selop;
            plan.mask = MaskKernel::kSelOp;
            plan.last_kernel = "selop";
        } else {
            plan.seltag = true;
            plan.mask = MaskKernel::kSelTag;
            plan.last_kernel = "seltag";
        }
        plan.combine = f.combine;
        plan.soft = f.combine != CombineOp::kNone && f.soft;
        plan.scratch_mask = f.combine != CombineOp::kNone || !f.have_feas;
        if (const RankedMember *m = ranked_member(flags)) {
            plan.ranked = m->pick;
            plan.last_pick = m->name;
        } else if (pick_s || pick_b) {
            if (pick_s) plan.sampled = SampledPick::kFromMask;
            else plan.bestfit = BestfitPick::kFromMask;
            plan.last_pick = "from-mask";
        }
        return plan;
    }
    if (f.combine != CombineOp::kNone) {
        if (kern == KSCHED_KERNEL_FUSED && !can_fused) return plan_unsupported(PlanError::kFusedNotApplicable);
        plan.combine = f.combine;
        plan.soft = f.soft;
        plan.scratch_mask = true;
        plan.mask = kern == KSCHED_KERNEL_FUSED ? MaskKernel::kFused : MaskKernel::kDirect;
        plan.last_kernel = kern == KSCHED_KERNEL_FUSED ? "fused" : "direct";
        if (const RankedMember *m = ranked_member(flags)) {
            plan.ranked = m->pick;
            plan.last_pick = m->name;
        } else if (pick_s || pick_b) {
            if (pick_s) plan.sampled = SampledPick::kFromMask;
            else plan.bestfit = BestfitPick::kFromMask;
            plan.last_pick = "from-mask";
        }
        return plan;
    }
    if (const RankedMember *m = ranked_member(flags)) {
        if (kern == KSCHED_KERNEL_FUSED && !can_fused) return plan_unsupported(PlanError::kFusedNotApplicable);
        plan.scratch_mask = !f.have_feas;
        plan.mask = kern == KSCHED_KERNEL_FUSED ? MaskKernel::kFused : MaskKernel::kDirect;
        plan.last_kernel = kern == KSCHED_KERNEL_FUSED ? "fused" : "direct";
        plan.ranked = m->pick;
        plan.last_pick = m->name;
        return plan;
    }
    const bool select_direct = pick_s && !f.opt_pick_from_mask;
    const bool tile_pays = f.tiles >= 2u && f.tiles <= 12u;
    const bool tile_form = f.opt_fused_pick == 3 || (f.opt_fused_pick == 1 && can_fused && tile_pays && f.fused_tile_pick_applicable);
    bool ride_pays = true;
    if (f.opt_fused_pick == 1 && can_fused) {
        if (tile_form) {
            ride_pays = p <= (1u << 19);
        } else {
            const uint32_t tiles = std::max(1u, f.tiles), cus = f.opt_grid_cus ? f.opt_grid_cus : 256u;
            const uint32_t chunks = std::max(1u, std::min(cus / tiles, (p + 255u) / 256u));
            ride_pays = (uint64_t)p <= (uint64_t)chunks * 5u * 64u * f.fused_waves;
        }
    }
    const bool pick_rides = select_direct && want_mask && f.opt_fused_pick && kern == KSCHED_KERNEL_FUSED && can_fused && ride_pays &&
                            f.fused_pick_applicable;
    if (pick_rides) {
        if (tile_form && !f.fused_tile_pick_applicable) return plan_unsupported(PlanError::kTilePickNotApplicable);
        plan.sampled = tile_form ? SampledPick::kRidesTiles : SampledPick::kRidesFill;
        plan.last_pick = tile_form ? "fused-tile" : "fused";
    } else if (select_direct) {
        plan.sampled = SampledPick::kOwnLaunch;
        plan.last_pick = "select";
        if (!want_mask) return plan;
    }
    if (pick_b && !f.opt_pick_from_mask && f.bf_rows_built) {
        const bool sel = (flags & KSCHED_SEL) && f.have_psel && f.nkeys > 0;
        const bool lists = sel && f.nlist > 0;
        const bool two_stage = lists || f.opt_bestfit_stages == 2 || (f.opt_bestfit_stages == 0 && p >= 24576u);
        if (!lists && (!two_stage || (f.debug & 0x400u) || f.n > kBfLanesMaxNodes)) {
            plan.bestfit = BestfitPick::kRowsOneStage;
        } else {
            if (f.n > kBfLanesMaxNodes) return plan_unsupported(PlanError::kListKeysTooManyNodes);
            plan.bestfit = lists ? BestfitPick::kRowsTwoStagesListed : BestfitPick::kRowsTwoStages;
        }
        plan.last_pick = "bestfit-rows";
        if (!want_mask) return plan;
    }
    plan.scratch_mask = !f.have_feas;
    if (kern == KSCHED_KERNEL_FUSED && !can_fused) return plan_unsupported(PlanError::kFusedNotApplicable);
    plan.mask = kern == KSCHED_KERNEL_FUSED ? MaskKernel::kFused : MaskKernel::kDirect;
    plan.last_kernel = kern == KSCHED_KERNEL_FUSED ? "fused" : "direct";
    if (pick_reads_mask(flags, f.opt_pick_from_mask, f.bf_rows_built)) {
        if (pick_s) plan.sampled = SampledPick::kFromMask;
        else plan.bestfit = BestfitPick::kFromMask;
        plan.last_pick = "from-mask";
    }
    return plan;
}

static bool same_plan(const EvalPlan &a, const EvalPlan &b) {
    return a.error == b.error && a.why == b.why && a.mask == b.mask && a.scratch_mask == b.scratch_mask && a.sampled == b.sampled && a.bestfit == b.bestfit &&
           a.ranked == b.ranked && a.combine == b.combine && a.soft == b.soft && a.selop == b.selop && a.seltag == b.seltag && is(a.last_kernel, b.last_kernel) &&
           is(a.last_pick, b.last_pick);
}

// the facts tests/cpp/seltag_plan_tests.cpp walks, with the tagged call among the predicate sets: none carries the field, every plan is the parent's
static void without_the_field_every_plan_is_what_it_was() {
    const uint32_t preds[] = {KSCHED_FIT, KSCHED_FIT | KSCHED_SEL, KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT, KSCHED_SEL | kExists, KSCHED_SEL | kGt, KSCHED_SEL | kLt,
                              KSCHED_SEL | kTagged};
    unsigned plans = 0, errors = 0, tagged = 0;
    for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
        for (uint32_t pick : kPicks)
            for (uint32_t pred : preds)
                for (uint32_t outs = 0; outs < 4; ++outs)  // bit 0: out_feasible, bit 1: out_fit (+ WANT_FIT_MASK)
                    for (int opt_kernel : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
                        for (uint32_t applic = 0; applic < 4; ++applic)
                            for (int from_mask = 0; from_mask < 2; ++from_mask)
                                for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
                                    for (int stages = 0; stages <= 2; ++stages)
                                        for (int bf = 0; bf < 2; ++bf)
                                            for (uint32_t p : {1u, 24575u, 24576u, 100000u, (1u << 19) + 1u})
                                                for (uint32_t shape = 0; shape < 4; ++shape) {  // (tiles, nlist, n)
                                                    if (!pick && !outs) continue;
                                                    if (comb && outs != 1u) continue;
                                                    if ((pred & (kAny | kTagged)) && (outs & 2u)) continue;  // (an operator or tagged call has no fit mask)
                                                    EvalFacts f;
                                                    f.p = p;
                                                    f.n = shape == 3 ? kBfLanesMaxNodes + 1 : 5000;
                                                    f.attempts = pick & KSCHED_PICK_DRAWS ? 5 : 0;
                                                    f.flags = pred | pick | comb | ((outs & 2u) ? KSCHED_WANT_FIT_MASK : 0u);
                                                    f.nkeys = 8;
                                                    f.have_feas = outs & 1u;
                                                    f.have_fit = outs & 2u;
                                                    f.have_psel = pred & KSCHED_SEL;
                                                    f.tiles = shape == 0 ? 1 : shape == 1 ? 5 : 13;
                                                    f.nlist = shape >= 2 ? 2 : 0;
                                                    f.fused_applicable = applic >= 1;
                                                    f.fused_pick_applicable = applic >= 2;
                                                    f.fused_tile_pick_applicable = applic >= 3;
                                                    f.bf_rows_built = bf;
                                                    f.fused_waves = 16;
                                                    f.opt_kernel = opt_kernel;
                                                    f.opt_fused_pick = fused_pick;
                                                    f.opt_bestfit_stages = stages;
                                                    f.opt_pick_from_mask = from_mask;
                                                    f.combine = combine_op(f.flags);
                                                    f.soft = combine_soft(f.flags);
                                                    f.selop = sel_op(f.flags);
                                                    f.seltag = sel_tagged(f.flags);
                                                    f.terms = sel_terms(f.flags);
                                                    const EvalPlan now = plan_eval(f), was = plan_eval_as_it_was(f);
                                                    CHECK(f.terms == 0u && now.terms == 0u && now.mask != MaskKernel::kSelTerms);
                                                    CHECK(same_plan(now, was));
                                                    ++plans;
                                                    errors += now.error != KSCHED_OK;
                                                    tagged += now.mask == MaskKernel::kSelTag;
                                                }
    CHECK(plans > 100000 && errors > 0 && errors < plans && tagged > 0 && tagged < plans);
    std::printf("without the field: %u plans compared with the plan as it was (%u of them refusals, %u tagged calls)\n", plans, errors, tagged);
}

int main() {
    the_field();
    the_argument_rules();
    the_layout();
    the_row_rule();
    the_launch();
    the_plan_with_the_field();
    without_the_field_every_plan_is_what_it_was();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
