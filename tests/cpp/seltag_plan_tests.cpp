// seltag_plan_tests.cpp -- host-side check of the rules of a tagged call (extension E9, KSCHED_SELOP_TAGGED: csrc/sel_tags.hpp,
// csrc/eval_plan.hpp), no GPU and no HIP: the constants and what they leave alone; every refusal and every accepted combination of
// check_seltag_args, the flag beside each KSCHED_SELOP_* flag included; the rule for one (entry, id) pair against a table written out by
// hand, and the one compare form the kernel decodes every tag into (seltag_form, and seltag_form_bits -- the kernel's arithmetic) against
// that rule; seltag_row against a loop over single bits written here, padding bits under NE and ABSENT included; the launch plan walked on
// the CPU as k_eval_seltag walks it (every word below W of every row by exactly one lane of exactly one wave, no padding word ever, every
// key by exactly one pass); the plan of a tagged call -- plain, combining, soft, each pick, KSCHED_OPT_KERNEL forced each way --; and that
// a request without the flag gets the plan it got before the field existed (plan_eval_as_it_was below).  The expectations are written out
// here, not computed by the header.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/eval_plan.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/mask_combine_soft.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/sel_ops.hpp"
#include "../../kube_scheduler_rs_reference_amd/csrc/sel_tags.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static bool is(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

static const uint32_t kTagged = 0x40000u;
static const uint32_t kExists = 0x4000u, kGt = 0x8000u, kLt = 0x10000u, kAny = 0x1C000u;
static const uint32_t kAnd = 0x200u, kOr = 0x400u, kAndNot = 0x800u, kSoft = 0x2000u;
static const uint32_t kNever = 0xFFFFFFFFu;
static const uint32_t kOpFlags[] = {kExists, kGt, kLt};
static const uint32_t kPicks[] = {0u, KSCHED_PICK_SAMPLED, KSCHED_PICK_BESTFIT, KSCHED_PICK_UNIFORM, KSCHED_PICK_SPREAD, KSCHED_PICK_PACK};
enum : uint32_t { EQ = 0, NE = 1, EX = 2, AB = 3, GT = 4, LT = 5 };

static uint32_t ent(uint32_t tag, uint32_t id) { return (tag << 29) | id; }

// ---- the constants ---------------------------------------------------------------------------------------------------------------------
static void the_flag() {
    CHECK(KSCHED_SELOP_TAGGED == kTagged && KSCHED_SELTAG_SHIFT == 29u && KSCHED_SELTAG_ID_MASK == 0x1FFFFFFFu);
    CHECK(KSCHED_SELTAG_EQ == 0u && KSCHED_SELTAG_NE == 1u && KSCHED_SELTAG_EXISTS == 2u && KSCHED_SELTAG_ABSENT == 3u && KSCHED_SELTAG_GT == 4u && KSCHED_SELTAG_LT == 5u);
    CHECK((kTagged & (kTagged - 1u)) == 0 && !(kTagged & (0x1FFu | 0xE00u | 0x2000u | 0x1C000u | 0x1000u | 0x20000u)));
    CHECK(KSCHED_SELOP_ANY == kAny && !(KSCHED_SELOP_ANY & kTagged));  // a modifier of KSCHED_SEL, not a member of the operators
    CHECK((KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_ANY | KSCHED_WANT_FIT_MASK) == 0x1FFu && KSCHED_COMBINE_ANY == 0xE00u && KSCHED_COMBINE_SOFT == 0x2000u);
    CHECK(KSCHED_SEL_NEVER == kNever && KSCHED_ABI_VERSION == 7u);
    CHECK(seltag_tag(kNever) == 7u && seltag_id(kNever) == 0x1FFFFFFFu && seltag_tag(0x80000010u) == GT && seltag_id(0x80000010u) == 16u);
    CHECK(seltag_entry(GT, 16) == 0x80000010u && seltag_entry(EQ, 5) == 5u && seltag_entry(7, 0x1FFFFFFFu) == kNever && seltag_entry(EQ, 0) == 0u);
    for (uint32_t rest : {0u, 0x1FFu, 0xE00u, 0x2000u, 0x1000u, 0x20000u, 0x1C000u, 0xFFF80000u}) {
        CHECK(!sel_tagged(rest) && sel_tagged(rest | kTagged));
        // the flag changes neither the operator of a word, nor its combine op, nor its modifier
        CHECK(sel_op(rest | kTagged) == sel_op(rest) && combine_op(rest | kTagged) == combine_op(rest) && combine_soft(rest | kTagged) == combine_soft(rest));
    }
}

// ---- the refusals -----------------------------------------------------------------------------------------------------------------------
static void the_argument_rules() {
    // accepted: SEL and the flag; a combine op, the modifier and a pick beside them change nothing here (their rules are their own)
    for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
        for (uint32_t pick : kPicks) {
            const uint32_t f = KSCHED_SEL | kTagged | comb | pick;
            CHECK(check_seltag_args(f, true, false) == KSCHED_OK);
            CHECK(check_selop_args(f, true, false) == KSCHED_OK && check_selop_args(f, false, false) == KSCHED_OK);  // no operator: E8's rule says nothing
            CHECK(check_seltag_args(f, false, false) == KSCHED_E_INVAL);  // an entry point that takes no tagged call
            CHECK(check_seltag_args(f, true, true) == KSCHED_E_INVAL);    // out_fit
            CHECK(check_seltag_args(f, false, true) == KSCHED_E_INVAL);
            CHECK(check_seltag_args(f & ~(uint32_t)KSCHED_SEL, true, false) == KSCHED_E_INVAL);  // no KSCHED_SEL
            CHECK(check_seltag_args(f | KSCHED_FIT, true, false) == KSCHED_E_INVAL);
            CHECK(check_seltag_args(f | KSCHED_TAINT, true, false) == KSCHED_E_INVAL);
            CHECK(check_seltag_args(f | KSCHED_FIT | KSCHED_TAINT, true, false) == KSCHED_E_INVAL);
            CHECK(check_seltag_args(f | KSCHED_WANT_FIT_MASK, true, false) == KSCHED_E_INVAL);
            CHECK(check_seltag_args(f | KSCHED_WANT_FIT_MASK, true, true) == KSCHED_E_INVAL);
            for (uint32_t op : kOpFlags) CHECK(check_seltag_args(f | op, true, false) == KSCHED_E_INVAL);  // beside each operator flag
            CHECK(check_seltag_args(f | kGt | kLt, true, false) == KSCHED_E_INVAL && check_seltag_args(f | kAny, true, false) == KSCHED_E_INVAL);
        }
    CHECK(check_seltag_args(kTagged, true, false) == KSCHED_E_INVAL);  // the flag alone
    // a word without the flag: the rule says nothing, whatever the rest
    for (uint32_t rest : {0u, 0x1FFu, (uint32_t)KSCHED_SEL, (uint32_t)(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT), 0xE00u, kSoft, 0x1000u, 0x20000u,
                          (uint32_t)KSCHED_WANT_FIT_MASK, KSCHED_SEL | kGt, kAny, KSCHED_FIT | kExists})
        for (int accepted = 0; accepted < 2; ++accepted)
            for (int fit = 0; fit < 2; ++fit) CHECK(check_seltag_args(rest, accepted, fit) == KSCHED_OK);
    // the combine's and the modifier's own rules hold beside the flag as beside none
    for (uint32_t comb : {kAnd, kOr, kAndNot, kAnd | kSoft, kOr | kSoft, kSoft, kAnd | kOr})
        for (int accepted = 0; accepted < 2; ++accepted)
            for (int feas = 0; feas < 2; ++feas)
                CHECK(check_soft_args(KSCHED_SEL | kTagged | comb, accepted, feas, false) == check_soft_args(KSCHED_SEL | comb, accepted, feas, false));
}

// ---- one pair ---------------------------------------------------------------------------------------------------------------------------
static const uint32_t kId = 1000u;
static const uint32_t kNodeIds[12] = {0u, 1u, 2u, kId - 1u, kId, kId + 1u, 0x1FFFFFFFu, 0x20000000u, 0x20000001u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu};
// per tag 0 .. 7 the bit for each node id above, with the entry's id = 1000: the table of tests/test_seltag_restatement.py, by hand
static const int kTable[8][12] = {
    {0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0},  // EQ
    {1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1},  // NE: an absent node passes
    {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},  // EXISTS
    {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},  // ABSENT
    {0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1},  // GT: an absent node fails
    {0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0},  // LT: an absent node fails
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
};

static void the_pair_rule() {
    for (uint32_t tag = 0; tag < 8; ++tag)
        for (int i = 0; i < 12; ++i) CHECK(seltag_pass(ent(tag, kId), kNodeIds[i]) == (kTable[tag][i] != 0));
    for (uint32_t v : kNodeIds) {
        CHECK(seltag_pass(0u, v));        // e == 0: not constrained, also on a node without the key
        CHECK(!seltag_pass(kNever, v));   // tag 7
        for (uint32_t id : {0u, 1u, 2u, kId, 0x1FFFFFFEu, 0x1FFFFFFFu}) {
            CHECK(!seltag_pass(ent(6, id), v) && !seltag_pass(ent(7, id), v));  // whatever the id field holds
            CHECK(seltag_pass(ent(EX, id), v) == (v != 0u) && seltag_pass(ent(AB, id), v) == (v == 0u));  // the id field is not looked at
        }
        CHECK(!seltag_pass(ent(LT, 0), v) && !seltag_pass(ent(LT, 1), v) && seltag_pass(ent(LT, 2), v) == (v == 1u));
        CHECK(seltag_pass(ent(GT, 0x1FFFFFFFu), v) == (v >= 0x20000000u));  // ids at or above 2^29 pass GT for every bound
        CHECK(seltag_pass(ent(GT, 0), v) == (v != 0u) && seltag_pass(ent(NE, 0), v) == (v != 0u));
    }
    // the node's id is compared WHOLE: 0x20000001 & 0x1FFFFFFF == 1, yet it is not id 1
    CHECK(!seltag_pass(ent(EQ, 1), 0x20000001u) && seltag_pass(ent(NE, 1), 0x20000001u) && !seltag_pass(ent(LT, 2), 0x20000001u));
    CHECK(seltag_pass(ent(EQ, 0x1FFFFFFFu), 0x1FFFFFFFu) && !seltag_pass(ent(EQ, 0x1FFFFFFFu), 0xFFFFFFFFu) && !seltag_pass(ent(LT, 0x1FFFFFFFu), 0x80000000u));
}

// the compare form the kernel reduces every entry to -- (v - lo < len) != neg -- gives seltag_pass for every constrained entry, both as the
// header states it per tag and as the kernel computes it from the tag's bits
static void the_compare_form() {
    const uint32_t ids[] = {0u, 1u, 2u, 3u, kId, 0x1FFFFFFEu, 0x1FFFFFFFu};
    const uint32_t vs[] = {0u, 1u, 2u, 3u, 4u, kId - 1u, kId, kId + 1u, 0x1FFFFFFDu, 0x1FFFFFFEu, 0x1FFFFFFFu, 0x20000000u, 0x20000001u, 0x20000002u,
                           0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    unsigned pairs = 0;
    for (uint32_t tag = 0; tag < 8; ++tag)
        for (uint32_t id : ids) {
            const uint32_t e = ent(tag, id);
            if (e == 0u) continue;  // (the kernel skips an unconstrained entry before it decodes)
            const SeltagForm f = seltag_form(e), b = seltag_form_bits(e);
            CHECK(f.neg == (tag == NE || tag == AB) && b.neg == f.neg && b.len == f.len);
            CHECK(f.len == 0u || b.lo == f.lo);  // (an empty range starts anywhere)
            for (uint32_t v : vs) {
                CHECK(seltag_form_pass(f, v) == seltag_pass(e, v));
                CHECK(seltag_form_pass(b, v) == seltag_pass(e, v));
                ++pairs;
            }
        }
    CHECK(pairs == (8u * 7u - 1u) * 20u);
    // the numbers of a few forms
    SeltagForm f = seltag_form(ent(GT, 16));
    CHECK(f.lo == 17u && f.len == 0xFFFFFFEFu && !f.neg);
    f = seltag_form(ent(LT, 16));
    CHECK(f.lo == 1u && f.len == 15u && !f.neg);
    f = seltag_form(ent(NE, 3));
    CHECK(f.lo == 3u && f.len == 1u && f.neg);
    f = seltag_form(ent(AB, 9));
    CHECK(f.lo == 1u && f.len == 0xFFFFFFFFu && f.neg);
    CHECK(seltag_form(kNever).len == 0u && !seltag_form(kNever).neg && seltag_form(ent(LT, 1)).len == 0u && seltag_form(ent(LT, 0)).len == 0u);
}

// ---- one row ----------------------------------------------------------------------------------------------------------------------------
static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static void the_row_rule() {
    const uint32_t pool[] = {0u, 1u, 2u, 3u, 0x1FFFFFFFu, 0x20000000u, 0x20000001u, 0x80000000u, 0xFFFFFFFEu};
    uint32_t seed = 0xE9u;
    unsigned rows = 0, full = 0, empty = 0;
    for (uint32_t n : {1u, 63u, 64u, 65u, 130u})
        for (uint32_t nkeys : {1u, 2u, 9u}) {
            const uint32_t p = 11, W = (n + 63u) / 64u;
            std::vector<uint32_t> lab((size_t)nkeys * n), sel((size_t)nkeys * p);
            for (uint32_t &v : lab) v = pool[(lcg(seed) >> 8) % 9u];
            for (uint32_t &e : sel) {
                const uint32_t r = (lcg(seed) >> 8) % 24u;  // a third constrained: the six tags, 6, 7 and NEVER
                e = r < 8u ? ent(r, pool[(lcg(seed) >> 8) % 5u]) : r == 8u ? kNever : 0u;
            }
            for (uint32_t pod = 0; pod < p; ++pod) {
                std::vector<uint64_t> row(W, ~0ull), want(W, 0);
                seltag_row(lab.data(), sel.data(), nkeys, n, p, pod, row.data());
                for (uint32_t node = 0; node < n; ++node) {  // bit by bit, from the header's table
                    bool ok = true;
                    for (uint32_t k = 0; k < nkeys; ++k) {
                        const uint32_t e = sel[(size_t)k * p + pod], v = lab[(size_t)k * n + node];
                        if (e == 0u) continue;
                        const uint32_t tag = e >> 29, id = e & 0x1FFFFFFFu;
                        if (tag == EQ) ok = ok && v == id;
                        else if (tag == NE) ok = ok && v != id;
                        else if (tag == EX) ok = ok && v != 0u;
                        else if (tag == AB) ok = ok && v == 0u;
                        else if (tag == GT) ok = ok && v != 0u && v > id;
                        else if (tag == LT) ok = ok && v != 0u && v < id;
                        else ok = false;
                    }
                    if (ok) want[node / 64u] |= 1ull << (node % 64u);
                }
                CHECK(row == want);
                ++rows;
                bool all = true, none = true;
                for (uint32_t w = 0; w < W; ++w) {
                    all = all && want[w] == (w + 1u < W || n % 64u == 0 ? ~0ull : (1ull << (n % 64u)) - 1ull);
                    none = none && want[w] == 0;
                }
                full += all;
                empty += none;
            }
            // a row that every real node passes under NE and under ABSENT: the padding bits stay zero
            std::vector<uint32_t> absent((size_t)nkeys * n, 0u), neg((size_t)nkeys * p, 0u);
            neg[0] = ent(NE, 5);
            neg[1] = ent(AB, 5);
            for (uint32_t pod = 0; pod < 2; ++pod) {
                std::vector<uint64_t> row(W, 0x5A5Aull);
                seltag_row(absent.data(), neg.data(), nkeys, n, p, pod, row.data());
                for (uint32_t w = 0; w < W; ++w) CHECK(row[w] == ((w + 1u < W || n % 64u == 0) ? ~0ull : (1ull << (n % 64u)) - 1ull));
            }
            // no selectors, and no keys: every node passes, padding bits zero
            std::vector<uint64_t> row(W, 0x5A5Aull);
            seltag_row(lab.data(), nullptr, nkeys, n, p, 0, row.data());
            std::vector<uint64_t> row0(W, 0x5A5Aull);
            seltag_row(nullptr, sel.data(), 0, n, p, 0, row0.data());
            for (uint32_t w = 0; w < W; ++w) {
                const uint64_t valid = (w + 1u < W || n % 64u == 0) ? ~0ull : (1ull << (n % 64u)) - 1ull;
                CHECK(row[w] == valid && row0[w] == valid);
            }
        }
    CHECK(rows == 5u * 3u * 11u && full > 0 && empty > 0 && full + empty < rows);
}

// ---- the launch plan ----------------------------------------------------------------------------------------------------------------------
// every thread block of every pass walks as k_eval_seltag does; `seen` counts the stores into every word of a [p][pitch] buffer by the first
// pass (the later passes touch the same words: they AND into them)
static void walk(uint32_t p, uint32_t W, uint32_t pitch, uint32_t nkeys) {
    const SeltagLaunch l = plan_seltag_launch(p, W, nkeys);
    const SelopLaunch o = plan_selop_launch(p, W, nkeys);  // the same geometry, not restated
    CHECK(l.block == o.block && l.gx == o.gx && l.gy == o.gy && l.pod_tiles == o.pod_tiles && l.pod_tiles_per_block == o.pod_tiles_per_block && l.passes == o.passes);
    CHECK(l.block == 256u && l.gx == (W + 15u) / 16u && l.gy >= 1u && l.gy <= 2048u && l.pod_tiles == (p + 63u) / 64u);
    CHECK((uint64_t)l.gy * l.pod_tiles_per_block >= l.pod_tiles && (uint64_t)(l.gy - 1u) * l.pod_tiles_per_block < l.pod_tiles);
    CHECK(l.passes == (nkeys == 0 ? 1u : (nkeys + 7u) / 8u));
    // the keys: every key by exactly one pass, at most eight a pass
    std::vector<uint8_t> key_seen(nkeys, 0);
    for (uint32_t pass = 0; pass < l.passes; ++pass) {
        const uint32_t k0 = selop_pass_key0(pass), nk = selop_pass_keys(nkeys, pass);
        CHECK(k0 == 8u * pass && nk <= 8u && (nk > 0 || nkeys == 0) && k0 + nk <= nkeys);
        for (uint32_t k = 0; k < nk; ++k) ++key_seen[k0 + k];
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
                    for (uint32_t lane = 0; lane < jmax; ++lane)
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
        for (uint32_t W : {1u, 2u, 4u, 5u, 15u, 16u, 17u, 33u, 65u})
            for (uint32_t extra : {0u, 1u, 15u})
                for (uint32_t nkeys : {0u, 1u, 8u, 9u, 16u, 17u, 32u}) walk(p, W, W + extra, nkeys);
    SeltagLaunch l = plan_seltag_launch(100000, 79, 8);  // C3: 5 column blocks, 391 block rows of 4 tiles
    CHECK(l.gx == 5 && l.pod_tiles == 1563 && l.gy == 391 && l.pod_tiles_per_block == 4 && l.passes == 1);
    l = plan_seltag_launch(64, 16, 32);
    CHECK(l.gx == 1 && l.gy == 1 && l.pod_tiles_per_block == 1 && l.passes == 4);
    l = plan_seltag_launch(0, 5, 8);
    CHECK(l.gx == 0 && l.gy == 0 && l.passes == 0);  // nothing to launch
    l = plan_seltag_launch(5, 0, 8);
    CHECK(l.gx == 0 && l.gy == 0 && l.passes == 0);
    walk(2048u * 64u + 1u, 1, 1, 8);  // one pod more than 2048 block rows of one tile: two tiles a block
    walk(3u * 2048u * 64u + 65u, 3, 4, 9);
}

// ---- the plan of a tagged call --------------------------------------------------------------------------------------------------------------
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
    return f;
}

static void the_plan_of_a_tagged_call() {
    CHECK(!EvalFacts().seltag && !EvalPlan().seltag);
    unsigned plans = 0;
    for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
        for (uint32_t pick : kPicks)
            for (int have_feas = 0; have_feas < 2; ++have_feas)
                for (int opt : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
                    for (int can = 0; can < 2; ++can)
                        for (int from_mask = 0; from_mask < 2; ++from_mask)
                            for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
                                for (int bf = 0; bf < 2; ++bf) {
                                    if (comb && !have_feas) continue;  // (check_combine_args refuses a combining call without its mask)
                                    if (!pick && !have_feas) continue;  // (check_eval_args refuses a call with nothing to write)
                                    EvalFacts f = step(KSCHED_SEL | kTagged | comb | pick, have_feas);
                                    f.opt_kernel = opt;
                                    f.fused_applicable = f.fused_pick_applicable = f.fused_tile_pick_applicable = can;
                                    f.opt_pick_from_mask = from_mask;
                                    f.opt_fused_pick = fused_pick;
                                    f.bf_rows_built = bf;
                                    const EvalPlan pl = plan_eval(f);
                                    ++plans;
                                    // the tagged kernel, whatever KSCHED_OPT_KERNEL says and whether or not the snapshot has an index
                                    CHECK(pl.error == KSCHED_OK && pl.why == PlanError::kNone);
                                    CHECK(pl.mask == MaskKernel::kSelTag && pl.seltag && pl.selop == SelOp::kNone && is(pl.last_kernel, "seltag"));
                                    CHECK(pl.combine == combine_op(comb) && pl.soft == ((comb & kSoft) != 0));
                                    CHECK(pl.scratch_mask == (comb != 0 || !have_feas));
                                    CHECK(!pl.pick_rides() && !pl.bestfit_rows());
                                    CHECK(pl.pick_from_mask() == (pick != 0));
                                    const char *name = !pick ? "none" : pick == KSCHED_PICK_UNIFORM ? "uniform" : pick == KSCHED_PICK_SPREAD ? "spread" :
                                                       pick == KSCHED_PICK_PACK ? "pack" : "from-mask";
                                    CHECK(is(pl.last_pick, name));
                                    CHECK(pl.sampled == (pick == KSCHED_PICK_SAMPLED ? SampledPick::kFromMask : SampledPick::kNone));
                                    CHECK(pl.bestfit == (pick == KSCHED_PICK_BESTFIT ? BestfitPick::kFromMask : BestfitPick::kNone));
                                    CHECK(pl.ranked == (pick == KSCHED_PICK_UNIFORM ? RankedPick::kUniform : pick == KSCHED_PICK_SPREAD ? RankedPick::kSpread :
                                                        pick == KSCHED_PICK_PACK ? RankedPick::kPack : RankedPick::kNone));
                                }
    CHECK(plans > 1500);
    // the modifier without an op reaches no plan (check_soft_args refuses such a word before a plan is made)
    EvalFacts f = step(KSCHED_SEL | kTagged, true);
    f.soft = true;
    CHECK(!plan_eval(f).soft && plan_eval(f).combine == CombineOp::kNone && plan_eval(f).mask == MaskKernel::kSelTag);
    // an operator call is planned as it was: the operator kernel, no tagged one
    for (uint32_t op : kOpFlags) {
        const EvalPlan pl = plan_eval(step(KSCHED_SEL | op | kAnd | KSCHED_PICK_PACK, true));
        CHECK(pl.mask == MaskKernel::kSelOp && !pl.seltag && pl.selop == sel_op(op) && is(pl.last_kernel, "selop") && pl.combine == CombineOp::kAnd && is(pl.last_pick, "pack"));
    }
}

// ---- without the flag: today's plans --------------------------------------------------------------------------------------------------------
// plan_eval as it was before EvalFacts and EvalPlan had the seltag field (the parent's function, word for word)
static EvalPlan plan_eval_as_it_was(const EvalFacts &f) {
    EvalPlan plan;
    const uint32_t p = f.p, flags = f.flags;
    const bool pick_s = flags & KSCHED_PICK_SAMPLED, pick_b = flags & KSCHED_PICK_BESTFIT;
    const bool want_mask = f.have_feas || f.have_fit;
    const bool can_fused = f.fused_applicable;
    const int kern = choose_kernel(f.opt_kernel, can_fused);
    if (f.selop != SelOp::kNone) {
        plan.selop = f.selop;
        plan.mask = MaskKernel::kSelOp;
        plan.last_kernel = "selop";
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
           a.ranked == b.ranked && a.combine == b.combine && a.soft == b.soft && a.selop == b.selop && is(a.last_kernel, b.last_kernel) && is(a.last_pick, b.last_pick);
}

// the facts tests/cpp/selop_plan_tests.cpp walks for "no operator", with each combine op (and the modifier) beside them, and the operator
// calls of E8 on top: none carries the flag, every plan is the parent's
static void without_the_flag_every_plan_is_what_it_was() {
    const uint32_t preds[] = {KSCHED_FIT, KSCHED_FIT | KSCHED_SEL, KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT, KSCHED_SEL | kExists, KSCHED_SEL | kGt, KSCHED_SEL | kLt};
    unsigned plans = 0, errors = 0, operators = 0;
    for (uint32_t comb : {0u, kAnd, kOr, kAndNot, kAnd | kSoft, kAndNot | kSoft})
        for (uint32_t pick : kPicks)
            for (uint32_t pred : preds)
                for (uint32_t outs = 0; outs < 4; ++outs)  // bit 0: out_feasible, bit 1: out_fit (+ WANT_FIT_MASK)
                    for (int opt_kernel : {KSCHED_KERNEL_AUTO, KSCHED_KERNEL_DIRECT, KSCHED_KERNEL_FUSED})
                        for (uint32_t applic = 0; applic < 4; ++applic)  // 0: nothing fused applies, 1: the mask kernel, 2: + riding pick, 3: + tile pick
                            for (int from_mask = 0; from_mask < 2; ++from_mask)
                                for (int fused_pick = 0; fused_pick <= 3; ++fused_pick)
                                    for (int stages = 0; stages <= 2; ++stages)
                                        for (int bf = 0; bf < 2; ++bf)
                                            for (uint32_t p : {1u, 24575u, 24576u, 100000u, (1u << 19) + 1u})
                                                for (uint32_t shape = 0; shape < 4; ++shape) {  // (tiles, nlist, n)
                                                    if (!pick && !outs) continue;  // (check_eval_args refuses a call with nothing to write)
                                                    if (comb && outs != 1u) continue;  // (a combining call has its mask and no fit mask)
                                                    if ((pred & kAny) && (outs & 2u)) continue;  // (an operator call has no fit mask)
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
                                                    const EvalPlan now = plan_eval(f), was = plan_eval_as_it_was(f);
                                                    CHECK(!f.seltag && !now.seltag && now.mask != MaskKernel::kSelTag);
                                                    CHECK(same_plan(now, was));
                                                    ++plans;
                                                    errors += now.error != KSCHED_OK;
                                                    operators += now.mask == MaskKernel::kSelOp;
                                                }
    CHECK(plans > 100000 && errors > 0 && errors < plans && operators > 0 && operators < plans);
    std::printf("without the flag: %u plans compared with the plan as it was (%u of them refusals, %u operator calls)\n", plans, errors, operators);
}

int main() {
    the_flag();
    the_argument_rules();
    the_pair_rule();
    the_compare_form();
    the_row_rule();
    the_launch();
    the_plan_of_a_tagged_call();
    without_the_flag_every_plan_is_what_it_was();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
