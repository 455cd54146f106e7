// apply_admit_tests.cpp -- host-side check of KSCHED_APPLY_WHILE_FIT's chunk walk (csrc/apply_admit.hpp), no GPU and no HIP.
//
// A 64-lane emulation of k_apply_admit's loop over one node's segment -- the same steps in the same order, every number through the
// functions of apply_admit.hpp: split halves scanned with the doubling scan, the per-lane test, the ballot's first failing lane, the
// carry -- against the serial rule written out in 128-bit integers.  Exhaustive over segments of up to 4 pods with requests and
// `available` from {-1, 0, 1, 2, INT64_MAX, INT64_MIN} on both resources; random over segments of 63, 64, 65, 128, 129 and 1000 pods.
// Both with and without the shortcut for chunks that hold no negative request (the kernel has it), and the step counts it promises.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/apply_admit.hpp"

using namespace ksched;

static std::atomic<int> g_fail{0};
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

enum : int { A = 0, D = 3, O = 4 };  // KSCHED_APPLY_APPLIED, _DEFERRED, _OVERFLOW
struct Req {
    int64_t c, m;
};

// the rule as the header states it, one pod after the other
static void serial(int64_t &rc, int64_t &rm, const Req *q, size_t n, int *st) {
    for (size_t i = 0; i < n; ++i) {
        if (q[i].c <= rc && q[i].m <= rm) {
            const __int128 nc = (__int128)rc - q[i].c, nm = (__int128)rm - q[i].m;
            if (nc > (__int128)INT64_MAX || nm > (__int128)INT64_MAX) {
                st[i] = O;
            } else {
                rc = (int64_t)nc;
                rm = (int64_t)nm;
                st[i] = A;
            }
        } else {
            st[i] = D;
        }
    }
}

// the kernel's inclusive scan: log2(64) doubling steps; lanes at and past `nl` hold zero and nobody below reads them
static void scan(int64_t *v, uint32_t nl) {
    for (uint32_t d = 1; d < kAdmitLanes; d <<= 1)
        for (uint32_t j = nl; j-- > d;) v[j] += v[j - d];  // (descending: lane j reads lane j - d's value of before this step)
}

// k_apply_admit's walk over one segment; returns the number of steps
static uint32_t wave(int64_t &r_cpu, int64_t &r_mem, const Req *q, size_t n, int *st_out, bool shortcut) {
    uint32_t steps = 0;
    for (size_t g = 0; g < n; g += kAdmitLanes) {
        const uint32_t nl = (uint32_t)(n - g < kAdmitLanes ? n - g : kAdmitLanes);  // live lanes; the others are decided from the start and add 0
        int64_t c[kAdmitLanes], m[kAdmitLanes], hc[kAdmitLanes], lc[kAdmitLanes], hm[kAdmitLanes], lm[kAdmitLanes];
        int64_t shc[kAdmitLanes], slc[kAdmitLanes], shm[kAdmitLanes], slm[kAdmitLanes];
        bool undecided[kAdmitLanes];
        int st[kAdmitLanes], verdict[kAdmitLanes];
        bool shrink_only = shortcut;
        for (uint32_t j = 0; j < nl; ++j) {
            c[j] = q[g + j].c;
            m[j] = q[g + j].m;
            undecided[j] = true;
            st[j] = A;
            if (c[j] < 0 || m[j] < 0) shrink_only = false;
        }
        for (;;) {
            bool any = false;
            for (uint32_t j = 0; j < nl; ++j) any |= undecided[j];
            if (!any) break;
            ++steps;
            for (uint32_t j = 0; j < nl; ++j) {
                if (shrink_only && undecided[j] && !admit_fits(r_cpu, r_mem, c[j], m[j])) {
                    st[j] = D;
                    undecided[j] = false;
                }
                shc[j] = hc[j] = undecided[j] ? admit_hi(c[j]) : 0;
                slc[j] = lc[j] = undecided[j] ? admit_lo(c[j]) : 0;
                shm[j] = hm[j] = undecided[j] ? admit_hi(m[j]) : 0;
                slm[j] = lm[j] = undecided[j] ? admit_lo(m[j]) : 0;
            }
            scan(shc, nl), scan(slc, nl), scan(shm, nl), scan(slm, nl);
            uint64_t failing = 0;
            for (uint32_t j = 0; j < nl; ++j) {
                verdict[j] = admit_lane_test(r_cpu, r_mem, admit_join(shc[j] - hc[j], slc[j] - lc[j]), admit_join(shm[j] - hm[j], slm[j] - lm[j]), c[j], m[j]);
                if (undecided[j] && verdict[j] != kAdmitPass) failing |= 1ull << j;
            }
            const uint32_t f = admit_first_failing(failing);
            __int128 pc, pm;
            if (f == kAdmitLanes) {  // lane 63's inclusive sums = the last live lane's: the lanes between add 0
                pc = admit_join(shc[nl - 1], slc[nl - 1]);
                pm = admit_join(shm[nl - 1], slm[nl - 1]);
            } else {
                st[f] = verdict[f] == kAdmitOverflow ? O : D;
                pc = admit_join(shc[f] - hc[f], slc[f] - lc[f]);
                pm = admit_join(shm[f] - hm[f], slm[f] - lm[f]);
            }
            for (uint32_t j = 0; j < nl && j <= f; ++j) undecided[j] = false;
            CHECK((__int128)r_cpu - pc >= (__int128)INT64_MIN && (__int128)r_cpu - pc <= (__int128)INT64_MAX);  // the carry is a state of the serial walk
            CHECK((__int128)r_mem - pm >= (__int128)INT64_MIN && (__int128)r_mem - pm <= (__int128)INT64_MAX);
            r_cpu = admit_carry(r_cpu, pc);
            r_mem = admit_carry(r_mem, pm);
        }
        for (uint32_t j = 0; j < nl; ++j) st_out[g + j] = st[j];
    }
    return steps;
}

static std::atomic<long> g_cases{0};
thread_local long t_cases = 0;  // (added to g_cases when the thread's share is done)
static uint32_t both(int64_t rc, int64_t rm, const Req *q, size_t n) {
    thread_local std::vector<int> s0, s1;
    s0.assign(n, -1);
    uint32_t steps = 0;
    int64_t ac = rc, am = rm;
    serial(ac, am, q, n, s0.data());
    bool negative = false;  // (with a negative request in every chunk the shortcut is never taken: one walk says it all)
    for (size_t g = 0; g < n; g += kAdmitLanes) {
        bool neg = false;
        for (size_t i = g; i < n && i < g + kAdmitLanes; ++i) neg |= q[i].c < 0 || q[i].m < 0;
        negative = neg;
        if (!neg) break;
    }
    for (int shortcut = negative ? 1 : 0; shortcut < 2; ++shortcut) {
        s1.assign(n, -1);
        int64_t bc = rc, bm = rm;
        steps = wave(bc, bm, q, n, s1.data(), shortcut != 0);
        CHECK(ac == bc && am == bm);
        CHECK(s0 == s1);
    }
    ++t_cases;
    return steps;  // with the shortcut
}

static const int64_t kEdge[6] = {-1, 0, 1, 2, INT64_MAX, INT64_MIN};

// (the segments are dealt to `of` threads: 62 million in all)
static void exhaustive(int part, int of) {
    Req q[4];
    for (int len = 0; len <= 4; ++len) {
        long combos = 1;
        for (int i = 0; i < len; ++i) combos *= 36;
        for (long k = 0; k < combos; ++k) {
            if (k % of != part) continue;
            long r = k;
            for (int i = 0; i < len; ++i, r /= 36) q[i] = Req{kEdge[r % 6], kEdge[(r / 6) % 6]};
            for (int a = 0; a < 36; ++a) both(kEdge[a % 6], kEdge[a / 6], q, (size_t)len);
        }
    }
    g_cases += t_cases;
}

static void random_segments() {
    std::mt19937_64 rng(20260);
    const int64_t big[] = {0, 1, -1, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MIN + 1, (int64_t)1 << 62, -((int64_t)1 << 62), ((int64_t)1 << 32) + 5, -((int64_t)1 << 33)};
    const int64_t avail[] = {0, -1, 5, 40, 1000, 64000, INT64_MAX, INT64_MIN, INT64_MAX - 2, (int64_t)1 << 62, (int64_t)1 << 40};
    const size_t lens[] = {63, 64, 65, 128, 129, 1000};
    std::vector<Req> q;
    for (size_t len : lens) {
        const int trials = len == 1000 ? 400 : 3000;
        for (int t = 0; t < trials; ++t) {
            const int mode = t % 4;
            auto draw = [&]() -> int64_t {
                switch (mode) {
                    case 0: return (int64_t)(rng() % 6);                   // small, no negative request: the shortcut's ground
                    case 1: return (int64_t)(rng() % 10) - 3;              // small, both signs
                    case 2: return (int64_t)(rng() % (1ull << 34));        // both halves of the split in play
                    default: return big[rng() % (sizeof big / sizeof *big)];  // the ends of int64
                }
            };
            q.resize(len);
            for (Req &r : q) r = Req{draw(), draw()};
            const int64_t rc = mode == 2 ? (int64_t)(rng() % (1ull << 40)) : avail[rng() % (sizeof avail / sizeof *avail)];
            const int64_t rm = mode == 2 ? (int64_t)(rng() % (1ull << 40)) : avail[rng() % (sizeof avail / sizeof *avail)];
            both(rc, rm, q.data(), len);
        }
    }
}

// what the shortcut promises: a node that is full resolves a chunk without a negative request in one step, and a herd fills in few
static void step_counts() {
    std::vector<Req> herd(20000, Req{10, 10});
    CHECK(both(1000, 5000, herd.data(), herd.size()) <= 20000 / kAdmitLanes + 2);  // 100 pods fit: chunk 1 takes two steps, every other one
    std::vector<Req> full(64, Req{3, 3});
    CHECK(both(2, 100, full.data(), full.size()) == 1);
    CHECK(both(64 * 3, 64 * 3, full.data(), full.size()) == 1);  // exactly filled at the chunk's end: everybody passes at once
    std::vector<Req> two(128, Req{3, 3});
    CHECK(both(64 * 3, 64 * 3, two.data(), two.size()) == 2);    // ... and the next chunk is deferred in one step
    CHECK(both(63 * 3, 63 * 3, two.data(), two.size()) == 2);    // first failing lane 63, the chunk's last: one step, and chunk 2 at once
    CHECK(both(65 * 3, 65 * 3, two.data(), two.size()) == 3);    // first failing lane 65: the next chunk's second
}

int main() {
    const int of = 8;
    std::vector<std::thread> pool;
    for (int part = 0; part < of; ++part) pool.emplace_back(exhaustive, part, of);
    random_segments();
    step_counts();
    g_cases += t_cases;
    for (std::thread &t : pool) t.join();
    std::printf("%ld segments walked by the 64-lane emulation and by the serial rule\n", g_cases.load());
    std::printf("%d failed check(s)\n", g_fail.load());
    return g_fail.load() ? 1 : 0;
}
