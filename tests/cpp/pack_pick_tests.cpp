// pack_pick_tests.cpp -- Context::pick_pack of the host mirror (kube_scheduler_rs_reference_amd/host/scheduler.hpp: extension E5,
// KSCHED_PICK_PACK), driven by tests/test_gpu_pack_host.py.  Every mode needs a device.
//
//   pack_pick_tests objects <objects.json>     select_nodes_for_pods over a golden object set with pick_pack = 3 and a SplitMixChooser:
//                                              every pod's node is the tightest -- smallest (available memory, available cpu), lowest node
//                                              among equals -- of the candidates its recorded draws name in its own mask row, exactly the pods
//                                              with a feasible node (explain_unschedulable) get one, nothing is rejected; with pick_pack = 0
//                                              the selection is the sampled pick, draw for draw; together with pick_uniform or pick_spread it
//                                              is refused.
//                                              Prints the bindings ("bindings ...": the driver compares a three-way shard's line with one
//                                              device's).
//   (run it with KSCHED_SHARDED=n under the test hooks for the row-sharded path)
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/host/encoder.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/predicates.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/scheduler.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/util.hpp"
#include "objects_json.hpp"

using namespace ksched_host;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            ++g_fail;                                                        \
            std::printf("    FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

static void run(const char *name, const std::function<void()> &f) {
    const int before = g_fail;
    try {
        f();
    } catch (const std::exception &e) {
        ++g_fail;
        std::printf("    FAILED: exception %s\n", e.what());
    }
    std::printf("%s  %s\n", g_fail == before ? "ok" : "FAIL", name);
}

constexpr uint64_t kSeed = 0xE5E5E5E5ull;
constexpr uint32_t kDraws = 3;

// set bit number k (0-based, ascending) of a mask row over nodes [0, n), or -1; *count = the row's set bits
static int32_t kth_set_bit(const uint64_t *row, uint32_t n, uint64_t k, uint32_t *count) {
    int32_t found = -1;
    uint32_t c = 0;
    for (uint32_t node = 0; node < n; ++node)
        if ((row[node >> 6] >> (node & 63u)) & 1ull) {
            if (c == k) found = (int32_t)node;
            ++c;
        }
    *count = c;
    return found;
}

static void context_over(const objects_json::ObjectSet &obj, Context &ctx) {
    auto lister = std::make_shared<StaticPodLister>();
    lister->pods = obj.bound;
    ctx.client = lister;
    ctx.node_store.assign(obj.nodes.rbegin(), obj.nodes.rend());  // store order != canonical order
    ctx.warn = nullptr;
}

static void objects_tests(const char *path) {
    const objects_json::ObjectSet obj = objects_json::read_objects(path);
    std::vector<const corev1::Pod *> pp;
    for (const auto &p : obj.pods) pp.push_back(&p);
    const uint32_t p = (uint32_t)pp.size();

    run("pick_pack: every pod's node is the tightest of the candidates its recorded draws name in its own mask row", [&] {
        Context ctx;
        context_over(obj, ctx);
        ctx.pick_pack = kDraws;
        SplitMixChooser ch(kSeed);
        const BatchSelection sel = select_nodes_for_pods(pp, ctx, ch, /*want_rejected=*/true);
        const uint32_t n = ctx.snapshot->n(), W = ctx.snapshot->mask_words();
        CHECK(n == obj.nodes.size() && sel.node_store_index.size() == p && sel.validity.binding.size() == p);
        CHECK(sel.validity.feasible.size() == (size_t)p * W && sel.validity.W == W);
        CHECK(sel.rejected.empty());  // there are no rejected draws
        // the draws: kDraws per pod, in pod order and draw-major within a pod, chooser.choose(2^32)
        const bool have = sel.samples.size() == (size_t)p * kDraws;
        CHECK(have);
        SplitMixChooser again(kSeed);
        bool same_draws = have;
        for (size_t i = 0; same_draws && i < (size_t)p * kDraws; ++i) same_draws = sel.samples[i] == (uint32_t)*again.choose(size_t(1) << 32);
        CHECK(same_draws);
        const std::vector<Unschedulable> why = explain_unschedulable(pp, ctx);
        CHECK(why.size() == p);
        const std::vector<int64_t> &mem = ctx.snapshot->columns().avail_mem_bytes, &cpu = ctx.snapshot->columns().avail_cpu_milli;
        CHECK(mem.size() == n && cpu.size() == n);
        uint32_t bound = 0, several = 0, not_first = 0, bad = 0;
        for (uint32_t i = 0; i < p && have && why.size() == p && mem.size() == n && cpu.size() == n; ++i) {
            const uint64_t *row = sel.validity.feasible.data() + (size_t)i * W;
            uint32_t c = 0;
            (void)kth_set_bit(row, n, ~0ull, &c);
            int32_t want = -1, first = -1;
            for (uint32_t j = 0; c && j < kDraws; ++j) {
                const int32_t v = kth_set_bit(row, n, ((uint64_t)sel.samples[(size_t)i * kDraws + j] * c) >> 32, &c);
                if (j == 0) first = v;
                if (want < 0 || std::make_tuple(mem[(size_t)v], cpu[(size_t)v], v) < std::make_tuple(mem[(size_t)want], cpu[(size_t)want], want)) want = v;
            }
            const int32_t got = sel.validity.binding[i];
            bool ok = got == want && (got >= 0) == (why[i].ok > 0) && why[i].ok == c;
            if (got >= 0) {
                const int32_t store = sel.node_store_index[i];
                ok = ok && store >= 0 && (size_t)store < ctx.node_store.size() &&
                     corev1::name_any(ctx.node_store[(size_t)store].metadata) == ctx.snapshot->columns().names[(size_t)got];
                ++bound;
            } else {
                ok = ok && sel.node_store_index[i] == -1;
            }
            several += c >= 2;
            not_first += got >= 0 && got != first;
            if (!ok && bad++ < 5) std::printf("    pod %u: got %d want %d (c = %u, summary ok = %u)\n", i, got, want, c, why[i].ok);
        }
        CHECK(bad == 0);
        CHECK(bound > 0 && several > 0 && not_first > 0);  // (not vacuous: some pod's comparison chose another node than its first candidate)
        // nothing to warn about: no draw was rejected
        std::vector<std::string> lines;
        ctx.warn = [&](const std::string &l) { lines.push_back(l); };
        warn_rejected(pp, ctx, sel);
        CHECK(lines.empty());
        std::printf("    %u pods x %u nodes: %u bound, %u with two or more feasible nodes, %u bound to another node than candidate 0\n", p, n, bound, several,
                    not_first);
        std::printf("bindings");
        for (uint32_t i = 0; i < p; ++i) std::printf(" %d", sel.validity.binding[i]);
        std::printf("\n");
    });

    run("pick_pack = 0: the sampled pick, draw for draw", [&] {
        Context ctx;
        context_over(obj, ctx);
        CHECK(ctx.pick_pack == 0 && ctx.pick_spread == 0 && !ctx.pick_uniform);  // the defaults
        SplitMixChooser ch(kSeed);
        const BatchSelection sel = select_nodes_for_pods(pp, ctx, ch, /*want_rejected=*/true);
        const uint32_t n = ctx.snapshot->n(), W = ctx.snapshot->mask_words();
        const size_t store = ctx.node_store.size();
        CHECK(sel.samples.size() == (size_t)p * ATTEMPTS && sel.rejected.size() == p && sel.validity.binding.size() == p);
        SplitMixChooser again(kSeed);
        uint32_t bad = 0;
        for (uint32_t i = 0; i < p && sel.samples.size() == (size_t)p * ATTEMPTS && sel.rejected.size() == p; ++i) {
            int32_t want = -1;
            size_t refused = 0;
            bool ok = true;
            for (uint32_t t = 0; t < ATTEMPTS; ++t) {  // ATTEMPTS draws per pod in pod order; the first feasible one wins
                const uint32_t s = ctx.snapshot->canonical_index((uint32_t)*again.choose(store));
                ok = ok && sel.samples[(size_t)i * ATTEMPTS + t] == s;
                if (want >= 0) continue;
                if ((sel.validity.feasible[(size_t)i * W + (s >> 6)] >> (s & 63u)) & 1ull) want = (int32_t)s;
                else ++refused;
            }
            ok = ok && sel.validity.binding[i] == want && sel.rejected[i].size() == refused &&
                 sel.node_store_index[i] == (want >= 0 ? (int32_t)ctx.snapshot->store_index((uint32_t)want) : -1);
            if (!ok && bad++ < 5) std::printf("    pod %u: got %d want %d\n", i, sel.validity.binding[i], want);
        }
        CHECK(bad == 0 && n > 0);
    });

    run("pick_pack together with pick_uniform or pick_spread: refused before anything is evaluated", [&] {
        for (int other = 0; other < 3; ++other) {  // with pick_uniform, with pick_spread, above the maximum
            Context ctx;
            context_over(obj, ctx);
            ctx.pick_pack = other == 2 ? KSCHED_MAX_ATTEMPTS + 1 : kDraws;  // (2: more draws than one call takes)
            ctx.pick_uniform = other == 0;
            ctx.pick_spread = other == 1 ? 2u : 0u;
            SplitMixChooser ch(kSeed);
            bool refused = false;
            try {
                (void)select_nodes_for_pods(pp, ctx, ch, /*want_rejected=*/false);
            } catch (const EncodeError &) {
                refused = true;
            }
            CHECK(refused);
            CHECK(!ctx.snapshot);  // no snapshot was built: nothing reached a device
            SplitMixChooser fresh(kSeed);
            CHECK(*ch.choose(size_t(1) << 32) == *fresh.choose(size_t(1) << 32));  // and no draw was taken
        }
    });
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "objects" && argc > 2) objects_tests(argv[2]);
    else {
        std::printf("usage: pack_pick_tests objects <objects.json>\n");
        return 2;
    }
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
