// uniform_pick_tests.cpp -- Context::pick_uniform of the host mirror (kube_scheduler_rs_reference_amd/host/scheduler.hpp: extension E3,
// KSCHED_PICK_UNIFORM), driven by tests/test_uniform_host.py.  Every mode needs a device.
//
//   uniform_pick_tests objects <objects.json>   select_nodes_for_pods over a golden object set with the option on and a SplitMixChooser:
//                                               every pod's node is the k-th set bit of its own mask row for its recorded draw, exactly
//                                               the pods with a feasible node (explain_unschedulable) get one, nothing is rejected; with
//                                               the option off the selection is the sampled pick, draw for draw.  Prints the bindings
//                                               ("bindings ...": the driver compares a three-way shard's line with one device's).
//   uniform_pick_tests reconcile                reconcile_batch on a scripted batch: one pod's selector matches exactly one node and
//                                               the scripted sampled draws miss it
//   (run them with KSCHED_SHARDED=n under the test hooks for the row-sharded path)
#include <cstdio>
#include <functional>
#include <map>
#include <string>
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

constexpr uint64_t kSeed = 0xE3E3E3E3ull;

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

    run("pick_uniform: every pod's node is the k-th set bit of its own mask row for its recorded draw", [&] {
        Context ctx;
        context_over(obj, ctx);
        ctx.pick_uniform = true;
        SplitMixChooser ch(kSeed);
        const BatchSelection sel = select_nodes_for_pods(pp, ctx, ch, /*want_rejected=*/true);
        const uint32_t n = ctx.snapshot->n(), W = ctx.snapshot->mask_words();
        CHECK(n == obj.nodes.size() && sel.node_store_index.size() == p && sel.validity.binding.size() == p);
        CHECK(sel.validity.feasible.size() == (size_t)p * W && sel.validity.W == W);
        CHECK(sel.rejected.empty());  // there are no rejected draws
        // the draws: one per pod, in pod order, chooser.choose(2^32)
        CHECK(sel.samples.size() == p);
        SplitMixChooser again(kSeed);
        bool same_draws = sel.samples.size() == p;
        for (uint32_t i = 0; same_draws && i < p; ++i) same_draws = sel.samples[i] == (uint32_t)*again.choose(size_t(1) << 32);
        CHECK(same_draws);
        const std::vector<Unschedulable> why = explain_unschedulable(pp, ctx);
        CHECK(why.size() == p);
        uint32_t bound = 0, several = 0, bad = 0;
        for (uint32_t i = 0; i < p && sel.samples.size() == p && why.size() == p; ++i) {
            uint32_t c = 0;
            (void)kth_set_bit(sel.validity.feasible.data() + (size_t)i * W, n, ~0ull, &c);
            const int32_t want = c ? kth_set_bit(sel.validity.feasible.data() + (size_t)i * W, n, ((uint64_t)sel.samples[i] * c) >> 32, &c) : -1;
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
            if (!ok && bad++ < 5) std::printf("    pod %u: got %d want %d (c = %u, summary ok = %u)\n", i, got, want, c, why[i].ok);
        }
        CHECK(bad == 0);
        CHECK(bound > 0 && several > 0);  // (not vacuous: some pod chose among several nodes)
        // nothing to warn about: no draw was rejected
        std::vector<std::string> lines;
        ctx.warn = [&](const std::string &l) { lines.push_back(l); };
        warn_rejected(pp, ctx, sel);
        CHECK(lines.empty());
        std::printf("    %u pods x %u nodes: %u bound, %u with two or more feasible nodes\n", p, n, bound, several);
        std::printf("bindings");
        for (uint32_t i = 0; i < p; ++i) std::printf(" %d", sel.validity.binding[i]);
        std::printf("\n");
    });

    run("pick_uniform off: the sampled pick, draw for draw", [&] {
        Context ctx;
        context_over(obj, ctx);
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
}

// ---- the scripted batch ----------------------------------------------------------------------------------------------------------
static corev1::Node node(const std::string &name, const char *cpu, const char *mem, const char *disk = nullptr) {
    corev1::Node n;
    n.metadata.name = name;
    if (disk) n.metadata.labels = corev1::StringMap{{"disk", disk}};
    corev1::NodeStatus st;
    std::map<std::string, corev1::Quantity> al;
    al["cpu"] = cpu;
    al["memory"] = mem;
    st.allocatable = al;
    n.status = st;
    return n;
}
static corev1::Pod pod(const std::string &name, const char *cpu, const char *mem, const char *disk = nullptr) {
    corev1::Pod p;
    p.metadata.namespace_ = "test";
    p.metadata.name = name;
    corev1::PodSpec spec;
    corev1::Container c;
    corev1::ResourceRequirements rr;
    std::map<std::string, corev1::Quantity> req;
    req["cpu"] = cpu;
    req["memory"] = mem;
    rr.requests = req;
    c.resources = rr;
    spec.containers.push_back(c);
    if (disk) spec.node_selector = corev1::StringMap{{"disk", disk}};
    p.spec = spec;
    return p;
}
struct OkSink : BindingSink {
    std::vector<std::pair<std::string, std::string>> posted;
    bool create_pod_binding(const std::string &pod_name, const std::string &, const Binding &b) override {
        posted.emplace_back(pod_name, b.target_name);
        return true;
    }
};

// Eight roomy nodes of which only n5 carries disk=ssd; the pod asks for disk=ssd.  The scripted draws 0 .. 4 (store order) all miss n5.
static ReconcileOutcome scripted(bool uniform, std::vector<std::pair<std::string, std::string>> *posted, std::vector<std::string> *lines) {
    Context ctx;
    ctx.client = std::make_shared<StaticPodLister>();
    for (int i = 0; i < 8; ++i) ctx.node_store.push_back(node("n" + std::to_string(i), "8", "32Gi", i == 5 ? "ssd" : "hdd"));
    ctx.warn = [&](const std::string &l) { lines->push_back(l); };
    ctx.pick_uniform = uniform;
    const corev1::Pod a = pod("a", "1", "1Gi", "ssd");
    ScriptedChooser ch;
    ch.script = {0, 1, 2, 3, 4};
    OkSink sink;
    const std::vector<ReconcileOutcome> out = reconcile_batch({&a}, ctx, ch, sink);
    CHECK(out.size() == 1);
    *posted = sink.posted;
    return out.empty() ? ReconcileOutcome{} : out[0];
}

static void reconcile_tests() {
    run("reconcile_batch, option off: the five draws miss the one matching node -> NoNodeFound, as today", [] {
        std::vector<std::pair<std::string, std::string>> posted;
        std::vector<std::string> lines;
        const ReconcileOutcome r = scripted(false, &posted, &lines);
        CHECK(!r.ok && r.error == ReconcileError::NoNodeFound && !r.bound_to && posted.empty());
        CHECK(lines.size() == 6 && lines[0] == "Node n0 failed validity check for pod test/a: NodeSelectorMismatch" &&
              lines[5] == "reconcile failed on pod test/a: NoNodeFound");
    });
    run("reconcile_batch, option on: bound to the one matching node, one POST", [] {
        std::vector<std::pair<std::string, std::string>> posted;
        std::vector<std::string> lines;
        const ReconcileOutcome r = scripted(true, &posted, &lines);
        CHECK(r.ok && r.bound_to && *r.bound_to == "n5");
        CHECK(posted.size() == 1 && posted[0].first == "a" && posted[0].second == "n5");
        CHECK(lines.empty());  // no rejected draw, no failed reconcile
    });
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "objects" && argc > 2) objects_tests(argv[2]);
    else if (mode == "reconcile") reconcile_tests();
    else {
        std::printf("usage: uniform_pick_tests objects <objects.json> | reconcile\n");
        return 2;
    }
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
