// node_events_tests.cpp -- Snapshot::observe_nodes / Context::observe_nodes (the node-watch twin of observe_pods).
//
//   node_events_tests cpu   event sequences on an encode-only snapshot: after each, the decoded snapshot (available, label values,
//                           taints per node) equals a rebuild from scratch over the final node set; LIST, generation and
//                           strong-guarantee accounting
//   node_events_tests gpu   objects -> events -> reconcile_batch equals reconcile_batch over a snapshot built from scratch
//                           (run it with KSCHED_SHARDED=1 for the one-device sharded path)
#include <cstdio>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/host/encoder.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/scheduler.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/util.hpp"

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

static corev1::Node node(const std::string &name, const char *cpu, const char *mem, std::map<std::string, std::string> labels = {},
                         std::vector<std::pair<std::string, std::string>> taints = {}) {
    corev1::Node n;
    n.metadata.name = name;
    if (!labels.empty()) n.metadata.labels = corev1::StringMap(labels.begin(), labels.end());
    corev1::NodeStatus st;
    std::map<std::string, corev1::Quantity> al;
    if (cpu) al["cpu"] = cpu;
    if (mem) al["memory"] = mem;
    st.allocatable = al;
    n.status = st;
    if (!taints.empty()) {
        corev1::NodeSpec sp;
        sp.taints = std::vector<corev1::Taint>{};
        for (const auto &[k, e] : taints) {
            corev1::Taint t;
            t.key = k;
            t.effect = e;
            sp.taints->push_back(t);
        }
        n.spec = sp;
    }
    return n;
}

static corev1::Pod pod(const std::string &name, const char *cpu, const char *mem, const char *node_name = nullptr,
                       std::map<std::string, std::string> selector = {}) {
    corev1::Pod p;
    p.metadata.namespace_ = "test";
    p.metadata.name = name;
    corev1::PodSpec spec;
    corev1::Container c;
    corev1::ResourceRequirements rr;
    std::map<std::string, corev1::Quantity> req;
    if (cpu) req["cpu"] = cpu;
    if (mem) req["memory"] = mem;
    rr.requests = req;
    c.resources = rr;
    spec.containers.push_back(c);
    if (node_name) spec.node_name = std::string(node_name);
    if (!selector.empty()) spec.node_selector = corev1::StringMap(selector.begin(), selector.end());
    p.spec = spec;
    return p;
}

static const std::string kAbsent = "<no such label>";

// ---- the decoded snapshot ------------------------------------------------------------------------------------------------
struct Decoded {
    std::vector<std::string> names;
    std::vector<__int128> cpu, mem;
    std::map<std::string, std::vector<std::string>> labels;  // key -> per node: value, or kAbsent
    std::vector<std::set<TaintId>> taints;
};

static Decoded decode(const Snapshot &s, const std::vector<corev1::Node> &objects) {
    const NodeColumns &c = s.columns();
    Decoded d;
    d.names = c.names;
    std::map<std::string, const corev1::Node *> by_name;
    for (const auto &o : objects) by_name[corev1::name_any(o.metadata)] = &o;
    for (uint32_t i = 0; i < c.n; ++i) {
        d.cpu.push_back((__int128)c.avail_cpu_milli[i] * s.cpu_unit_nanos());
        d.mem.push_back((__int128)c.avail_mem_bytes[i] * s.mem_unit_nanos());
        std::set<TaintId> t;
        for (const auto &[id, bit] : s.taint_ids())
            if (c.taints[i] >> bit & 1ull) t.insert(id);
        d.taints.push_back(t);
    }
    // label ids -> values: the id of every node must name the value its object carries, one id per value (exact interning)
    for (uint32_t k = 0; k < c.n_keys; ++k) {
        std::map<uint32_t, std::string> value_of;
        std::map<std::string, uint32_t> id_of;
        auto &col = d.labels[c.keys[k]];
        for (uint32_t i = 0; i < c.n; ++i) {
            const uint32_t id = c.label_val_ids[(size_t)k * c.n + i];
            const corev1::Node *o = by_name.at(c.names[i]);
            std::string v = kAbsent;
            if (o->metadata.labels) {
                auto it = o->metadata.labels->find(c.keys[k]);
                if (it != o->metadata.labels->end()) v = it->second;
            }
            CHECK((id == 0) == (v == kAbsent));
            if (id) {
                auto [a, fa] = value_of.emplace(id, v);
                auto [b, fb] = id_of.emplace(v, id);
                CHECK(a->second == v && b->second == id);
                (void)fa;
                (void)fb;
            }
            col.push_back(id ? v : std::string(kAbsent));
        }
    }
    return d;
}

static bool same(const Decoded &a, const Decoded &b) {
    return a.names == b.names && a.cpu == b.cpu && a.mem == b.mem && a.labels == b.labels && a.taints == b.taints;
}

static const std::set<std::string> kKeys = {"zone", "disk"};

// the snapshot a rebuild from scratch over `nodes` gives (encode-only)
static Decoded fresh(const std::vector<corev1::Node> &nodes, const std::vector<corev1::Pod> &pods) {
    Snapshot s(Snapshot::kEncodeOnly);
    s.ensure_keys(kKeys);
    s.enable_taints();
    StaticPodLister l;
    l.pods = pods;
    s.rebuild(nodes, &l);
    return decode(s, nodes);
}

static void check_store_maps(const Context &ctx) {
    const Snapshot &s = *ctx.snapshot;
    CHECK(ctx.node_store.size() == s.n());
    for (uint32_t c = 0; c < s.n() && ctx.node_store.size() == s.n(); ++c) {
        CHECK(corev1::name_any(ctx.node_store[s.store_index(c)].metadata) == s.columns().names[c]);
        CHECK(s.canonical_index(s.store_index(c)) == c);
    }
}

static void cpu_tests() {
    std::vector<corev1::Pod> pods = {pod("p1", "1", "1Gi", "a"), pod("p2", "500m", "512Mi", "b"), pod("p3", "250m", "256Mi", "d"),
                                     pod("p4", "100m", "1Mi", "c")};
    Context ctx;
    ctx.warn = nullptr;
    auto lister = std::make_shared<StaticPodLister>();
    lister->pods = pods;
    ctx.client = lister;
    ctx.node_store = {node("c", "2", "4Gi", {{"zone", "z1"}}), node("a", "4", "8Gi", {{"zone", "z1"}, {"disk", "ssd"}}),
                      node("b", "8", "16Gi", {{"zone", "z2"}, {"disk", "hdd"}}, {{"t1", "NoSchedule"}})};
    ctx.snapshot = std::make_shared<Snapshot>(Snapshot::kEncodeOnly);
    ctx.snapshot->ensure_keys(kKeys);
    ctx.snapshot->enable_taints();
    ctx.snapshot->rebuild(ctx.node_store, lister.get());
    CHECK(lister->list_calls == 3);

    struct Step {
        const char *what;
        std::vector<std::pair<NodeEvent, corev1::Node>> events;
        size_t changed;
        uint64_t lists;  // LISTs the step may issue
        bool moves;      // generation() changes
    };
    auto by_name = [&](const std::string &n) {
        for (const auto &x : ctx.node_store)
            if (corev1::name_any(x.metadata) == n) return x;
        throw std::runtime_error("no node " + n);
    };
    corev1::Node status_only = by_name("a");
    std::vector<Step> steps = {
        {"label change (a: zone z1 -> z2, a value other nodes carry)", {{NodeEvent::Applied, node("a", "4", "8Gi", {{"zone", "z2"}, {"disk", "ssd"}})}}, 1, 0, true},
        {"new label value (c: zone z9)", {{NodeEvent::Applied, node("c", "2", "4Gi", {{"zone", "z9"}})}}, 1, 0, true},
        {"key removed (b: no disk)", {{NodeEvent::Applied, node("b", "8", "16Gi", {{"zone", "z2"}}, {{"t1", "NoSchedule"}})}}, 1, 0, true},
        {"taint added (c: t2 NoExecute)", {{NodeEvent::Applied, node("c", "2", "4Gi", {{"zone", "z9"}}, {{"t2", "NoExecute"}})}}, 1, 0, true},
        {"taint removed (b: t1 gone)", {{NodeEvent::Applied, node("b", "8", "16Gi", {{"zone", "z2"}})}}, 1, 0, true},
        {"allocatable change (a: 4 -> 6 cpus, 8Gi -> 9Gi)", {{NodeEvent::Applied, node("a", "6", "9Gi", {{"zone", "z2"}, {"disk", "ssd"}})}}, 1, 0, true},
        {"status-only Modified (a heartbeat: same object)", {{NodeEvent::Applied, node("a", "6", "9Gi", {{"zone", "z2"}, {"disk", "ssd"}})}}, 0, 0, false},
        {"status-only Modified (a PreferNoSchedule taint, which never filters)",
         {{NodeEvent::Applied, node("a", "6", "9Gi", {{"zone", "z2"}, {"disk", "ssd"}}, {{"soft", "PreferNoSchedule"}})}}, 0, 0, false},
        {"Added (d, with a pod already bound to it)", {{NodeEvent::Applied, node("d", "3", "6Gi", {{"zone", "z1"}, {"disk", "nvme"}})}}, 1, 1, true},
        {"Deleted (b)", {{NodeEvent::Deleted, node("b", "8", "16Gi")}}, 1, 0, true},
        {"Deleted of an unknown node", {{NodeEvent::Deleted, node("zz", "1", "1")}}, 0, 0, false},
        {"a batch: Modified c, Added e, Deleted d, Modified e",
         {{NodeEvent::Applied, node("c", "2", "5Gi", {{"zone", "z1"}})}, {NodeEvent::Applied, node("e", "1", "1Gi")},
          {NodeEvent::Deleted, node("d", "3", "6Gi")}, {NodeEvent::Applied, node("e", "2", "1Gi", {{"disk", "ssd"}})}}, 4, 1, true},
        {"label change of a key no column holds", {{NodeEvent::Applied, node("e", "2", "1Gi", {{"disk", "ssd"}, {"rack", "r1"}})}}, 1, 0, true},
    };
    (void)status_only;
    for (auto &st : steps) {
        run(st.what, [&] {
            std::vector<std::pair<NodeEvent, const corev1::Node *>> ev;
            for (const auto &[k, n] : st.events) ev.emplace_back(k, &n);
            const uint64_t lists = lister->list_calls, gen = ctx.snapshot->generation();
            const size_t changed = ctx.observe_nodes(ev);
            CHECK(changed == st.changed);
            CHECK(lister->list_calls - lists == st.lists);
            CHECK((ctx.snapshot->generation() != gen) == st.moves);
            CHECK(same(decode(*ctx.snapshot, ctx.node_store), fresh(ctx.node_store, pods)));
            check_store_maps(ctx);
        });
    }
    run("EncodeError events change nothing (allocatable without memory; a 65th distinct taint)", [&] {
        const Decoded before = decode(*ctx.snapshot, ctx.node_store);
        const size_t store_n = ctx.node_store.size();
        const uint64_t gen = ctx.snapshot->generation(), lists = lister->list_calls;
        std::vector<corev1::Node> bad = {node("a", "6", nullptr), node("new", "1", nullptr)};
        std::vector<std::pair<std::string, std::string>> many;
        for (int i = 0; i < 70; ++i) many.emplace_back("x" + std::to_string(i), "NoSchedule");
        bad.push_back(node("c", "2", "5Gi", {{"zone", "z1"}}, many));
        for (const auto &b : bad) {
            bool threw = false;
            try {
                ctx.observe_nodes({{NodeEvent::Applied, &b}});
            } catch (const EncodeError &) {
                threw = true;
            }
            CHECK(threw);
        }
        CHECK(ctx.snapshot->generation() == gen && lister->list_calls == lists && ctx.node_store.size() == store_n);
        CHECK(same(decode(*ctx.snapshot, ctx.node_store), before));
        check_store_maps(ctx);
    });
}

// ---- GPU: objects -> events -> reconcile_batch, against a snapshot built from scratch ------------------------------------------
struct RecordingSink : BindingSink {
    std::vector<std::pair<std::string, std::string>> posts;
    bool create_pod_binding(const std::string &pod_name, const std::string &ns, const Binding &b) override {
        posts.push_back({ns + "/" + pod_name, b.target_name});
        return true;
    }
};

static void gpu_tests() {
    run("objects -> node events -> reconcile_batch == reconcile_batch over a fresh snapshot", [&] {
        const char *zones[] = {"z1", "z2", "z3", "z4"};
        std::vector<corev1::Node> nodes;
        std::vector<corev1::Pod> bound;
        for (int i = 0; i < 300; ++i) {
            const std::string nm = "n" + std::to_string(1000 + i);
            nodes.push_back(node(nm, (i % 3) ? "4" : "2", "8Gi", {{"zone", zones[i % 4]}, {"disk", (i % 2) ? "ssd" : "hdd"}}));
            if (i % 5 == 0) bound.push_back(pod("b" + std::to_string(i), "1", "2Gi", nm.c_str()));
        }
        bound.push_back(pod("late", "3", "1Gi", "n9999"));  // on a node that joins later
        std::vector<corev1::Pod> pending;
        for (int i = 0; i < 400; ++i) {
            std::map<std::string, std::string> sel;
            if (i % 3 == 0) sel["zone"] = zones[i % 4];
            if (i % 4 == 1) sel["disk"] = (i % 8 == 1) ? "nvme" : "ssd";
            if (i % 7 == 2) sel["zone"] = "z9";
            pending.push_back(pod("q" + std::to_string(i), (i % 2) ? "1500m" : "500m", "1Gi", nullptr, sel));
        }
        auto make = [&](std::vector<corev1::Node> ns) {
            Context c;
            c.warn = nullptr;
            auto l = std::make_shared<StaticPodLister>();
            l->pods = bound;
            c.client = l;
            c.node_store = std::move(ns);
            c.refresh_snapshot();
            return c;
        };
        Context a = make(nodes);
        // relabels (values new and old), allocatable changes, a node joining (with a bound pod), nodes leaving
        std::vector<corev1::Node> ev_nodes;
        for (int i = 0; i < 300; i += 7) ev_nodes.push_back(node("n" + std::to_string(1000 + i), "4", "8Gi", {{"zone", (i % 2) ? "z9" : "z2"}, {"disk", "nvme"}}));
        for (int i = 3; i < 300; i += 11) ev_nodes.push_back(node("n" + std::to_string(1000 + i), "1", "2Gi", {{"zone", zones[i % 4]}}));
        std::vector<std::pair<NodeEvent, const corev1::Node *>> ev;
        for (const auto &n : ev_nodes) ev.emplace_back(NodeEvent::Applied, &n);
        CHECK(a.observe_nodes(ev) == ev.size());
        CHECK(a.snapshot->n() == 300);
        corev1::Node joins = node("n9999", "8", "16Gi", {{"zone", "z9"}, {"disk", "nvme"}});
        corev1::Node leaves1 = node("n1010", "1", "1"), leaves2 = node("n1100", "1", "1");
        CHECK(a.observe_nodes({{NodeEvent::Applied, &joins}, {NodeEvent::Deleted, &leaves1}, {NodeEvent::Deleted, &leaves2}}) == 3);
        CHECK(a.snapshot->n() == 299);
        Context b = make(a.node_store);
        std::vector<const corev1::Pod *> pp;
        for (const auto &p : pending) pp.push_back(&p);
        SplitMixChooser ca(7), cb(7);
        RecordingSink sa, sb;
        const auto oa = reconcile_batch(pp, a, ca, sa), ob = reconcile_batch(pp, b, cb, sb);
        CHECK(oa.size() == ob.size());
        size_t bound_n = 0;
        for (size_t i = 0; i < oa.size() && i < ob.size(); ++i) {
            CHECK(oa[i].ok == ob[i].ok && oa[i].bound_to == ob[i].bound_to);
            bound_n += oa[i].bound_to.has_value();
        }
        CHECK(sa.posts == sb.posts);
        CHECK(bound_n > 50 && bound_n < pp.size());
        std::printf("    %zu of %zu pods bound, the same nodes through both snapshots\n", bound_n, pp.size());
    });
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "cpu") cpu_tests();
    else if (mode == "gpu") gpu_tests();
    else {
        std::printf("usage: node_events_tests cpu|gpu\n");
        return 2;
    }
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
