// summary_tests.cpp -- explain_unschedulable / format_unschedulable / Context::explain_no_node_found of the host mirror
// (kube_scheduler_rs_reference_amd/host/scheduler.hpp), driven by tests/test_summary_host.py.
//
//   summary_tests format                                   format_unschedulable's text, exactly (no device)
//   summary_tests objects <objects.json> <expected.json>   explain_unschedulable over a golden object set == the counts the Python driver
//                                                          computed with the object-level oracle ([p][4]: ok, resources, selector, taint);
//                                                          expected.json = {"taints": bool, "counts": [[..4..], ...]}
//   summary_tests reconcile                                reconcile_batch / reconcile_batch_sequential on a scripted batch: with the option off
//                                                          the WARN output is what it is without this feature, with it on exactly the NoNodeFound
//                                                          pods gain one line, and it reflects the snapshot the batch was evaluated against
//   (objects / reconcile need a device; run them with KSCHED_SHARDED=1 for the one-device sharded path)
#include <cstdio>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/host/encoder.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/predicates.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/scheduler.hpp"
#include "../../kube_scheduler_rs_reference_amd/host/util.hpp"
#include "json_min.hpp"

using namespace ksched_host;
using jmin::Value;

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

static void check_text(const Unschedulable &u, const std::string &want) {
    const std::string got = format_unschedulable(u);
    if (got != want) {
        ++g_fail;
        std::printf("    FAILED: got \"%s\" want \"%s\"\n", got.c_str(), want.c_str());
    }
}

static void format_tests() {
    run("format_unschedulable", [] {
        // {nodes, ok, not_enough_resources, node_selector_mismatch, taint_not_tolerated}
        check_text({5000, 0, 3120, 1880, 0}, "0/5000 nodes are available: 3120 NotEnoughResources, 1880 NodeSelectorMismatch.");
        check_text({5000, 5000, 0, 0, 0}, "5000/5000 nodes are available");
        check_text({0, 0, 0, 0, 0}, "0/0 nodes are available");
        check_text({10, 1, 2, 3, 4}, "1/10 nodes are available: 2 NotEnoughResources, 3 NodeSelectorMismatch, 4 TaintNotTolerated.");
        check_text({7, 0, 0, 0, 7}, "0/7 nodes are available: 7 TaintNotTolerated.");
        check_text({7, 3, 0, 4, 0}, "3/7 nodes are available: 4 NodeSelectorMismatch.");
        check_text({9, 2, 6, 0, 1}, "2/9 nodes are available: 6 NotEnoughResources, 1 TaintNotTolerated.");
    });
    run("unschedulable_line", [] {
        corev1::Pod p;
        p.metadata.namespace_ = "ns";
        p.metadata.name = "web-0";
        CHECK(unschedulable_line(p, {3, 0, 3, 0, 0}) == "pod ns/web-0 found no node: 0/3 nodes are available: 3 NotEnoughResources.");
    });
}

// ---- Kubernetes JSON objects -> corev1 (the fields the predicates read) ----------------------------------------------------------
static std::optional<std::string> opt_str(const Value &o, const char *k) {
    const Value *v = o.get(k);
    if (!v) return std::nullopt;
    return v->str;
}
static corev1::StringMap str_map(const Value &o) {
    corev1::StringMap m;
    for (const auto &[k, v] : o.obj) m[k] = v.str;
    return m;
}
static corev1::ObjectMeta meta_of(const Value &obj) {
    corev1::ObjectMeta m;
    if (const Value *md = obj.get("metadata")) {
        m.name = opt_str(*md, "name");
        m.namespace_ = opt_str(*md, "namespace");
        if (const Value *l = md->get("labels")) m.labels = str_map(*l);
    }
    return m;
}
static std::vector<corev1::Container> containers_of(const Value *arr) {
    std::vector<corev1::Container> out;
    if (!arr) return out;
    for (const Value &c : arr->arr) {
        corev1::Container k;
        k.name = opt_str(c, "name").value_or("");
        if (const Value *r = c.get("resources")) {
            corev1::ResourceRequirements rr;
            if (const Value *q = r->get("requests")) rr.requests = str_map(*q);
            if (const Value *q = r->get("limits")) rr.limits = str_map(*q);
            k.resources = rr;
        }
        out.push_back(std::move(k));
    }
    return out;
}
static corev1::Pod pod_of(const Value &o) {
    corev1::Pod p;
    p.metadata = meta_of(o);
    if (const Value *s = o.get("spec")) {
        corev1::PodSpec spec;
        spec.containers = containers_of(s->get("containers"));
        spec.init_containers = containers_of(s->get("initContainers"));
        if (const Value *ns = s->get("nodeSelector")) spec.node_selector = str_map(*ns);
        spec.node_name = opt_str(*s, "nodeName");
        if (const Value *t = s->get("tolerations")) {
            std::vector<corev1::Toleration> ts;
            for (const Value &x : t->arr) {
                corev1::Toleration tol;
                tol.key = opt_str(x, "key");
                tol.operator_ = opt_str(x, "operator");
                tol.value = opt_str(x, "value");
                tol.effect = opt_str(x, "effect");
                ts.push_back(tol);
            }
            spec.tolerations = ts;
        }
        p.spec = spec;
    }
    return p;
}
static corev1::Node node_of(const Value &o) {
    corev1::Node n;
    n.metadata = meta_of(o);
    if (const Value *s = o.get("spec")) {
        corev1::NodeSpec spec;
        if (const Value *t = s->get("taints")) {
            std::vector<corev1::Taint> ts;
            for (const Value &x : t->arr) {
                corev1::Taint taint;
                taint.key = opt_str(x, "key").value_or("");
                taint.value = opt_str(x, "value");
                taint.effect = opt_str(x, "effect").value_or("");
                ts.push_back(taint);
            }
            spec.taints = ts;
        }
        n.spec = spec;
    }
    if (const Value *st = o.get("status")) {
        corev1::NodeStatus ns;
        if (const Value *a = st->get("allocatable")) ns.allocatable = str_map(*a);
        n.status = ns;
    }
    return n;
}
static Value read_json(const char *path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::stringstream ss;
    ss << f.rdbuf();
    return jmin::parse(ss.str());
}

static void objects_test(const char *objects_path, const char *expected_path) {
    run("explain_unschedulable == the object-level oracle's counts", [&] {
        const Value doc = read_json(objects_path), exp = read_json(expected_path);
        std::vector<corev1::Pod> pods, bound;
        std::vector<corev1::Node> nodes;
        for (const Value &v : doc.at("pods").arr) pods.push_back(pod_of(v));
        for (const Value &v : doc.at("bound").arr) bound.push_back(pod_of(v));
        for (const Value &v : doc.at("nodes").arr) nodes.push_back(node_of(v));
        std::vector<const corev1::Pod *> pp;
        for (const auto &p : pods) pp.push_back(&p);
        Context ctx;
        auto lister = std::make_shared<StaticPodLister>();
        lister->pods = bound;
        ctx.client = lister;
        ctx.node_store.assign(nodes.rbegin(), nodes.rend());  // store order != canonical order
        ctx.warn = nullptr;
        const bool taints = exp.at("taints").b;
        const std::vector<Unschedulable> got = explain_unschedulable(pp, ctx, taints);
        const auto &want = exp.at("counts").arr;
        CHECK(got.size() == want.size() && got.size() == pods.size());
        size_t bad = 0;
        for (size_t i = 0; i < got.size() && i < want.size(); ++i) {
            const auto &w = want[i].arr;
            const uint32_t e[4] = {(uint32_t)w[0].num, (uint32_t)w[1].num, (uint32_t)w[2].num, (uint32_t)w[3].num};
            const Unschedulable &u = got[i];
            const bool same = u.nodes == nodes.size() && u.ok == e[0] && u.not_enough_resources == e[1] && u.node_selector_mismatch == e[2] &&
                              u.taint_not_tolerated == e[3] && u.ok + u.not_enough_resources + u.node_selector_mismatch + u.taint_not_tolerated == u.nodes;
            if (!same && bad++ < 5)
                std::printf("    pod %zu: got %u/%u res %u sel %u taint %u, want ok %u res %u sel %u taint %u\n", i, u.ok, u.nodes, u.not_enough_resources,
                            u.node_selector_mismatch, u.taint_not_tolerated, e[0], e[1], e[2], e[3]);
        }
        CHECK(bad == 0);
        std::printf("    %zu pods x %zu nodes, taints %s\n", pods.size(), nodes.size(), taints ? "on" : "off");
    });
}

// ---- the scripted batch ----------------------------------------------------------------------------------------------------------
static corev1::Node node(const std::string &name, const char *cpu, const char *mem) {
    corev1::Node n;
    n.metadata.name = name;
    corev1::NodeStatus st;
    std::map<std::string, corev1::Quantity> al;
    al["cpu"] = cpu;
    al["memory"] = mem;
    st.allocatable = al;
    n.status = st;
    return n;
}
static corev1::Pod pod(const std::string &name, const char *cpu, const char *mem) {
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

// Two nodes: `big` takes one pod of a whole core, `small` none.  Pod a draws `big` and is bound there -- which FILLS it --, pod b draws
// `small` five times and finds no node (src/main.rs:116-118), pod c too (and fits nowhere at all).  The batch was evaluated against the
// snapshot in which `big` is still free: b's line must say 1/2 (after the commit it would be 0/2: the order ADVICE r6 is about).
static std::vector<std::string> scripted(bool sequential, bool explain, std::vector<std::pair<std::string, std::string>> *posted = nullptr) {
    Context ctx;
    ctx.client = std::make_shared<StaticPodLister>();
    ctx.node_store = {node("big", "1", "4Gi"), node("small", "100m", "4Gi")};
    std::vector<std::string> lines;
    ctx.warn = [&](const std::string &l) { lines.push_back(l); };
    ctx.explain_no_node_found = explain;
    const std::vector<corev1::Pod> pods = {pod("a", "1", "1Gi"), pod("b", "1", "1Gi"), pod("c", "2", "1Gi")};
    std::vector<const corev1::Pod *> pp;
    for (const auto &p : pods) pp.push_back(&p);
    ScriptedChooser ch;
    ch.script = {0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};  // store order: 0 = big, 1 = small
    OkSink sink;
    const std::vector<ReconcileOutcome> out = sequential ? reconcile_batch_sequential(pp, ctx, ch, sink) : reconcile_batch(pp, ctx, ch, sink);
    CHECK(out.size() == 3 && out[0].ok && out[0].bound_to && *out[0].bound_to == "big");
    CHECK(!out[1].ok && out[1].error == ReconcileError::NoNodeFound && !out[2].ok && out[2].error == ReconcileError::NoNodeFound);
    // the binding did land in the snapshot afterwards: `big` is full now
    const std::vector<Unschedulable> after = explain_unschedulable({&pods[1]}, ctx);
    CHECK(after.size() == 1 && after[0].ok == 0 && after[0].not_enough_resources == 2 && after[0].nodes == 2);
    if (posted) *posted = sink.posted;
    return lines;
}

static void reconcile_tests() {
    const std::vector<std::string> today = {
        // src/main.rs:62 for every rejected draw, pod by pod, then src/main.rs:123 for every failed reconcile
        "Node small failed validity check for pod test/b: NotEnoughResources", "Node small failed validity check for pod test/b: NotEnoughResources",
        "Node small failed validity check for pod test/b: NotEnoughResources", "Node small failed validity check for pod test/b: NotEnoughResources",
        "Node small failed validity check for pod test/b: NotEnoughResources", "Node small failed validity check for pod test/c: NotEnoughResources",
        "Node small failed validity check for pod test/c: NotEnoughResources", "Node small failed validity check for pod test/c: NotEnoughResources",
        "Node small failed validity check for pod test/c: NotEnoughResources", "Node small failed validity check for pod test/c: NotEnoughResources",
        "reconcile failed on pod test/b: NoNodeFound", "reconcile failed on pod test/c: NoNodeFound"};
    for (const bool sequential : {false, true}) {
        const std::string which = sequential ? "reconcile_batch_sequential" : "reconcile_batch";
        run((which + ": option off = today's output").c_str(), [&] {
            std::vector<std::pair<std::string, std::string>> posted;
            const std::vector<std::string> off = scripted(sequential, false, &posted);
            CHECK(off == today);
            CHECK(posted.size() == 1 && posted[0].first == "a" && posted[0].second == "big");
            if (off != today)
                for (const auto &l : off) std::printf("    | %s\n", l.c_str());
        });
        run((which + ": option on = one line per NoNodeFound pod, from the pre-commit snapshot").c_str(), [&] {
            const std::vector<std::string> on = scripted(sequential, true);
            std::vector<std::string> want = today;
            want.insert(want.begin() + 11, "pod test/b found no node: 1/2 nodes are available: 1 NotEnoughResources.");
            want.push_back("pod test/c found no node: 0/2 nodes are available: 2 NotEnoughResources.");
            CHECK(on == want);
            if (on != want)
                for (const auto &l : on) std::printf("    | %s\n", l.c_str());
        });
    }
    run("explain_no_node_found with the WARN level off: nothing is computed, nothing is said", [] {
        Context ctx;
        ctx.client = std::make_shared<StaticPodLister>();
        ctx.node_store = {node("small", "100m", "4Gi")};
        ctx.warn = nullptr;
        ctx.explain_no_node_found = true;
        const corev1::Pod b = pod("b", "1", "1Gi");
        ScriptedChooser ch;
        ch.script = {0, 0, 0, 0, 0};
        OkSink sink;
        const auto out = reconcile_batch({&b}, ctx, ch, sink);
        CHECK(out.size() == 1 && !out[0].ok && out[0].error == ReconcileError::NoNodeFound);
    });
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "format";
    if (mode == "format") format_tests();
    else if (mode == "objects" && argc > 3) objects_test(argv[2], argv[3]);
    else if (mode == "reconcile") reconcile_tests();
    else {
        std::printf("usage: summary_tests format | objects <objects.json> <expected.json> | reconcile\n");
        return 2;
    }
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
