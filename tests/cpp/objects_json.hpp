// objects_json.hpp -- Kubernetes JSON objects (tests/golden/*_objects.json) -> corev1, the fields the predicates read.  For the C++ tests
// of the host mirror that take a golden object set; header-only.
#pragma once
#include <fstream>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/host/corev1.hpp"
#include "json_min.hpp"

namespace objects_json {
using namespace ksched_host;
using jmin::Value;

inline std::optional<std::string> opt_str(const Value &o, const char *k) {
    const Value *v = o.get(k);
    if (!v) return std::nullopt;
    return v->str;
}
inline corev1::StringMap str_map(const Value &o) {
    corev1::StringMap m;
    for (const auto &[k, v] : o.obj) m[k] = v.str;
    return m;
}
inline corev1::ObjectMeta meta_of(const Value &obj) {
    corev1::ObjectMeta m;
    if (const Value *md = obj.get("metadata")) {
        m.name = opt_str(*md, "name");
        m.namespace_ = opt_str(*md, "namespace");
        if (const Value *l = md->get("labels")) m.labels = str_map(*l);
    }
    return m;
}
inline std::vector<corev1::Container> containers_of(const Value *arr) {
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
inline corev1::Pod pod_of(const Value &o) {
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
inline corev1::Node node_of(const Value &o) {
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
inline Value read_json(const char *path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::stringstream ss;
    ss << f.rdbuf();
    return jmin::parse(ss.str());
}


struct ObjectSet {
    std::vector<corev1::Pod> pods, bound;
    std::vector<corev1::Node> nodes;
};
inline ObjectSet read_objects(const char *path) {
    const Value doc = read_json(path);
    ObjectSet s;
    for (const Value &v : doc.at("pods").arr) s.pods.push_back(pod_of(v));
    for (const Value &v : doc.at("bound").arr) s.bound.push_back(pod_of(v));
    for (const Value &v : doc.at("nodes").arr) s.nodes.push_back(node_of(v));
    return s;
}
}  // namespace objects_json
