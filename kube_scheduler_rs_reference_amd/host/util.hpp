// util.hpp -- host mirror of the reference's `util` module (src/util.rs:1-75).
//
// Same names and meaning as the Rust items they stand for:
//   Context              src/util.rs:12-15   {client, node_store}; gains the device snapshot
//   PodResources         src/util.rs:17-36   {cpu, memory} of ParsedQuantity, new() seeds "0", SubAssign
//   is_pod_bound         src/util.rs:38-45
//   full_name            src/util.rs:47-52
//   total_pod_resources  src/util.rs:54-75   containers only; requests only
// `kube::Client` is reduced to the one call the predicate path makes on it: the LIST of pods with
// field selector spec.nodeName=<node> (src/predicates.rs:21-25,34) -> PodLister.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "corev1.hpp"
#include "quantity.hpp"

namespace ksched_host {

class Snapshot;

// One event of a node WATCH (the reflector behind node_store, src/main.rs:134-139): Applied = Added / Modified (the node as it is now),
// Deleted = Deleted.
enum class NodeEvent { Applied, Deleted };

// The slice of kube::Api<Pod> the path uses (src/predicates.rs:21-34).
struct PodLister {
    virtual ~PodLister() = default;
    // every pod whose spec.nodeName == node_name, any phase (the reference applies no phase filter)
    virtual std::vector<corev1::Pod> list_pods_on_node(const std::string &node_name) = 0;
    uint64_t list_calls = 0;  // observability: how many LISTs were issued
};

// In-memory cluster state: what a fake API server would answer.
struct StaticPodLister : PodLister {
    std::vector<corev1::Pod> pods;
    std::vector<corev1::Pod> list_pods_on_node(const std::string &node_name) override;
};

struct PodResources {
    ParsedQuantity cpu, memory;
    PodResources();  // PodResources::new(): both "0" (src/util.rs:22-29)
    PodResources &operator-=(const PodResources &o) {  // impl SubAssign (src/util.rs:31-36)
        cpu -= o.cpu;
        memory -= o.memory;
        return *this;
    }
};

struct Context {
    std::shared_ptr<PodLister> client;     // pub client: Client
    std::vector<corev1::Node> node_store;  // pub node_store: reflector::Store<Node> (state() = this vector, any order)
    int device = 0;                        // HIP device the evaluator lives on ...
    // ... or several: the batch row-shards over them and the bindings are all-gathered (sharded.hpp).  Empty = $KSCHED_DEVICES
    // ("0,1,2,3" / "all"), and without that variable {device}.  $KSCHED_SHARDED=1 takes the sharded path with one device too.
    std::vector<int> devices;
    // Device-resident snapshot of node_store + LISTs (added field; SURVEY.md section 8b allows it).
    std::shared_ptr<Snapshot> snapshot;
    // one-node scratch snapshot used by the per-pair predicates::* entry points
    std::shared_ptr<Snapshot> pair_snapshot;

    // tracing's WARN level: where the reference's warn!() lines go -- one per rejected candidate (src/main.rs:62: "Node {} failed validity
    // check for pod {}: {:?}") and one per failed reconcile (:123).  The reference's subscriber prints everything up to INFO (:128), so the
    // default writes them to stderr; $KSCHED_LOG=off (or =error) or an empty function switches the level off, and then NOTHING is computed
    // for it: the batched path asks the device for the rejected draws' reasons (ksched_explain) only when somebody listens.
    std::function<void(const std::string &)> warn = default_warn_sink();

    // Opt-in (default off): with the WARN level on, reconcile_batch / reconcile_batch_sequential follow every NoNodeFound pod's
    // "reconcile failed" line with one line saying why -- "pod ns/name found no node: 0/5000 nodes are available: 3120 NotEnoughResources,
    // 1880 NodeSelectorMismatch." (scheduler.hpp: explain_unschedulable) -- from ONE ksched_summarize call per batch over exactly those pods,
    // against the snapshot the batch was evaluated against.  Off: not one byte of output and no device call changes.
    bool explain_no_node_found = false;

    // Opt-in (default off; extension E3): select_nodes_for_pods -- and with it reconcile_batch / reconcile_batch_sequential -- picks
    // UNIFORMLY AMONG EACH POD'S FEASIBLE NODES on the device (KSCHED_PICK_UNIFORM) instead of testing ATTEMPTS blind draws: a pod ends
    // with NoNodeFound only when no node passes.  One draw per pod, chooser.choose(2^32), in pod order.  Outside the parity claim (the
    // reference tests five blind draws, src/main.rs:51-71).  Off: nothing changes, draw for draw.
    bool pick_uniform = false;

    // Opt-in (0 = off, the default; extension E4): select_nodes_for_pods picks THE LEAST LOADED OF d = pick_spread UNIFORMLY DRAWN FEASIBLE
    // NODES on the device (KSCHED_PICK_SPREAD; 1 <= d <= KSCHED_MAX_ATTEMPTS): d draws per pod, chooser.choose(2^32), in pod order and
    // draw-major within a pod; the largest (available memory, available cpu) of the snapshot the batch is evaluated against wins, the
    // lowest node index among equals.  Not together with pick_uniform: refused before anything is evaluated.  Outside the parity claim.
    // 0: nothing changes, draw for draw.
    uint32_t pick_spread = 0;

    // Opt-in (0 = off, the default; extension E5): select_nodes_for_pods picks THE TIGHTEST OF d = pick_pack UNIFORMLY DRAWN FEASIBLE NODES
    // on the device (KSCHED_PICK_PACK; 1 <= d <= KSCHED_MAX_ATTEMPTS): pick_spread's draws -- d per pod, chooser.choose(2^32), in pod order
    // and draw-major within a pod -- with the comparison turned round: the smallest (available memory, available cpu) wins, the lowest node
    // index among equals.  Not together with pick_uniform or pick_spread: refused before anything is evaluated.  Outside the parity claim.
    // 0: nothing changes, draw for draw.
    uint32_t pick_pack = 0;

    // (Re)build `snapshot` from node_store and one LIST per node.
    void refresh_snapshot();
    // Keep node_store and the snapshot current from node watch events, the way the reflector's writer does: an Applied node already in
    // the store is replaced in place, an unknown one appended, a Deleted one erased.  The snapshot follows (Snapshot::observe_nodes,
    // its store <-> canonical maps included) and is changed first: on EncodeError neither has changed.  Without a snapshot yet only
    // node_store changes (the next refresh_snapshot builds it).  Returns how many events changed what the predicates read.
    size_t observe_nodes(const std::vector<std::pair<NodeEvent, const corev1::Node *>> &events);

    static std::function<void(const std::string &)> default_warn_sink();
};

bool is_pod_bound(const corev1::Pod &pod);
std::string full_name(const corev1::ObjectMeta &meta);
PodResources total_pod_resources(const corev1::Pod &pod);

}  // namespace ksched_host
