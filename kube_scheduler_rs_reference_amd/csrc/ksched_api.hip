// ksched_api.hip -- implementation of include/ksched.h (C ABI) on HIP for gfx950.
//
// Host side of the evaluator: owns the device-resident node snapshot and its indexes, launches
// the mask kernels and the pick kernels.  There is deliberately NO CPU implementation of the
// predicates in this library: without a HIP device ksched_create fails with KSCHED_E_NODEVICE.
#include "../../include/ksched.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <numeric>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>


#include "apply_plan.hpp"
#include "bestfit_layout.hpp"
#include "comm_rccl.hpp"
#include "eval_plan.hpp"
#include "eval_request.hpp"
#include "kernels_build.hpp"
#include "kernels_direct.hpp"
#include "kernels_fused.hpp"
#include "kernels_pick_uniform.hpp"
#include "kernels_summary.hpp"
#include "kernels_pick_spread.hpp"  // (uses kernels_pick_uniform.hpp's helpers)
#include "kernels_pick_pack.hpp"    // (k_pick_spread's body with the comparison turned round)
#include "kernels_combine.hpp"      // (extension E6: the scratch mask folded into the caller's mask)
#include "kernels_combine_soft.hpp" // (extension E7: ... row by row, unless that would leave the row empty)
#include "kernels_sel_walk.hpp"     // (what the three selector kernels share, and their one launch path)
#include "kernels_selop.hpp"        // (extension E8: the mask of an operator call -- Exists, Gt, Lt)
#include "kernels_seltag.hpp"       // (extension E9: the mask of a tagged call -- the operator per pod and key)
#include "kernels_selterms.hpp"     // (extension E10: ... with a term count -- the OR of several tagged rows per pod)
#include "mask_alloc.hpp"
#include "merge_sort_plan.hpp"
#include "pipe_plan.hpp"
#include "snapshot_change.hpp"
#include "stream_order.hpp"
#include "tile_index.hpp"

using namespace ksched;

static_assert(kListBytes == 6144u && kTileNodes == 1024, "k_pick_bestfit_listed (kernels_direct.hpp) addresses the tile lists with these sizes");
static_assert(kChangeTileNodes == (uint32_t)kTileNodes, "snapshot_change.hpp lists the tiles an update touches");
static_assert(kApplyTileNodes == (uint32_t)kTileNodes && kApplyIdleClaim == kApplyUnclaimed, "apply_plan.hpp sizes the commit by the tile and bounds the global pod indexes by the idle claim");
static_assert(sizeof(BestfitRowsArgs::lvl_off) == 4 * kBfMaxLevels && sizeof(BfLevelsArgs::lvl_off) == 4 * kBfMaxLevels, "bestfit_layout.hpp sizes the level arrays the kernels carry");

namespace {

// a device allocation that grows on demand and is released with its owner (the owner's device must be current then: ksched_destroy)
template <class T>
struct DevBuf {
    T *ptr = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }  // (move-only: the copy operations are deleted with these two declared)
    DevBuf &operator=(DevBuf &&o) noexcept {  // `o` leaves with what this one held, and releases it
        std::swap(ptr, o.ptr);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void **)&ptr, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
};

// the two ping-pong sets of one device merge sort (merge_sort_plan.hpp names them kSet0 / kSet1; launch_merge_sort walks a plan over
// them).  Best fit and the apply each own one, with their own sizes and growth rules.
struct SortScratch {
    DevBuf<int64_t> k0[2], k1[2];
    DevBuf<uint32_t> idx[2];
    bool holds(size_t n) const { return n <= k0[0].cap && n <= k0[1].cap && n <= idx[0].cap && n <= idx[1].cap; }
    hipError_t reserve(size_t n, bool second_key) {
        hipError_t e = hipSuccess;
        for (int b = 0; b < 2 && e == hipSuccess; ++b) {
            e = k0[b].reserve(n);
            if (e == hipSuccess && second_key) e = k1[b].reserve(n);
            if (e == hipSuccess) e = idx[b].reserve(n);
        }
        return e;
    }
};

// ---- the best-fit index: buffers and state ("the best-fit pick" below builds it and launches over it) -------------------------
// Everything a PICK_BESTFIT request reads beyond the snapshot's columns, sized by bestfit_layout.hpp.  Built lazily, by the first
// PICK_BESTFIT request after the snapshot changed: order_stale = the order (and with it everything) is stale, rows_stale = only the
// row bitmaps are (labels or taints changed, `available` did not).
struct BestfitIndex {
    DevBuf<uint32_t> bf_order, bf_rank;  // node at best-fit position i, and the inverse
    DevBuf<int64_t> bf_mem, bf_cpu;      // node columns once more, in best-fit order
    DevBuf<int64_t> cpu_sorted;          // ascending avail_cpu (rank of a cpu request)
    DevBuf<uint32_t> by_cpu, cpurank;    // node with cpu rank r, and the inverse
    DevBuf<int64_t> samples;             // sample arrays of bf_mem and cpu_sorted (BfOrderLayout)
    DevBuf<int64_t> levels;              // 8-ary level arrays of bf_mem / cpu_sorted (k_pick_bestfit_lanes)
    DevBuf<uint64_t> rows;               // [rows][Wbf] bitmaps over best-fit positions (k_pick_bestfit_rows); built with the tile index's row numbering
    SortScratch sort;                    // the orders' merge sort (bestfit_sort), n records with both keys
    DevBuf<uint32_t> handover;           // the two-stage pick's hand-over (BfHandoverLayout): counter sets in rotation, the listed mask, the sub-lists' 64-byte records
    DevBuf<uint64_t> trace;              // KSCHED_OPT_DEBUG bit 20: per-wave time stamps of the two stages (tools/bestfit_ab.py --trace)
    BfOrderLayout order;  // as of the latest build_bestfit
    BfRowLayout row;      // as of the latest build_bestfit_rows (rows_built)
    BfRotation rotation;  // which counter set of `handover` the next two-stage pick uses
    bool rows_built = false;
    bool order_stale = true, rows_stale = false;

    // the five arrays ksched_set_nodes reserves with the snapshot's columns; the lazy build reserves the rest
    hipError_t reserve_for(uint32_t n) {
        hipError_t e = bf_order.reserve(n);
        if (e == hipSuccess) e = bf_rank.reserve(n);
        if (e == hipSuccess) e = bf_mem.reserve(bf_searched_elems(n));
        if (e == hipSuccess) e = bf_cpu.reserve(n);
        if (e == hipSuccess) e = cpu_sorted.reserve(bf_searched_elems(n));
        return e;
    }
    // a committed snapshot change (SnapshotChange::commit)
    void mark(Stale what) {
        if (stale_order(what)) order_stale = true;
        if (stale_rows_only(what)) rows_stale = true;
        if (what == Stale::kEverything) rows_built = false;
    }
    bool stale() const { return order_stale || rows_stale; }
};

// ---- the apply's state (ksched_apply_bindings_device and its sharded forms, "applying a batch's bindings" below) ---------------
// The per-node scratch, idle between calls and sized by plan_apply_scratch (apply_plan.hpp), the receive buffer of the sharded
// forms, and the sort scratch of KSCHED_APPLY_WHILE_FIT.
struct ApplyState {
    DevBuf<uint64_t> acc;    // [scratch.n][4] split sums, idle 0
    DevBuf<uint32_t> claim;  // [scratch.n] lowest eligible pod index, idle 0xFFFFFFFF
    DevBuf<uint8_t> ovf;     // [scratch.n]
    DevBuf<uint32_t> dirty;  // [tiles of scratch.n + 1] dirty-tile generations, initially 0
    DevBuf<uint64_t> gath;   // ksched_apply_bindings_sharded*: every rank's acc [nranks][n][4] (or claims [nranks][n] uint32)
    ApplyScratch scratch;    // nodes the scratch holds in its idle state, and the generation of the latest call
    SortScratch admit_sort;  // KSCHED_APPLY_WHILE_FIT: the (node, pod) merge sort, no second key, grown on demand
    hipEvent_t ev = nullptr;  // the caller's stream, when the change rides another one (apply_order_begin)

    // a change that stopped halfway (SnapshotChange): the scratch may not be idle
    void invalidate() { scratch.invalidate(); }
    // the scratch in its idle state for n nodes, and the next generation; the (re)allocation and its memsets run once per snapshot
    // size, on `s`.  A failure leaves the scratch unknown.
    hipError_t ready(uint32_t n, hipStream_t s) {
        const ApplyScratchStep st = plan_apply_scratch(scratch, n);
        if (st.allocate) {
            scratch.invalidate();
            hipError_t e = acc.reserve(st.acc_elems);
            if (e == hipSuccess) e = claim.reserve(st.claim_elems);
            if (e == hipSuccess) e = ovf.reserve(st.ovf_elems);
            if (e == hipSuccess) e = dirty.reserve(st.dirty_elems);
            if (e == hipSuccess) e = hipMemsetAsync(acc.ptr, 0, st.acc_bytes, s);
            if (e == hipSuccess) e = hipMemsetAsync(claim.ptr, 0xFF, st.claim_bytes, s);
            if (e == hipSuccess) e = hipMemsetAsync(dirty.ptr, 0, st.dirty_bytes, s);
            if (e != hipSuccess) return e;
        }
        scratch = st.next;
        return hipSuccess;
    }
    // the admit's two sets for the plan's rows, regrown to its capacity when they do not hold them
    hipError_t reserve_admit(const ApplyRankPlan &pl) {
        return admit_sort.holds(pl.admit_rows) ? hipSuccess : admit_sort.reserve(pl.admit_cap, false);
    }
};

// what the ctx keeps per stream evaluations are enqueued on: the registry is stream_order.hpp's, one entry and one lookup per stream
struct StreamRes {
    hipEvent_t ev = nullptr;  // recorded on the stream when a snapshot change has to wait for what it holds (the ctx's own stream: none)
    // per-pod accumulators of the tile-test pick (kernels_fused.hpp PICK == 2): all zero between launches (the kernel zeroes what it
    // used); one buffer per stream, so that launches on different streams may overlap
    DevBuf<uint64_t> pick_acc;
};

}  // namespace

struct ksched_ctx {
    int device = 0;
    std::mutex mu;
    std::string last_error;
    hipStream_t stream = nullptr;  // used by the host-pointer entry points

    // node snapshot
    bool have_nodes = false;
    uint32_t n = 0, nkeys = 0, W = 0;
    bool have_taints = false;
    DevBuf<int64_t> ncpu, nmem;
    DevBuf<int64_t> nrec;  // 64-byte node records (kernels_direct.hpp): one cache line per candidate for the candidate-testing picks
    DevBuf<uint32_t> nlab;
    DevBuf<uint64_t> ntaint;
    BestfitIndex bestfit;  // the best-fit orders, rows and hand-over scratch, built lazily (ensure_bestfit)
    IndexedSnapshot idx;  // per-tile bitmap index (tile_index.hpp), built on the device (kernels_build.hpp)
    // what the index layout was planned for (index_plan), indexed or not: per key the largest id, and every taint bit; a label
    // update whose ids and bits stay within them keeps the layout
    uint32_t plan_lab_max[KSCHED_MAX_KEYS] = {};
    uint64_t plan_taints = 0;
    ApplyState apply;  // ksched_apply_bindings_device and its sharded forms: per-node scratch, receive buffer, the admit's sort scratch
    std::string index_reason;  // why the snapshot has no bitmap index (the fused kernel is then not applicable)
    // host -> device staging for the snapshot calls: pinned, so the copies are asynchronous on the change stream
    uint8_t *h_stage = nullptr;
    size_t h_stage_cap = 0;
    hipEvent_t ev_stage = nullptr;  // the last copy out of h_stage
    DevBuf<uint8_t> d_stage;
    // Every stream wait of the ctx is decided by stream_order.hpp (which stream carries a snapshot change, who waits for whom); the helpers
    // under "stream ordering" below execute its answers with these events and the per-stream ones in StreamRes.
    StreamOrder<StreamRes> order;
    hipEvent_t ev_build = nullptr;    // behind every snapshot change, on the stream that carried it
    hipEvent_t ev_scratch = nullptr;  // the scratch owner's last use, when the ctx-owned scratch changes hands

    // scratch for the host-pointer path
    DevBuf<int64_t> pcpu, pmem;
    DevBuf<uint32_t> psel, psamples;
    DevBuf<uint64_t> ptol, feas, fit;
    DevBuf<int32_t> binding;
    DevBuf<int32_t> gathered;  // ksched_gather_buffer: the all-gathered binding table of a host that drives several devices
    DevBuf<uint32_t> xpairs;  // ksched_explain: [pair_pod][pair_node]
    DevBuf<int32_t> xreason;
    DevBuf<uint64_t> sum_part;  // ksched_summarize*: [tiles][p] per-tile counts of the indexed kernel (scratch: one stream at a time, scratch_enter)
    DevBuf<uint32_t> sum_out;   // ksched_summarize: the [p][4] table of the host-pointer form
    // scratch mask when a pick is requested without an output mask
    DevBuf<uint64_t> scratch_mask;

    // options
    int opt_kernel = KSCHED_KERNEL_AUTO;
    uint32_t opt_timing = 0;       // 0 off, N: every N-th mask launch carries events
    uint64_t timing_seq = 0;
    uint32_t opt_debug = 0;
    bool opt_trace = false;
    bool opt_pick_from_mask = false;
    int opt_fused_pick = 1;       // KSCHED_OPT_FUSED_PICK: 0 = the pick is its own launch, 1 = it rides in the fused mask launch (the form is chosen
                                  // by the request), 2 = ... only as waves of the fill, 3 = ... only as tile tests
    int opt_pipe_mode = 0;        // KSCHED_OPT_PIPE_MODE: 0 split (mask stream / pick stream), m >= 1 alternate (whole steps, stream = slot % max(2, m))
    int opt_round_order = 0;      // KSCHED_OPT_ROUND_ORDER: 0 interleaved wave-major (default), 1 blocked, 2 interleaved chunk-major
    uint32_t opt_mask_probe = 6;  // KSCHED_OPT_MASK_PROBE: candidates of ksched_mask_alloc's probe-and-keep path
    double mask_probe_us[16] = {};  // what the latest probe measured per candidate (diagnostics: ksched_last_error carries them as text)
    uint32_t opt_grid_cus = 0;    // KSCHED_OPT_GRID_CUS: compute units ONE fused mask launch may occupy (0 = the whole chip)
    uint32_t fault_kind = 0, fault_skip = 0;  // KSCHED_OPT_FAULT (test hook of the no-unwind rule)
    int opt_bestfit_stages = 0;  // KSCHED_OPT_BESTFIT_STAGES: 0 auto, 1 one stage, 2 two stages
    int opt_index_build = 0;  // KSCHED_OPT_INDEX_BUILD: 0 = device kernels (default), 1 = host spec (tile_index.hpp)
    DevBuf<uint64_t> trace;
    uint32_t trace_blocks_last = 0;
    const char *last_kernel = "none";
    const char *last_pick = "none";  // how the latest evaluation's pick ran (ksched_last_pick)

    // timing
    struct EvPair {
        hipEvent_t a, b;
    };
    std::vector<EvPair> ev_pool;
    size_t ev_used = 0;
};

namespace {

// ---- nothing unwinds across the C ABI (include/ksched.h "Conventions") -----------------------------------------------------
// Every extern "C" body below is a function-try-block ending in KSCHED_ABI_CATCH: the library's own C++ (std::vector,
// std::string, std::mutex) may throw -- std::bad_alloc above all -- and an exception leaving an extern "C" function
// called from Rust or C is an abort.  bad_alloc -> KSCHED_E_NOMEM, anything else -> KSCHED_E_INVAL, text in ksched_last_error.
int abi_caught(ksched_ctx *c, int code, const char *what) noexcept {
    if (c) {
        try {  // (the body's lock_guard was released by the unwinding)
            std::lock_guard<std::mutex> lk(c->mu);
            c->last_error.assign("exception inside the library: ");
            c->last_error.append(what ? what : "?");
        } catch (...) {  // no memory for the text either: the code alone has to do
        }
    }
    return code;
}
#define KSCHED_ABI_CATCH(CTX)                                                                          \
    catch (const std::bad_alloc &) { return abi_caught((CTX), KSCHED_E_NOMEM, "std::bad_alloc"); }      \
    catch (const std::exception &e_) { return abi_caught((CTX), KSCHED_E_INVAL, e_.what()); }           \
    catch (...) { return abi_caught((CTX), KSCHED_E_INVAL, "unknown exception"); }

// KSCHED_OPT_FAULT: the test hook.  Called (with the ctx's mutex held) at the points where the library's C++ is entered.
void fault_point(ksched_ctx *c) {
    if (!c->fault_kind) return;
    if (c->fault_skip) {
        --c->fault_skip;
        return;
    }
    const uint32_t kind = c->fault_kind;
    c->fault_kind = 0;  // one shot
    if (kind == 1u) throw std::bad_alloc();
    throw std::runtime_error("injected fault (KSCHED_OPT_FAULT)");
}

int fail_hip(ksched_ctx *c, hipError_t e, const char *what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    c->last_error = buf;
    return e == hipErrorOutOfMemory ? KSCHED_E_NOMEM : KSCHED_E_HIP;
}

#define HIPCHK(ctx, call)                                   \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return fail_hip(ctx, e_, #call); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int timing_slot(ksched_ctx *c, size_t *slot) {
    if (c->ev_used == c->ev_pool.size()) {
        // Timing-only events: without the system-scope fence a default event performs when it is recorded (a cache
        // write-back / invalidate around the very kernel being measured: +2 us at C3 and a cold L2 for its tables).
        // KSCHED_TIMING_EVENT_FLAGS overrides the flags (A/B of that effect, tools/).
        unsigned flags = hipEventDisableSystemFence;
        if (const char *e = getenv("KSCHED_TIMING_EVENT_FLAGS")) flags = (unsigned)strtoul(e, nullptr, 0);
        ksched_ctx::EvPair ep;
        HIPCHK(c, hipEventCreateWithFlags(&ep.a, flags));
        HIPCHK(c, hipEventCreateWithFlags(&ep.b, flags));
        c->ev_pool.push_back(ep);
    }
    *slot = c->ev_used++;
    return KSCHED_OK;
}

// ---- stream ordering: the executors of stream_order.hpp's answers (ksched_ctx::order) -------------------------------------------
// Each asks the header, issues exactly the HIP calls the answer names and tells it what went through; the decisions, and the
// reasons for them, are in the header.

inline hipStream_t hip_stream_of(StreamKey s) { return (hipStream_t) const_cast<void *>(s); }
// where the snapshot change in progress is enqueued (snapshot_begin decides, the build / patch code uses it, snapshot_end records ev_build there)
inline hipStream_t change_stream(const ksched_ctx *c) { return hip_stream_of(c->order.change_stream()); }

// `s` waits for the latest snapshot change (ev_build) and has then met it
int stream_wait_build(ksched_ctx *c, hipStream_t s) {
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_build, 0));
    c->order.met(s);
    return KSCHED_OK;
}

// an evaluation is about to be enqueued on `s`: remembered for the next snapshot change, behind the latest one
int stream_enter(ksched_ctx *c, hipStream_t s) {
    const EnterPlan pl = c->order.plan_enter(s);
    if (pl.is_new) {
        StreamRes r;
        HIPCHK(c, hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
        c->order.add(s, std::move(r));
    }
    return pl.wait_build ? stream_wait_build(c, s) : KSCHED_OK;
}

// `s` is about to enqueue work that uses the ctx-owned scratch buffers
int scratch_enter(ksched_ctx *c, hipStream_t s) {
    const ScratchPlan pl = c->order.plan_scratch(s);
    if (pl.step == ScratchStep::kRecordOwnerAndWait) HIPCHK(c, hipEventRecord(c->ev_scratch, hip_stream_of(pl.owner)));
    if (pl.step != ScratchStep::kNothing) HIPCHK(c, hipStreamWaitEvent(s, c->ev_scratch, 0));
    c->order.scratch_taken(s);
    return KSCHED_OK;
}

void stream_forget(ksched_ctx *c, hipStream_t s) {
    // (its launches are ordered before whatever the caller does to the stream next: freeing is safe after a sync there; hipFree
    // synchronises the device itself)
    if (StreamRes *r = c->order.res(s)) r->pick_acc.release();
    bool recorded = false;
    if (c->order.plan_forget(s).record_scratch) {
        recorded = hipEventRecord(c->ev_scratch, s) == hipSuccess;
        if (!recorded) (void)hipGetLastError();
    }
    StreamRes gone;
    if (c->order.forget(s, recorded, &gone)) (void)hipEventDestroy(gone.ev);
}

// Before the snapshot changes: the stream that carries the change (ksched_ctx::order.change_stream()) and what it first waits for
int snapshot_begin(ksched_ctx *c) {
    StreamOrder<StreamRes> &o = c->order;
    const ProbePlan pr = o.plan_probe();
    bool alive = false;
    if (pr.probe) {  // host-side
        const hipError_t q = hipStreamQuery(hip_stream_of(pr.stream));
        alive = q == hipSuccess || q == hipErrorNotReady;
        if (!alive) (void)hipGetLastError();
    }
    const BeginPlan pl = o.begin(alive);
    const hipStream_t s = hip_stream_of(pl.carrier);
    if (pl.carrier_waits_build)
        if (int rc = stream_wait_build(c, s)) return rc;
    if (!pl.record_callers) return KSCHED_OK;
    for (size_t i = 0; i < o.callers();) {
        if (hipEventRecord(o.caller_res(i).ev, hip_stream_of(o.caller(i))) != hipSuccess) {  // the caller destroyed that stream
            (void)hipGetLastError();
            const StreamRes gone = o.drop(i);
            (void)hipEventDestroy(gone.ev);
            continue;
        }
        HIPCHK(c, hipStreamWaitEvent(s, o.caller_res(i).ev, 0));
        ++i;
    }
    return KSCHED_OK;
}

// after the change has been enqueued on the change stream: ev_build marks it for every other stream
int snapshot_end(ksched_ctx *c) {
    HIPCHK(c, hipEventRecord(c->ev_build, hip_stream_of(c->order.change_stream())));
    c->order.committed();
    return KSCHED_OK;
}

// An apply whose caller stream is `hs`, behind snapshot_begin: the change also waits for what `hs` holds ...
int apply_order_begin(ksched_ctx *c, hipStream_t hs) {
    if (!c->order.plan_apply(hs).change_waits_hs) return KSCHED_OK;
    if (!c->apply.ev) HIPCHK(c, hipEventCreateWithFlags(&c->apply.ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->apply.ev, hs));
    HIPCHK(c, hipStreamWaitEvent(hip_stream_of(c->order.change_stream()), c->apply.ev, 0));
    return KSCHED_OK;
}

// ... and behind snapshot_end, `hs` waits for the change (the caller reads status_out there)
int apply_order_end(ksched_ctx *c, hipStream_t hs) { return c->order.plan_apply(hs).hs_waits_change ? stream_wait_build(c, hs) : KSCHED_OK; }

// Every change of the node snapshot, in three calls: begin -> stage, fill, upload (a change that brings data) ->
// the caller's kernels on change_stream -> commit.  A change can stop halfway, by an error return or a throw: once armed, the ctx
// refuses evaluations until its next ksched_set_nodes unless the change is committed -- columns, index and apply scratch may disagree.
struct SnapshotChange {
    ksched_ctx *c = nullptr;
    bool done = false;
    ~SnapshotChange() {
        if (c && !done) {
            c->have_nodes = false;
            c->apply.invalidate();
        }
    }
    // (ksched_set_nodes alone is armed from the start, SnapshotChange chg{c}: whatever stops it, the old snapshot is gone)
    // Evaluations already enqueued read the snapshot as it was (snapshot_begin: events, no host wait; it chooses change_stream).  A
    // failure up to here leaves the snapshot as it was, one after it does not.
    int begin(ksched_ctx *ctx) {
        if (int rc = snapshot_begin(ctx)) return rc;
        c = ctx;
        return KSCHED_OK;
    }
    // The pinned block, `bytes` long, whose previous use (an async copy) has completed -- the caller fills it after a StageLayout --
    // and the device block (ksched_ctx::d_stage) for its first `dev_bytes` bytes.
    int stage(size_t bytes, size_t dev_bytes, uint8_t **h) {
        if (c->h_stage) HIPCHK(c, hipEventSynchronize(c->ev_stage));
        if (bytes > c->h_stage_cap) {
            if (c->h_stage) (void)hipHostFree(c->h_stage);
            c->h_stage = nullptr;
            c->h_stage_cap = 0;
            const size_t cap = std::max<size_t>(bytes + bytes / 4, 1u << 16);
            HIPCHK(c, hipHostMalloc((void **)&c->h_stage, cap, hipHostMallocDefault));
            c->h_stage_cap = cap;
        }
        *h = c->h_stage;
        HIPCHK(c, c->d_stage.reserve(dev_bytes));
        return KSCHED_OK;
    }
    // the pinned block's first `dev_bytes` bytes -> the device block, one copy on the change stream; ev_stage: the last copy out of the
    // pinned block (the caller's own copies out of it come before this call)
    int upload(size_t dev_bytes) {
        const hipStream_t s = change_stream(c);
        if (dev_bytes) HIPCHK(c, hipMemcpyAsync(c->d_stage.ptr, c->h_stage, dev_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipEventRecord(c->ev_stage, s));
        return KSCHED_OK;
    }
    // everything is enqueued: mark what the change made stale (the best-fit structures are rebuilt by the next PICK_BESTFIT request,
    // ensure_bestfit, not here), let the other streams see the change (snapshot_end), validate the snapshot
    int commit(Stale what) {
        c->bestfit.mark(what);
        if (int rc = snapshot_end(c)) return rc;
        c->have_nodes = true;
        done = true;
        return KSCHED_OK;
    }
};

// ---- index and best-fit build (kernels_build.hpp) --------------------------------------------------------------------

// (re)build the fit part of the listed tiles (or of every tile: tiles == nullptr) on the change stream
int launch_build_fit(ksched_ctx *c, const uint32_t *d_tile_list, uint32_t count, const uint32_t *d_dirty = nullptr) {
    const IndexedLayout &l = c->idx.lay;
    BuildFitArgs a{};
    a.ncpu = c->ncpu.ptr;
    a.nmem = c->nmem.ptr;
    a.tables = c->idx.d_tables;
    a.aux = c->idx.d_aux;
    a.tile_list = d_tile_list;
    a.dirty = d_tile_list ? nullptr : d_dirty;  // (every tile's block is launched; the clean ones exit at once)
    a.n = l.n;
    a.rows = l.rows;
    a.row_cpu = l.row_cpu;
    hipLaunchKernelGGL(k_build_tile_fit, dim3(d_tile_list ? count : l.tiles, 2), dim3(1024), 0, change_stream(c), a);
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// (re)build the list keys' slots of the listed tiles (or of every tile: d_tile_list == nullptr) on the change stream
int launch_build_lists(ksched_ctx *c, const uint32_t *d_tile_list = nullptr, uint32_t count = 0) {
    const IndexedLayout &l = c->idx.lay;
    if (l.nlist == 0) return KSCHED_OK;
    BuildListArgs a{};
    a.nlab = c->nlab.ptr;
    a.lists = c->idx.d_list;
    a.tile_list = d_tile_list;
    a.n = l.n;
    a.nlist = l.nlist;
    for (uint32_t j = 0; j < l.nlist; ++j) a.list_col[j] = l.list_col[j];
    hipLaunchKernelGGL(k_build_tile_list, dim3(d_tile_list ? count : l.tiles, l.nlist), dim3(1024), 0, change_stream(c), a);
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// (re)build the named rows (valid, taint, label) of the listed tiles (or of every tile: d_tile_list == nullptr)
int launch_build_named(ksched_ctx *c, const uint32_t *d_tile_list = nullptr, uint32_t count = 0) {
    const IndexedLayout &l = c->idx.lay;
    BuildNamedArgs a{};
    a.nlab = c->nlab.ptr;
    a.ntaint = c->have_taints ? c->ntaint.ptr : nullptr;
    a.tables = c->idx.d_tables;
    a.lab_meta = c->idx.d_lab_meta;
    a.tile_list = d_tile_list;
    a.n = l.n;
    a.rows = l.rows;
    a.nkeys = l.nkeys;
    a.ngroups = l.ngroups;
    a.row_valid = l.row_valid;
    a.row_taint = l.row_taint;
    a.named_rows = l.row_cpu;
    const uint32_t lds = l.row_cpu * 128u;
    HIPCHK(c, hipFuncSetAttribute((const void *)k_build_tile_named, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_build_tile_named, dim3(d_tile_list ? count : l.tiles), dim3(1024), lds, change_stream(c), a);
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// The pod operands every pick's argument struct carries (SelectArgs, BestfitRowsArgs, BestfitListedArgs), with the request's terms
// normalised: no selector columns and no keys unless the selector term is active, the taint term only over a snapshot with taints.
template <class A>
void fill_pod_operands(A &a, const ksched_ctx *c, const EvalRequest &r) {
    const bool sel = r.sel(c->nkeys);
    a.pcpu = r.pcpu;
    a.pmem = r.pmem;
    a.psel = sel ? r.psel : nullptr;
    a.ptol = r.ptol;
    a.binding = r.out_binding;
    a.p = r.p;
    a.n = c->n;
    a.nkeys = sel ? c->nkeys : 0u;
    a.do_fit = r.fit() ? 1u : 0u;
    a.do_taint = r.taint(c->have_taints) ? 1u : 0u;
}

// ---- the best-fit pick: build and launches over the BestfitIndex (sized by bestfit_layout.hpp) ---------------------------------

// One device merge sort (kernels_build.hpp: k_sort_runs, k_merge_pass), as merge_sort_plan.hpp planned it, on the change stream.  The
// plan names every step's buffers; `io` carries the caller's columns and destination arrays (SortInto::kDest), the sets are `sc`'s.
int launch_merge_sort(ksched_ctx *c, const SortPlan &pl, const SortScratch &sc, SortBuffers io) {
    const hipStream_t s = change_stream(c);
    for (int b = 0; b < 2; ++b) {
        io.set_k0[b] = sc.k0[b].ptr;
        io.set_k1[b] = sc.k1[b].ptr;
        io.set_idx[b] = sc.idx[b].ptr;
    }
    for (uint32_t i = 0; i < pl.nsteps; ++i) {
        const SortStep &st = pl.steps[i];
        const SortPtrs ptr = sort_step_ptrs(pl, st, io);
        SortArgs q{};
        q.n = pl.n;
        q.run = st.run;
        q.k0_in = ptr.k0_in;
        q.k1_in = ptr.k1_in;
        q.idx_in = ptr.idx_in;
        q.k0_out = ptr.k0_out;
        q.k1_out = ptr.k1_out;
        q.idx_out = ptr.idx_out;
        if (st.kernel == SortKernel::kRuns) hipLaunchKernelGGL(k_sort_runs, dim3(st.grid), dim3(kSortRun), 0, s, q);
        else hipLaunchKernelGGL(k_merge_pass, dim3(st.grid), dim3(256), 0, s, q);
        HIPCHK(c, hipGetLastError());
    }
    return KSCHED_OK;
}

// one order of the snapshot's n nodes: ascending (k0, k1, node) -- k1 may be null -- from the columns into dst_k0 / dst_idx, the arrays
// the pick kernels read (nobody reads the second key of the final order: it stays in the scratch)
int bestfit_sort(ksched_ctx *c, const int64_t *k0, const int64_t *k1, int64_t *dst_k0, uint32_t *dst_idx) {
    const SortPlan pl = plan_merge_sort(c->n, k1 != nullptr, SortInto::kDest);
    if (pl.refused) {  // (no snapshot of that size fits a GPU's memory anyway)
        c->last_error = "best-fit structures: more than 2^31 nodes";
        return KSCHED_E_INVAL;
    }
    SortBuffers io;
    io.col_k0 = k0;
    io.col_k1 = k1;
    io.dst_k0 = dst_k0;
    io.dst_idx = dst_idx;
    return launch_merge_sort(c, pl, c->bestfit.sort, io);
}

// Best-fit candidate order of the snapshot, ascending (avail_mem, avail_cpu, node), its inverse, the node
// columns in that order, the sorted cpu column with the sample arrays of the two rank searches, and -- when the snapshot has a
// bitmap index -- the named rows once more over best-fit positions plus the 257 cpu threshold rows (k_pick_bestfit_rows).
// Two device merge sorts (bestfit_sort) and two kernels, on the change stream; called lazily by the first PICK_BESTFIT request
// after the snapshot changed (ksched_set_nodes / ksched_update_nodes only mark it stale).
int build_bestfit_rows(ksched_ctx *c);
int build_bestfit(ksched_ctx *c) {
    BestfitIndex &bi = c->bestfit;
    const uint32_t n = c->n;
    bi.rows_built = false;
    hipStream_t s = change_stream(c);
    const BfOrderLayout &o = bi.order = bf_order_layout(n);
    HIPCHK(c, bi.by_cpu.reserve(n));
    HIPCHK(c, bi.cpurank.reserve(n));
    HIPCHK(c, bi.samples.reserve(o.sample_elems()));
    HIPCHK(c, bi.sort.reserve(n, true));
    // order 1: ascending (cpu, node) -> cpu_sorted (the sorted cpu column), by_cpu (node with cpu rank r)
    if (int rc = bestfit_sort(c, c->ncpu.ptr, nullptr, bi.cpu_sorted.ptr, bi.by_cpu.ptr)) return rc;
    // order 2: ascending (mem, cpu, node) -> bf_mem, bf_order
    if (int rc = bestfit_sort(c, c->nmem.ptr, c->ncpu.ptr, bi.bf_mem.ptr, bi.bf_order.ptr)) return rc;
    BfGatherArgs g{};
    g.ncpu = c->ncpu.ptr;
    g.nmem = c->nmem.ptr;
    g.bf_order = bi.bf_order.ptr;
    g.by_cpu = bi.by_cpu.ptr;
    g.bf_rank = bi.bf_rank.ptr;
    g.cpurank = bi.cpurank.ptr;
    g.bf_mem = bi.bf_mem.ptr;
    g.bf_cpu = bi.bf_cpu.ptr;
    g.cpu_sorted = bi.cpu_sorted.ptr;
    g.samples = bi.samples.ptr;
    g.n = n;
    g.n1 = o.n1;
    g.n2 = o.n2;
    hipLaunchKernelGGL(k_bf_gather, dim3((n + 255u) / 256u), dim3(256), 0, s, g);
    HIPCHK(c, hipGetLastError());
    // 8-ary level arrays for the lane-per-pod searches
    HIPCHK(c, bi.levels.reserve(o.level_elems()));
    if (o.nlev) {
        BfLevelsArgs lv{};
        lv.bf_mem = bi.bf_mem.ptr;
        lv.cpu_sorted = bi.cpu_sorted.ptr;
        lv.lvl = bi.levels.ptr;
        lv.n = n;
        lv.nlev = o.nlev;
        lv.lvl_half = o.lvl_half;
        for (uint32_t k = 0; k < kBfMaxLevels; ++k) lv.lvl_off[k] = o.lvl_off[k];
        hipLaunchKernelGGL(k_bf_levels, dim3(((n + 7u) / 8u + 255u) / 256u), dim3(256), 0, s, lv);
        HIPCHK(c, hipGetLastError());
    }
    return build_bestfit_rows(c);
}

// will the best-fit rows exist once ensure_bestfit has run?  (they are built with the bitmap index's row numbering)
inline bool bf_rows_expected(const ksched_ctx *c) { return c->idx.built && c->n > 0; }

// The row bitmaps in best-fit order alone, over the current order: what a label / taint change (ksched_update_node_labels) makes
// stale -- it cannot move the order, which reads `available` only.
int build_bestfit_rows(ksched_ctx *c) {
    BestfitIndex &bi = c->bestfit;
    const uint32_t n = c->n;
    hipStream_t s = change_stream(c);
    bi.rows_built = false;
    if (!bf_rows_expected(c)) return KSCHED_OK;  // (list keys have no rows: pods that constrain one are picked from the key's sorted lists, k_pick_bestfit_listed)
    const IndexedLayout &l = c->idx.lay;
    const BfRowLayout w = bf_row_layout(n, l.row_cpu);
    HIPCHK(c, bi.rows.reserve(w.words()));
    HIPCHK(c, hipMemsetAsync(bi.rows.ptr, 0, w.words() * 8, s));
    BfRowsArgs r{};
    r.nlab = c->nlab.ptr;
    r.ntaint = c->have_taints ? c->ntaint.ptr : nullptr;
    r.bf_order = bi.bf_order.ptr;
    r.cpurank = bi.cpurank.ptr;
    r.lab_meta = c->idx.d_lab_meta;
    r.rows = bi.rows.ptr;
    r.n = n;
    r.Wbf = w.Wbf;
    r.nkeys = c->nkeys;
    r.ngroups = l.ngroups;
    r.row_valid = l.row_valid;
    r.row_taint = l.row_taint;
    r.row_cpu0 = w.row_cpu0;
    r.q = w.q;
    r.levels = w.levels;
    hipLaunchKernelGGL(k_bf_rows, dim3((w.Wbf + 3u) / 4u), dim3(256), 0, s, r);
    HIPCHK(c, hipGetLastError());
    bi.row = w;
    bi.rows_built = true;
    return KSCHED_OK;
}

// a PICK_BESTFIT request is about to be enqueued: make sure the structures match the snapshot
int ensure_bestfit(ksched_ctx *c) {
    BestfitIndex &bi = c->bestfit;
    if (c->n == 0 || !bi.stale()) return KSCHED_OK;
    SnapshotChange chg;
    if (int rc = chg.begin(c)) return rc;  // picks already enqueued read the previous order
    if (int rc = bi.order_stale ? build_bestfit(c) : build_bestfit_rows(c)) {  // (rows only: no sort)
        chg.done = true;  // columns and index are untouched and the stale flags still set: nothing to invalidate, the next request tries again
        return rc;
    }
    bi.order_stale = bi.rows_stale = false;
    return chg.commit(Stale::kNothing);
}

// BestfitRowsArgs as all three kernels over the rows take them: the index's arrays, its layouts and the bitmap index's row numbers,
// and the request.  The hand-over members stay null / 0: the one-stage kernel reads none of them, launch_bestfit_two_stages adds them.
BestfitRowsArgs make_bestfit_rows_args(const ksched_ctx *c, const EvalRequest &r) {
    const BestfitIndex &bi = c->bestfit;
    const IndexedLayout &l = c->idx.lay;
    BestfitRowsArgs q{};
    q.rows = bi.rows.ptr;
    q.lab_meta = c->idx.d_lab_meta;
    q.cpu_sorted = bi.cpu_sorted.ptr;
    q.bf_mem = bi.bf_mem.ptr;
    q.bf_cpu = bi.bf_cpu.ptr;
    q.bf_order = bi.bf_order.ptr;
    if (bi.order.sampled) {
        q.mem_s1 = bi.samples.ptr;
        q.mem_s2 = bi.samples.ptr + bi.order.mem_s2();
        q.cpu_s1 = bi.samples.ptr + bi.order.cpu_s1();
        q.cpu_s2 = bi.samples.ptr + bi.order.cpu_s2();
    }
    fill_pod_operands(q, c, r);
    q.Wbf = bi.row.Wbf;
    q.ngroups = l.ngroups;
    q.row_valid = l.row_valid;
    q.row_zero = l.row_zero;
    q.row_taint = l.row_taint;
    q.row_cpu0 = bi.row.row_cpu0;
    q.q = bi.row.q;
    for (int k = 0; k < 8; ++k) {
        q.lab_base8[k] = l.lab_base[k];
        q.lab_max8[k] = l.lab_max[k];
    }
    return q;
}

// one wave per pod, one wave per block (scans differ tenfold in length: with four waves per block the long ones hold up the
// placement of whole blocks; 158 against 172 us for 125 k pods at the C5 shard)
int launch_bestfit_one_stage(ksched_ctx *c, const EvalRequest &r) {
    const BestfitRowsArgs q = make_bestfit_rows_args(c, r);
    hipLaunchKernelGGL(k_pick_bestfit_rows, dim3(r.p), dim3(64), 0, r.stream, q);
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// KSCHED_OPT_DEBUG bit 20: where the waves of the two best-fit stages spend their time (synchronous; stderr; tools only)
void bestfit_trace_report(ksched_ctx *c, uint32_t p, size_t slots2, hipStream_t s) {
    const size_t waves1 = (p + 63) / 64, total = waves1 * 8 + slots2 * 4;
    std::vector<uint64_t> h(total);
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h.data(), c->bestfit.trace.ptr, total * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    if (const char *path = getenv("KSCHED_BF_TRACE_FILE"))  // the raw stamps: [waves of stage 1][8] then [hand-over slots][4] uint64
        if (FILE *f = fopen(path, "wb")) {
            fwrite(h.data(), 8, total, f);
            fclose(f);
        }
    auto pct = [](std::vector<double> &v, double f) { return v.empty() ? 0.0 : v[(size_t)(f * (double)(v.size() - 1))]; };
    const double ghz = 0.1;  // s_memrealtime: the constant 100 MHz reference clock
    uint64_t t0 = ~0ull;
    for (size_t w = 0; w < waves1; ++w)
        if (h[w * 8]) t0 = std::min(t0, h[w * 8]);
    const char *names[4] = {"operands", "searches", "word trips", "hand-over"};
    std::vector<double> ph[4], entry, exit_, und;
    for (size_t w = 0; w < waves1; ++w) {
        const uint64_t *r = &h[w * 8];
        if (!r[0] || !r[4]) continue;
        for (int i = 0; i < 4; ++i) ph[i].push_back((double)(r[i + 1] - r[i]) / ghz * 1e-3);
        entry.push_back((double)(r[0] - t0) / ghz * 1e-3);
        exit_.push_back((double)(r[4] - t0) / ghz * 1e-3);
        und.push_back((double)r[5]);
    }
    auto line = [&](const char *what, std::vector<double> &v) {
        std::sort(v.begin(), v.end());
        double sum = 0;
        for (double x : v) sum += x;
        fprintf(stderr, "  %-28s mean %7.2f   p10 %7.2f  p50 %7.2f  p90 %7.2f  max %7.2f   (%zu waves)\n", what, v.empty() ? 0.0 : sum / (double)v.size(), pct(v, 0.1), pct(v, 0.5), pct(v, 0.9),
                pct(v, 1.0), v.size());
    };
    fprintf(stderr, "best-fit stage 1 (k_pick_bestfit_lanes), us:\n");
    line("entry after the first wave", entry);
    for (int i = 0; i < 4; ++i) line(names[i], ph[i]);
    line("exit after the first entry", exit_);
    line("lanes handed over per wave", und);
    const uint64_t *t2 = &h[waves1 * 8];
    uint64_t t20 = ~0ull;
    std::vector<double> e2, d2, x2, words;
    for (size_t w = 0; w < slots2; ++w)
        if (t2[w * 4]) t20 = std::min(t20, t2[w * 4]);
    for (size_t w = 0; w < slots2; ++w) {
        const uint64_t *r = &t2[w * 4];
        if (!r[0] || !r[1]) continue;
        e2.push_back((double)(r[0] - t20) / ghz * 1e-3);
        d2.push_back((double)(r[1] - r[0]) / ghz * 1e-3);
        x2.push_back((double)(r[1] - t20) / ghz * 1e-3);
    }
    fprintf(stderr, "best-fit stage 2 (k_pick_bestfit_handed), us:   first entry %.2f us after stage 1's first entry\n", t20 == ~0ull ? 0.0 : (double)(t20 - t0) / ghz * 1e-3);
    line("entry after the first wave", e2);
    line("scan of one pod", d2);
    line("exit after the first entry", x2);
}

// Two stages: one lane per pod decides from the first candidate words (k_pick_bestfit_lanes); the rare rest goes to the wave-per-pod
// kernel through the hand-over buffer (k_pick_bestfit_handed).  `lists`: pods that constrain a list key are split off by the first
// stage into the listed mask, for launch_bestfit_listed.
int launch_bestfit_two_stages(ksched_ctx *c, const EvalRequest &r, bool lists) {
    BestfitIndex &bi = c->bestfit;
    const hipStream_t s = r.stream;
    const IndexedLayout &l = c->idx.lay;
    const BfHandoverLayout h = bf_handover_layout(r.p);
    const BfDebug dbg = bf_debug(c->opt_debug);
    BestfitRowsArgs q = make_bestfit_rows_args(c, r);
    if (int rsc = scratch_enter(c, s)) return rsc;
    HIPCHK(c, bi.handover.reserve(h.total_u32()));
    if (bi.rotation.fresh(bi.handover.cap)) {  // a fresh allocation: all counters once
        HIPCHK(c, hipMemsetAsync(bi.handover.ptr, 0, h.ctr_u32 * 4, s));
        bi.rotation.zeroed(bi.handover.cap);
    }
    uint32_t *const words = bi.handover.ptr;
    q.handover_count = words + h.ctr_off(bi.rotation.use());
    q.zero_next = words + h.ctr_off(bi.rotation.zero());
    q.sub_cap = (uint32_t)h.sub_cap;
    q.lvl = bi.levels.ptr;
    q.nlev = bi.order.nlev;
    q.lvl_half = bi.order.lvl_half;
    for (uint32_t k = 0; k < kBfMaxLevels; ++k) q.lvl_off[k] = bi.order.lvl_off[k];
    q.handover_recs = words + h.rec_off();
    q.nlist = lists ? l.nlist : 0u;
    for (uint32_t j = 0; j < q.nlist; ++j) q.list_col[j] = l.list_col[j];
    q.listed_mask = lists ? reinterpret_cast<uint64_t *>(words + h.mask_off()) : nullptr;
    q.lane_blocks = dbg.lane_blocks;
    if (dbg.tracing) {
        HIPCHK(c, bi.trace.reserve(h.trace_u64()));
        HIPCHK(c, hipMemsetAsync(bi.trace.ptr, 0, h.trace_u64() * 8, s));
        q.trace = bi.trace.ptr;
        q.trace2 = bi.trace.ptr + h.trace1_u64();
    }
    hipLaunchKernelGGL(k_pick_bestfit_lanes, dim3((r.p + 255) / 256), dim3(256), 0, s, q);
    HIPCHK(c, hipGetLastError());
    bi.rotation.advance();  // (only once the kernel that zeroes the next set is on its way)
    BestfitRowsArgs q2 = q;
    q2.sub_count = q.handover_count;
    q2.pod_recs = q.handover_recs;
    hipLaunchKernelGGL(k_pick_bestfit_handed, dim3(bf_handed_grid(h.sub_cap, dbg.grid_shift)), dim3(64), 0, s, q2);
    if (dbg.tracing) bestfit_trace_report(c, r.p, h.slots2(), s);
    return KSCHED_OK;  // (launch_bestfit_rows checks the second stage's launch, with the listed kernel's if one follows)
}

// the pods the first stage split off (they constrain a list key): picked from the key's sorted lists in the bitmap index.
// plan_eval sets kRowsTwoStagesListed only when the selector term is active, so the psel / nkeys the shared fill gives are the
// unconditional r.psel / c->nkeys this kernel has always been given.
void launch_bestfit_listed(ksched_ctx *c, const EvalRequest &r) {
    const BestfitIndex &bi = c->bestfit;
    const IndexedLayout &l = c->idx.lay;
    BestfitListedArgs la{};
    la.lists = c->idx.d_list;
    la.nrec = c->nrec.ptr;
    la.nlab = c->nlab.ptr;
    la.bf_rank = bi.bf_rank.ptr;
    la.bf_order = bi.bf_order.ptr;
    fill_pod_operands(la, c, r);
    la.listed_mask = reinterpret_cast<uint64_t *>(bi.handover.ptr + bf_handover_layout(r.p).mask_off());  // (where the first stage has just written it)
    la.tiles = l.tiles;
    la.nlist = l.nlist;
    for (uint32_t j = 0; j < l.nlist; ++j) la.list_col[j] = l.list_col[j];
    hipLaunchKernelGGL(k_pick_bestfit_listed, dim3((r.p + 3) / 4), dim3(256), 0, r.stream, la);
}

// The best-fit pick from bitmaps kept in best-fit order, no mask involved: one stage, two, or two plus the listed kernel, as the plan says
int launch_bestfit_rows(ksched_ctx *c, const EvalRequest &r, const EvalPlan &plan) {
    if (plan.bestfit == BestfitPick::kRowsOneStage) return launch_bestfit_one_stage(c, r);
    const bool lists = plan.bestfit == BestfitPick::kRowsTwoStagesListed;
    if (int rc = launch_bestfit_two_stages(c, r, lists)) return rc;
    if (lists) launch_bestfit_listed(c, r);
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// ---- the bitmap index's layout: plan -> reserve -> build ----------------------------------------------------------------
// One decision for ksched_set_nodes and for a label update that leaves the planned layout (ksched_update_node_labels): the layout
// (indexed_plan: lab_max, row vs list keys, taint groups) is planned on the host, its buffers reserved and its meta words copied,
// then the index is built from the node columns.
struct IndexPlan {
    IndexedLayout l{};
    const char *why = "";
    bool indexed = false;
    uint32_t meta[72] = {};
};
constexpr size_t kPlanMetaBytes = sizeof(IndexPlan::meta), kPlanMetaWords = kPlanMetaBytes / 4;

// the layout for these per-key maxima and taint bits; they become the ctx's plan inputs
void index_plan(ksched_ctx *c, uint32_t n, uint32_t n_keys, const uint32_t *lab_max, uint64_t all_taints, IndexPlan &p) {
    p.indexed = indexed_plan(p.l, n, n_keys, lab_max, all_taints, &p.why);
    if (p.indexed) indexed_meta(p.l, p.meta);
    for (uint32_t k = 0; k < KSCHED_MAX_KEYS; ++k) c->plan_lab_max[k] = k < n_keys ? lab_max[k] : 0u;
    c->plan_taints = all_taints;
}

// the index's buffers, and the copy of its meta words out of `h_meta` (kPlanMetaBytes of the pinned staging block) on the change stream
int index_reserve(ksched_ctx *c, const IndexPlan &p, uint8_t *h_meta) {
    c->idx.built = false;
    if (!p.indexed) return KSCHED_OK;
    hipError_t e = indexed_reserve(c->idx, p.l);
    if (e != hipSuccess) return fail_hip(c, e, "indexed_reserve");
    memcpy(h_meta, p.meta, kPlanMetaBytes);
    HIPCHK(c, hipMemcpyAsync(c->idx.d_lab_meta, h_meta, kPlanMetaBytes, hipMemcpyHostToDevice, change_stream(c)));
    return KSCHED_OK;
}

// the whole index, by the kernels of kernels_build.hpp from the columns resident on the device -- or, with KSCHED_OPT_INDEX_BUILD = 1
// and the caller's host columns at hand (`host`: ksched_set_nodes), by the host spec; without an index, the reason the fused kernel
// is not applicable
int index_build(ksched_ctx *c, const IndexPlan &p, bool host, const int64_t *cpu, const int64_t *mem, const uint32_t *lab,
                const uint64_t *taints) {
    if (!p.indexed) {
        c->index_reason = p.why;
        return KSCHED_OK;
    }
    c->idx.lay = p.l;
    if (host && c->opt_index_build == 1) {
        hipError_t e = indexed_build_host(c->idx, p.l, cpu, mem, lab, taints, change_stream(c));
        if (e != hipSuccess) return fail_hip(c, e, "indexed_build_host");
    } else {
        if (int rc = launch_build_named(c)) return rc;
        if (int rc = launch_build_lists(c)) return rc;
        if (int rc = launch_build_fit(c, nullptr, 0)) return rc;
    }
    c->idx.built = true;
    c->index_reason.clear();
    return KSCHED_OK;
}

// ---- evaluation dispatch: request -> plan -> launchers ---------------------------------------------------------------
// An EvalRequest (eval_request.hpp) is the batch as an entry point hands it on; plan_eval (eval_plan.hpp) says which kernels it
// runs; the launchers below enqueue them.  eval_on_device strings the three together.

struct DirectPtrs {
    const int64_t *ncpu, *nmem;
    const uint32_t *nlab;
    const uint64_t *ntaint;
    const int64_t *pcpu, *pmem;
    const uint32_t *psel;
    const uint64_t *ptol;
    uint64_t *out_feas, *out_fit;
};

template <bool SEL, bool TAINT>
void launch_direct_t(const DirectPtrs &q, const DirectArgs &a, dim3 grid, bool want_fit, hipStream_t s) {
    if (want_fit)
        hipLaunchKernelGGL((k_eval_direct<SEL, TAINT, true>), grid, dim3(64 * kDirectWaves), 0, s, q.ncpu, q.nmem, q.nlab,
                           q.ntaint, q.pcpu, q.pmem, q.psel, q.ptol, q.out_feas, q.out_fit, a);
    else
        hipLaunchKernelGGL((k_eval_direct<SEL, TAINT, false>), grid, dim3(64 * kDirectWaves), 0, s, q.ncpu, q.nmem, q.nlab,
                           q.ntaint, q.pcpu, q.pmem, q.psel, q.ptol, q.out_feas, q.out_fit, a);
}

// out_feas: where the feasible mask goes (the request's, or the ctx's scratch one)
int run_direct(ksched_ctx *c, const EvalRequest &r, uint64_t *out_feas) {
    const hipStream_t s = r.stream;
    DirectPtrs q{};
    q.ncpu = c->ncpu.ptr;
    q.nmem = c->nmem.ptr;
    q.nlab = c->nlab.ptr;
    q.ntaint = c->have_taints ? c->ntaint.ptr : nullptr;
    q.pcpu = r.pcpu;
    q.pmem = r.pmem;
    q.psel = r.psel;
    q.ptol = r.ptol;
    q.out_feas = out_feas;
    q.out_fit = r.out_fit;
    DirectArgs a{};
    a.n = c->n;
    a.p = r.p;
    a.W = c->W;
    a.pitch = r.pitch;
    a.do_fit = r.fit() ? 1u : 0u;

    const bool sel = r.sel(c->nkeys);
    const bool taint = r.taint_flag();  // (the flag alone: without taints in the snapshot the kernel gets a null taint column)
    const bool want_fit = r.want_fit();

    const uint32_t words_per_block = kDirectCW * kDirectWaves;
    const uint32_t gx = (c->W + words_per_block - 1) / words_per_block;
    const uint32_t pod_tiles = (r.p + 63) / 64;
    // aim for >= ~2048 blocks so all 256 CUs (8 XCDs) stay busy, but keep a block on its node
    // columns for as many pods as possible (node registers are loaded once per block)
    uint32_t gy = std::max(1u, std::min(pod_tiles, (2048u + gx - 1) / gx));
    a.pod_tiles_per_block = (pod_tiles + gy - 1) / gy;
    gy = (pod_tiles + a.pod_tiles_per_block - 1) / a.pod_tiles_per_block;
    dim3 grid(gx, gy);

    // first pass: fit + taints + keys [0, 8)
    a.key0 = 0;
    a.nkeys = sel ? std::min(c->nkeys, (uint32_t)kDirectKeys) : 0;
    a.accumulate = 0;
    // (the fit term is a kernel argument here, not an instantiation.  The two terms go in negated: the instantiations are then first named
    // <true, true> ... <false, false>, the order in which the code object has always carried these kernels -- tools/same_device_code.py)
    with_predicates(false, !sel, !taint, [&](auto, auto NS, auto NT) { launch_direct_t<!decltype(NS)::value, !decltype(NT)::value>(q, a, grid, want_fit, s); });
    // further passes: 8 more keys each, ANDed into the feasible mask
    if (sel && out_feas) {
        for (uint32_t k0 = kDirectKeys; k0 < c->nkeys; k0 += kDirectKeys) {
            DirectArgs b = a;
            b.key0 = k0;
            b.nkeys = std::min(c->nkeys - k0, (uint32_t)kDirectKeys);
            b.accumulate = 1;
            b.do_fit = 0;
            DirectPtrs r2 = q;
            r2.out_fit = nullptr;
            r2.ptol = nullptr;
            launch_direct_t<true, false>(r2, b, grid, false, s);
        }
    }
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// the pick of select_node_for_pod (src/main.rs:51-71) / the best-fit extension, from a feasibility mask on the device
// (`feas`, rows r.pitch words apart; of the request: p, pmem, samples, attempts, flags, out_binding, stream)
int launch_pick(ksched_ctx *c, const EvalRequest &r, const uint64_t *feas) {
    const hipStream_t s = r.stream;
    if ((r.flags & KSCHED_PICK_BESTFIT) && c->n > 0)
        if (int rcb = ensure_bestfit(c)) return rcb;
    if (int rce = stream_enter(c, s)) return rce;
    if (r.flags & KSCHED_PICK_SAMPLED) {
        hipLaunchKernelGGL(k_pick_sampled, dim3((r.p + 255) / 256), dim3(256), 0, s, feas, r.samples, r.out_binding, r.p, c->n,
                           r.pitch, r.attempts);
    } else if (r.flags & KSCHED_PICK_BESTFIT) {
        const BestfitIndex &bi = c->bestfit;  // (the order and its inverse: no rows)
        hipLaunchKernelGGL(k_pick_bestfit, dim3((r.p + 3) / 4), dim3(256), 0, s, feas, bi.bf_order.ptr, bi.bf_rank.ptr, bi.bf_mem.ptr, r.pmem,
                           r.out_binding, r.p, c->n, c->W, r.pitch, r.fit() ? 1u : 0u);
    } else if (const RankedMember *m = ranked_member(r.flags)) {  // (every caller has c->n > 0 here: an empty snapshot's bindings are a memset)
        if (m->pick == RankedPick::kUniform) {
            hipLaunchKernelGGL(k_pick_uniform, dim3((r.p + kUniformWaves - 1) / kUniformWaves), dim3(64 * kUniformWaves), 0, s, feas, r.samples,
                               r.out_binding, r.p, c->n, c->W, r.pitch, r.attempts);
        } else {
            // the members that read the available columns, one launch shape (the stream_enter above puts the columns behind the latest
            // snapshot change; no best-fit order involved).  Two kernels on purpose: kernels_pick_pack.hpp.
            static_assert(kSpreadWaves == kPackWaves, "k_pick_spread and k_pick_pack are launched with one geometry");
            const auto kernel = m->pick == RankedPick::kSpread ? k_pick_spread : k_pick_pack;
            hipLaunchKernelGGL(kernel, dim3((r.p + kSpreadWaves - 1) / kSpreadWaves), dim3(64 * kSpreadWaves), 0, s, feas, r.samples,
                               (const int64_t *)c->nmem.ptr, (const int64_t *)c->ncpu.ptr, r.out_binding, r.p, c->n, c->W, r.pitch, r.attempts);
        }
    }
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// launch_pick for a caller that has not looked at the snapshot: no pods, nothing; no nodes, every binding -1 (choose() on an empty
// store yields None on every attempt, src/main.rs:56,70)
int pick_from_mask(ksched_ctx *c, const EvalRequest &r, const uint64_t *feas) {
    if (r.p == 0) return KSCHED_OK;
    if (c->n > 0) return launch_pick(c, r, feas);
    HIPCHK(c, hipMemsetAsync(r.out_binding, 0xFF, (size_t)r.p * sizeof(int32_t), r.stream));
    return KSCHED_OK;
}

SelectArgs make_select_args(const ksched_ctx *c, const EvalRequest &r) {
    SelectArgs q{};
    q.nrec = c->nrec.ptr;
    q.nlab = c->nlab.ptr;
    fill_pod_operands(q, c, r);
    q.samples = r.samples;
    q.attempts = r.attempts;
    return q;
}

// select_node_for_pod the reference's way: only the sampled candidates are tested, from the columns (k_select_sampled)
int launch_select(ksched_ctx *c, const EvalRequest &r) {
    const hipStream_t s = r.stream;
    const SelectArgs q = make_select_args(c, r);
    const dim3 grid((r.p + 255) / 256), block(256);  // (64- and 128-thread blocks measured slower: 6.6 / 6.5 us against 5.7 at C3)
    if (r.attempts <= 5) {
        switch ((c->opt_debug >> 8) & 3u) {  // KSCHED_OPT_DEBUG bits 8-9: A/B of the number of eagerly fetched draws (tools/)
            case 1: hipLaunchKernelGGL((k_select_sampled<5, 3>), grid, block, 0, s, q); break;
            case 2: hipLaunchKernelGGL((k_select_sampled<5, 5>), grid, block, 0, s, q); break;
            case 3: hipLaunchKernelGGL((k_select_sampled<5, 2>), grid, block, 0, s, q); break;
            default: hipLaunchKernelGGL((k_select_sampled<5, 1>), grid, block, 0, s, q);  // rocprofv3 at C3, in the step: 1 eager draw 5.79 us, 2: 6.08, 3: 6.78, 5: 7.25
        }
    }
    else hipLaunchKernelGGL((k_select_sampled<8, 2>), grid, block, 0, s, q);
    HIPCHK(c, hipGetLastError());
    return KSCHED_OK;
}

// the accumulators of the tile-test pick for launches on `s` (StreamRes::pick_acc): one buffer per stream, all zero between launches
int pick_acc_for(ksched_ctx *c, uint32_t p, hipStream_t s, uint64_t **out) {
    StreamRes *sr = c->order.res(s);
    if (!sr) {  // (every evaluation goes through stream_enter first)
        c->last_error = "the tile-test pick's stream has not been entered";
        return KSCHED_E_STATE;
    }
    DevBuf<uint64_t> &buf = sr->pick_acc;
    const size_t units = ((size_t)p + 7) / 8 + 8;  // one word per unit of eight pods (+ slack: the lanes past a batch's last unit compute an address, never use it)
    if (buf.cap < units) {  // (re)allocated: zero once; from then on the kernel leaves every word it used at zero
        HIPCHK(c, buf.reserve(units));
        HIPCHK(c, hipMemsetAsync(buf.ptr, 0, units * 8, s));
    }
    *out = buf.ptr;
    return KSCHED_OK;
}

// One launch in every opt_timing carries a pair of events from the pool (ksched_kernel_time_ms).  on_stream: the pair brackets the
// launches on the stream; otherwise the kernel carries it on its dispatch packet itself (run_fused: hipExtLaunchKernel).
struct TimingBracket {
    hipEvent_t a = nullptr, b = nullptr;  // null: this launch is not timed
    bool on_stream = false;
};

int timing_begin(ksched_ctx *c, hipStream_t s, bool on_stream, TimingBracket &t) {
    // (at most 65536 unread samples: a caller that switches timing on and never reads it does not grow the event pool for ever)
    const bool timed = c->opt_timing && c->ev_used < 65536u && (c->timing_seq++ % c->opt_timing) == 0;
    if (!timed) return KSCHED_OK;
    size_t slot = 0;
    if (int trc = timing_slot(c, &slot)) return trc;
    t.a = c->ev_pool[slot].a;
    t.b = c->ev_pool[slot].b;
    t.on_stream = on_stream;
    if (on_stream) HIPCHK(c, hipEventRecord(t.a, s));
    return KSCHED_OK;
}

int timing_end(ksched_ctx *c, hipStream_t s, const TimingBracket &t) {
    if (t.b && t.on_stream) HIPCHK(c, hipEventRecord(t.b, s));
    return KSCHED_OK;
}

// KSCHED_OPT_KERNEL forces the fused kernel where it does not apply (evaluations and summaries alike)
int fail_fused_not_applicable(ksched_ctx *c) {
    c->last_error = "fused kernel not applicable to this snapshot/request: " + (c->index_reason.empty() ? std::string("the bitmap index does not fit LDS") : c->index_reason);
    return KSCHED_E_UNSUPPORTED;
}

// the mask kernel of the plan -- with the riding pick, if one rides --, the combine of a combining call, and the pick that reads the mask, if one does
int launch_mask(ksched_ctx *c, const EvalRequest &r, const EvalPlan &plan) {
    const hipStream_t s = r.stream;
    const bool fused = plan.mask == MaskKernel::kFused;
    FusedOptions o;
    SelectArgs ride{};
    if (plan.pick_rides()) {
        ride = make_select_args(c, r);
        o.pick = &ride;
        if (plan.sampled == SampledPick::kRidesTiles) {
            o.pick_form = 2;
            if (int rc = pick_acc_for(c, r.p, s, &o.pick_acc)) return rc;
        }
    }
    uint64_t *feas = r.out_feas;
    if (plan.scratch_mask) {
        if (int rsc = scratch_enter(c, s)) return rsc;
        HIPCHK(c, c->scratch_mask.reserve((size_t)r.p * r.pitch));
        feas = c->scratch_mask.ptr;
    }
    // (the fused kernel carries its timing events on the dispatch packet itself -- hipExtLaunchKernel --, the multi-launch
    // paths are bracketed by stream events)
    TimingBracket t;
    if (int trc = timing_begin(c, s, !fused, t)) return trc;
    if (fused) {
        constexpr uint32_t kTraceBlocks = 8192;
        if (c->opt_trace) {
            DeviceGuard g2(c->device);
            if (int rsc = scratch_enter(c, s)) return rsc;
            HIPCHK(c, c->trace.reserve((size_t)kTraceBlocks * KSCHED_TRACE_WORDS));
            HIPCHK(c, hipMemsetAsync(c->trace.ptr, 0, (size_t)kTraceBlocks * KSCHED_TRACE_WORDS * 8, s));
            o.trace = c->trace.ptr;
            o.trace_blocks = kTraceBlocks;
        }
        o.debug = c->opt_debug;
        o.ev_start = t.a;
        o.ev_stop = t.b;
        o.grid_cus = c->opt_grid_cus;
        o.round_order = c->opt_round_order;
        hipError_t e = run_fused(c->idx, r, feas, o);
        if (e != hipSuccess) return fail_hip(c, e, "run_fused");
    } else if (plan.mask == MaskKernel::kSelOp || plan.mask == MaskKernel::kSelTag || plan.mask == MaskKernel::kSelTerms) {
        // (extensions E8, E9, E10: the selector term alone, from the label columns -- under the plan's operator, the operator read out of every
        // entry, or the OR over the plan's term count of such terms, entries [terms][nkeys][p])
        if (hipError_t e = run_selector_mask(plan.mask, plan.selop, plan.terms, c->nlab.ptr, r.sel(c->nkeys) ? r.psel : nullptr, feas, r.p, c->n, c->W, r.pitch, c->nkeys, s); e != hipSuccess)
            return fail_hip(c, e, plan.mask == MaskKernel::kSelOp ? "run_selop" : plan.mask == MaskKernel::kSelTag ? "run_seltag" : "run_selterms");
    } else if (int rc = run_direct(c, r, feas)) {
        return rc;
    }
    c->last_kernel = plan.last_kernel;
    if (int trc = timing_end(c, s, t)) return trc;
    if (plan.combine == CombineOp::kNone) return plan.pick_from_mask() ? launch_pick(c, r, feas) : KSCHED_OK;
    // a combining call: the scratch mask holds feasible(this call); fold it into the caller's mask, then pick from that mask alone -- the
    // pick is told nothing about the predicates (best fit must not skip candidates by req_mem: under OR and AND-NOT the combined mask
    // need not include the fit)
    // (KSCHED_COMBINE_SOFT, extension E7: the same fold, dropped for the rows it would empty)
    if (plan.soft) {
        if (hipError_t e = run_mask_combine_soft(plan.combine, r.out_feas, feas, r.p, c->n, c->W, r.pitch, s); e != hipSuccess) return fail_hip(c, e, "run_mask_combine_soft");
    } else if (hipError_t e = run_mask_combine(plan.combine, r.out_feas, feas, r.p, c->n, c->W, r.pitch, s); e != hipSuccess) {
        return fail_hip(c, e, "run_mask_combine");
    }
    if (!plan.pick_from_mask()) return KSCHED_OK;
    EvalRequest pick = r;
    pick.flags = r.flags & KSCHED_PICK_ANY;
    return launch_pick(c, pick, r.out_feas);
}

// what plan_eval decides by, read off the ctx and the request
EvalFacts eval_facts(const ksched_ctx *c, const EvalRequest &r) {
    EvalFacts f;
    f.p = r.p;
    f.n = c->n;
    f.attempts = r.attempts;
    f.flags = r.flags;
    f.nkeys = c->nkeys;
    f.have_feas = r.out_feas != nullptr;
    f.have_fit = r.out_fit != nullptr;
    f.have_psel = r.psel != nullptr;
    f.tiles = c->idx.lay.tiles;
    f.nlist = c->idx.lay.nlist;
    const TileTerms t = tile_terms(r, c->idx.lay);
    f.fused_applicable = fused_applicable(c->idx, t);
    f.fused_pick_applicable = fused_pick_applicable(c->idx, t, r.p);
    f.fused_tile_pick_applicable = fused_tile_pick_applicable(c->idx.lay, t, r.attempts);
    f.bf_rows_built = c->bestfit.rows_built;
    f.fused_waves = kFusedWaves;
    f.opt_kernel = c->opt_kernel;
    f.opt_fused_pick = c->opt_fused_pick;
    f.opt_bestfit_stages = c->opt_bestfit_stages;
    f.opt_pick_from_mask = c->opt_pick_from_mask;
    f.opt_grid_cus = c->opt_grid_cus;
    f.debug = c->opt_debug;
    f.combine = combine_op(r.flags);
    f.soft = combine_soft(r.flags);
    f.selop = sel_op(r.flags);
    f.seltag = sel_tagged(r.flags);
    f.terms = sel_terms(r.flags);
    return f;
}

int fail_plan(ksched_ctx *c, const EvalPlan &plan) {
    switch (plan.why) {
        case PlanError::kTilePickNotApplicable:
            c->last_error = "the tile-test pick is not applicable to this request (attempts != 5, taints, more than eight label keys, or no room in LDS)";
            break;
        case PlanError::kListKeysTooManyNodes:
            c->last_error = "best fit over a snapshot with list keys supports at most " + std::to_string(kBfLanesMaxNodes) + " nodes";
            break;
        default: return fail_fused_not_applicable(c);
    }
    return plan.error;
}

int eval_on_device(ksched_ctx *c, const EvalRequest &r) {
    const bool pick_b = r.flags & KSCHED_PICK_BESTFIT;
    if (r.p == 0) return KSCHED_OK;
    if (pick_b && c->n > 0)
        if (int rcb = ensure_bestfit(c)) return rcb;  // lazily (re)built after a snapshot change, on the change stream
    if (int rce = stream_enter(c, r.stream)) return rce;  // the stream waits for the latest snapshot change; remembered for the next one
    if (c->n == 0) {
        // no nodes: empty mask rows, no binding possible (reference: choose() on an empty store
        // yields None on every attempt, src/main.rs:56,70)
        if ((r.flags & KSCHED_PICK_ANY) && r.out_binding) HIPCHK(c, hipMemsetAsync(r.out_binding, 0xFF, (size_t)r.p * sizeof(int32_t), r.stream));
        return KSCHED_OK;
    }
    fault_point(c);
    const EvalPlan plan = plan_eval(eval_facts(c, r));
    if (plan.error) return fail_plan(c, plan);  // (nothing has been enqueued)
    c->last_pick = plan.last_pick;
    if (plan.sampled == SampledPick::kOwnLaunch)  // first: nothing waits on a mask kernel
        if (int rc = launch_select(c, r)) return rc;
    if (plan.bestfit_rows())
        if (int rc = launch_bestfit_rows(c, r, plan)) return rc;
    if (plan.mask != MaskKernel::kNone) return launch_mask(c, r, plan);
    return KSCHED_OK;
}

// ---- host staging ------------------------------------------------------------------------------------------------
// The operands of a host batch that a host-pointer entry point uploads into the ctx's pcpu / pmem / psel / ptol / psamples
// buffers: the caller states which by leaving the others null.
struct HostBatch {
    const int64_t *pcpu = nullptr, *pmem = nullptr;
    const uint32_t *psel = nullptr;  // [n_keys][sel_stride], of which the first p entries of every column are the batch's
    uint32_t sel_stride = 0;
    uint32_t terms = 0;  // not 0 (extension E10): [terms][n_keys][sel_stride], selterms_columns columns in all
    const uint64_t *ptol = nullptr;
    const uint32_t *samples = nullptr;  // [p][attempts]
    uint32_t attempts = 0;
};

int stage_batch(ksched_ctx *c, uint32_t p, const HostBatch &h, hipStream_t s) {
    if (h.pcpu) {
        HIPCHK(c, c->pcpu.reserve(p));
        HIPCHK(c, hipMemcpyAsync(c->pcpu.ptr, h.pcpu, (size_t)p * 8, hipMemcpyHostToDevice, s));
    }
    if (h.pmem) {
        HIPCHK(c, c->pmem.reserve(p));
        HIPCHK(c, hipMemcpyAsync(c->pmem.ptr, h.pmem, (size_t)p * 8, hipMemcpyHostToDevice, s));
    }
    if (h.psel) {
        const size_t cols = selterms_columns(h.terms, c->nkeys);  // (n_keys without a term count)
        HIPCHK(c, c->psel.reserve((size_t)p * cols));
        if (h.sel_stride == p)
            HIPCHK(c, hipMemcpyAsync(c->psel.ptr, h.psel, (size_t)p * cols * 4, hipMemcpyHostToDevice, s));
        else  // rows [lo, lo + p) of a [n_keys][sel_stride] array: column k of the shard starts sel_stride entries after column k - 1's
            HIPCHK(c, hipMemcpy2DAsync(c->psel.ptr, (size_t)p * 4, h.psel, (size_t)h.sel_stride * 4, (size_t)p * 4, cols, hipMemcpyHostToDevice, s));
    }
    if (h.ptol) {
        HIPCHK(c, c->ptol.reserve(p));
        HIPCHK(c, hipMemcpyAsync(c->ptol.ptr, h.ptol, (size_t)p * 8, hipMemcpyHostToDevice, s));
    }
    if (h.samples) {
        HIPCHK(c, c->psamples.reserve((size_t)p * h.attempts));
        HIPCHK(c, hipMemcpyAsync(c->psamples.ptr, h.samples, (size_t)p * h.attempts * 4, hipMemcpyHostToDevice, s));
    }
    return KSCHED_OK;
}

// the pick flags (KSCHED_PICK_ANY): at most one per call.  KSCHED_PICK_DRAWS are the picks that read `samples`: node indices (sampled),
// 32-bit draws (uniform: entry 0 of every row; spread and pack: all `attempts` of them)
inline bool at_most_one_pick(uint32_t flags) {
    const uint32_t pick = flags & KSCHED_PICK_ANY;
    return (pick & (pick - 1u)) == 0;
}

// the arguments of an evaluation call: the scalars, and which pointers are null (host or device pointers alike: none is followed).
// combine_accepted: the entry point takes the KSCHED_COMBINE_* flags (the two device-pointer evaluations; mask_combine.hpp and
// mask_combine_soft.hpp have the rules).  selop_accepted: it takes the KSCHED_SELOP_* flags (every evaluation but ksched_pipe_submit;
// sel_ops.hpp has the rules) and, with them, KSCHED_SELOP_TAGGED (sel_tags.hpp has the rules) and its term count (sel_terms.hpp)
int check_eval_args(const EvalRequest &r, bool combine_accepted = false, bool selop_accepted = true) {
    const uint32_t flags = r.flags;
    const uint32_t known = KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT | KSCHED_PICK_ANY | KSCHED_WANT_FIT_MASK | KSCHED_COMBINE_ANY | KSCHED_COMBINE_SOFT | KSCHED_SELOP_ANY |
                           KSCHED_SELOP_TAGGED | KSCHED_SEL_TERMS_MASK;
    if (flags & ~known) return KSCHED_E_INVAL;
    if (int rcc = check_soft_args(flags, combine_accepted, r.out_feas != nullptr, r.out_fit != nullptr)) return rcc;
    if (int rco = check_selop_args(flags, selop_accepted, r.out_fit != nullptr)) return rco;
    if (int rct = check_seltag_args(flags, selop_accepted, r.out_fit != nullptr)) return rct;
    if (int rcm = check_selterms_args(flags, selop_accepted, r.out_fit != nullptr)) return rcm;
    if (!at_most_one_pick(flags)) return KSCHED_E_INVAL;
    if (r.p > 0 && (!r.pcpu || !r.pmem)) return KSCHED_E_INVAL;
    if (flags & KSCHED_PICK_DRAWS) {
        if (!r.out_binding || r.attempts == 0 || r.attempts > KSCHED_MAX_ATTEMPTS) return KSCHED_E_INVAL;
        if (r.p > 0 && !r.samples) return KSCHED_E_INVAL;
    }
    if ((flags & KSCHED_PICK_BESTFIT) && !r.out_binding) return KSCHED_E_INVAL;
    if ((flags & KSCHED_WANT_FIT_MASK) && !r.out_fit) return KSCHED_E_INVAL;
    if (!(flags & KSCHED_WANT_FIT_MASK) && r.out_fit) return KSCHED_E_INVAL;
    if (!(flags & KSCHED_PICK_ANY) && !r.out_feas && !r.out_fit) return KSCHED_E_INVAL;
    return KSCHED_OK;
}

// the arguments of a pick from the caller's masks (ksched_pick, ksched_pick_device) over a snapshot of n nodes
int check_pick_args(uint32_t n, uint32_t p, const uint64_t *feasible, const int64_t *req_mem_bytes, const uint32_t *samples, uint32_t attempts,
                    uint32_t flags, const int32_t *out_binding) {
    if (!(flags & KSCHED_PICK_ANY) || !at_most_one_pick(flags) || (flags & ~(KSCHED_PICK_ANY | KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT))) return KSCHED_E_INVAL;
    if (!out_binding || (p > 0 && n > 0 && !feasible)) return KSCHED_E_INVAL;
    if ((flags & KSCHED_PICK_DRAWS) && (attempts == 0 || attempts > KSCHED_MAX_ATTEMPTS || (p > 0 && !samples))) return KSCHED_E_INVAL;
    if ((flags & KSCHED_PICK_BESTFIT) && (flags & KSCHED_FIT) && p > 0 && !req_mem_bytes) return KSCHED_E_INVAL;
    return KSCHED_OK;
}

}  // namespace

extern "C" {

uint32_t ksched_abi_version(void) { return KSCHED_ABI_VERSION; }

int ksched_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

uint32_t ksched_mask_words(uint32_t n_nodes) { return (uint32_t)(((uint64_t)n_nodes + 63u) / 64u); }

const char *ksched_strerror(int code) {
    switch (code) {
        case KSCHED_OK: return "ok";
        case KSCHED_E_INVAL: return "invalid argument";
        case KSCHED_E_NODEVICE: return "no HIP device (this library has no CPU fallback)";
        case KSCHED_E_HIP: return "HIP runtime error";
        case KSCHED_E_NOMEM: return "out of memory";
        case KSCHED_E_STATE: return "ksched_set_nodes has not been called";
        case KSCHED_E_UNSUPPORTED: return "unsupported request";
        case KSCHED_E_RCCL: return "RCCL error (see ksched_comm_last_error)";
        default: return "unknown error";
    }
}

int ksched_create(ksched_ctx **out, int device_id) try {
    if (!out) return KSCHED_E_INVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return KSCHED_E_NODEVICE;
    if (device_id < 0 || device_id >= count) return KSCHED_E_INVAL;
    ksched_ctx *c = new (std::nothrow) ksched_ctx();
    if (!c) return KSCHED_E_NOMEM;
    c->device = device_id;
    DeviceGuard g(device_id);
    if (!g.ok || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_build, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_stage, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_scratch, hipEventDisableTiming) != hipSuccess) {
        if (c->ev_build) (void)hipEventDestroy(c->ev_build);
        if (c->ev_stage) (void)hipEventDestroy(c->ev_stage);
        if (c->stream) (void)hipStreamDestroy(c->stream);
        delete c;
        return KSCHED_E_HIP;
    }
    c->order.set_own_stream(c->stream);
    *out = c;
    return KSCHED_OK;
} KSCHED_ABI_CATCH(nullptr)

void ksched_destroy(ksched_ctx *c) try {
    if (!c) return;
    {
        DeviceGuard g(c->device);
        (void)hipDeviceSynchronize();
        if (c->h_stage) (void)hipHostFree(c->h_stage);
        for (size_t i = 0; i < c->order.callers(); ++i) (void)hipEventDestroy(c->order.caller_res(i).ev);
        if (c->ev_build) (void)hipEventDestroy(c->ev_build);
        if (c->ev_stage) (void)hipEventDestroy(c->ev_stage);
        if (c->ev_scratch) (void)hipEventDestroy(c->ev_scratch);
        if (c->apply.ev) (void)hipEventDestroy(c->apply.ev);
        indexed_release(c->idx);
        {  // masks the caller never handed back (ksched_mask_alloc)
            MaskRegistry &reg = mask_registry();
            std::lock_guard<std::mutex> rl(reg.mu);
            for (size_t i = reg.live.size(); i-- > 0;)
                if (reg.live[i].owner == c) {
                    (void)mask_release(reg.live[i]);
                    reg.live.erase(reg.live.begin() + (long)i);
                }
        }
        for (auto &ep : c->ev_pool) {
            (void)hipEventDestroy(ep.a);
            (void)hipEventDestroy(ep.b);
        }
        if (c->stream) (void)hipStreamDestroy(c->stream);
        delete c;  // every device buffer goes with its owner, while the ctx's device is still the current one
    }
} catch (...) {  // nothing unwinds across the C ABI
}

const char *ksched_last_error(const ksched_ctx *c) { return c ? c->last_error.c_str() : ""; }
uint32_t ksched_num_nodes(const ksched_ctx *c) { return (c && c->have_nodes) ? c->n : 0; }
uint32_t ksched_num_keys(const ksched_ctx *c) { return (c && c->have_nodes) ? c->nkeys : 0; }
const char *ksched_last_kernel(const ksched_ctx *c) { return c ? c->last_kernel : "none"; }
const char *ksched_last_pick(const ksched_ctx *c) { return c ? c->last_pick : "none"; }

int ksched_set_option(ksched_ctx *c, int option, int64_t value) try {
    if (!c) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    switch (option) {
        case KSCHED_OPT_KERNEL:
            if (value != KSCHED_KERNEL_AUTO && value != KSCHED_KERNEL_DIRECT && value != KSCHED_KERNEL_FUSED) return KSCHED_E_INVAL;
            c->opt_kernel = (int)value;
            return KSCHED_OK;
        case KSCHED_OPT_TIMING:
            if (value < 0 || value > 1000000) return KSCHED_E_INVAL;
            c->opt_timing = (uint32_t)value;
            c->timing_seq = 0;
            return KSCHED_OK;
        case KSCHED_OPT_DEBUG:
            c->opt_debug = (uint32_t)value;
            return KSCHED_OK;
        case KSCHED_OPT_TRACE:
            c->opt_trace = value != 0;
            return KSCHED_OK;
        case KSCHED_OPT_PICK_FROM_MASK:
            c->opt_pick_from_mask = value != 0;
            return KSCHED_OK;
        case KSCHED_OPT_BESTFIT_STAGES:
            if (value < 0 || value > 2) return KSCHED_E_INVAL;
            c->opt_bestfit_stages = (int)value;
            return KSCHED_OK;
        case KSCHED_OPT_INDEX_BUILD:
            if (value != 0 && value != 1) return KSCHED_E_INVAL;
            c->opt_index_build = (int)value;
            return KSCHED_OK;
        case KSCHED_OPT_SNAPSHOT_STREAM:
            if (value != 0 && value != 1) return KSCHED_E_INVAL;
            c->order.set_opt_own_stream(value == 1);
            return KSCHED_OK;
        case KSCHED_OPT_FUSED_PICK:
            if (value < 0 || value > 3) return KSCHED_E_INVAL;
            c->opt_fused_pick = (int)value;
            return KSCHED_OK;
        case KSCHED_OPT_PIPE_MODE:
            if (value < 0 || value > (int64_t)KSCHED_PIPE_MAX_STREAMS) return KSCHED_E_INVAL;
            c->opt_pipe_mode = (int)value;
            return KSCHED_OK;
        case KSCHED_OPT_GRID_CUS:
            if (value != 0 && (value < 8 || value > 256)) return KSCHED_E_INVAL;
            c->opt_grid_cus = (uint32_t)value;
            return KSCHED_OK;
        case KSCHED_OPT_ROUND_ORDER:
            if (value < 0 || value > 2) return KSCHED_E_INVAL;
            c->opt_round_order = (int)value;
            return KSCHED_OK;
        case KSCHED_OPT_MASK_PROBE:
            if (value < 1 || value > 16) return KSCHED_E_INVAL;
            c->opt_mask_probe = (uint32_t)value;
            return KSCHED_OK;
        case KSCHED_OPT_FAULT:  // low byte: 0 off, 1 std::bad_alloc, 2 std::runtime_error; bits 8..: fault points to pass first
            if (ksched_test_hooks_enabled == nullptr) {  // the shipped library: no fault injection (tests/cpp/test_hooks.cpp is not linked in)
                c->last_error = "KSCHED_OPT_FAULT exists in the test build of the library only";
                return KSCHED_E_UNSUPPORTED;
            }
            if (value < 0 || (value & 0xFF) > 2 || value > 0xFFFFFF) return KSCHED_E_INVAL;
            c->fault_kind = (uint32_t)(value & 0xFF);
            c->fault_skip = (uint32_t)(value >> 8);
            return KSCHED_OK;

        default:
            return KSCHED_E_INVAL;
    }
} KSCHED_ABI_CATCH(c)

int ksched_forget_stream(ksched_ctx *c, void *hip_stream) try {
    if (!c) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    stream_forget(c, (hipStream_t)hip_stream);
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_set_nodes(ksched_ctx *c, uint32_t n, const int64_t *cpu, const int64_t *mem, const uint32_t *lab,
                     uint32_t n_keys, const uint64_t *taints) try {
    if (!c) return KSCHED_E_INVAL;
    if (n > 0 && (!cpu || !mem)) return KSCHED_E_INVAL;
    if (n_keys > KSCHED_MAX_KEYS) return KSCHED_E_INVAL;
    if (n_keys > 0 && n > 0 && !lab) return KSCHED_E_INVAL;
    // one pass over the label columns: the largest id per key (the index layout needs it) doubles as the validity check
    uint32_t lab_max[KSCHED_MAX_KEYS] = {};
    for (uint32_t k = 0; k < n_keys; ++k) {
        uint32_t mx = 0;
        const uint32_t *col = lab + (size_t)k * n;
        for (uint32_t i = 0; i < n; ++i) mx = std::max(mx, col[i]);
        if (mx == KSCHED_SEL_NEVER) return KSCHED_E_INVAL;
        lab_max[k] = mx;
    }
    uint64_t all_taints = 0;
    if (taints)
        for (uint32_t i = 0; i < n; ++i) all_taints |= taints[i];
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    SnapshotChange chg{c};  // armed before the fault point: if anything below fails (or throws), a half-built snapshot is never evaluated
    fault_point(c);
    if (int rc = chg.begin(c)) return rc;
    c->n = n;
    c->nkeys = n_keys;
    c->W = ksched_mask_words(n);
    c->have_taints = taints != nullptr;
    HIPCHK(c, c->ncpu.reserve(n));
    HIPCHK(c, c->nmem.reserve(n));
    HIPCHK(c, c->nrec.reserve((size_t)n * kNodeRecWords));
    HIPCHK(c, c->nlab.reserve((size_t)n * n_keys));
    HIPCHK(c, c->ntaint.reserve(n));
    HIPCHK(c, c->bestfit.reserve_for(n));
    hipStream_t s = change_stream(c);  // (snapshot_begin chose it)
    // the per-tile bitmap index: layout on the host (it fixes kernel arguments and LDS sizes), contents on the device
    IndexPlan plan;
    index_plan(c, n, n_keys, lab_max, all_taints, plan);
    // the caller's arrays (and the index's meta words) -> pinned staging -> asynchronous copies on the chosen stream; nothing is
    // copied from pageable or stack memory, so the call never waits for work already queued on that stream
    StageLayout f;  // [cpu][mem][ids n_keys x n][taints][meta words]: each column is copied to its own device buffer
    const size_t o_cpu = f.add<int64_t>(n), o_mem = f.add<int64_t>(n), o_lab = f.add<uint32_t>((size_t)n * n_keys);
    const size_t o_taint = f.add<uint64_t>(taints ? n : 0), o_meta = f.add<uint32_t>(plan.indexed ? kPlanMetaWords : 0);
    uint8_t *h = nullptr;
    if (int rc = f.total ? chg.stage(f.total, 0, &h) : KSCHED_OK) return rc;
    if (n > 0) {
        const size_t b_col = (size_t)n * 8, b_lab = (size_t)n * n_keys * 4;
        memcpy(h + o_cpu, cpu, b_col);
        memcpy(h + o_mem, mem, b_col);
        if (b_lab) memcpy(h + o_lab, lab, b_lab);
        if (taints) memcpy(h + o_taint, taints, b_col);
        HIPCHK(c, hipMemcpyAsync(c->ncpu.ptr, h + o_cpu, b_col, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->nmem.ptr, h + o_mem, b_col, hipMemcpyHostToDevice, s));
        if (b_lab) HIPCHK(c, hipMemcpyAsync(c->nlab.ptr, h + o_lab, b_lab, hipMemcpyHostToDevice, s));
        if (taints) HIPCHK(c, hipMemcpyAsync(c->ntaint.ptr, h + o_taint, b_col, hipMemcpyHostToDevice, s));
    }
    if (int rc = index_reserve(c, plan, h + o_meta)) return rc;
    if (int rc = h ? chg.upload(0) : KSCHED_OK) return rc;  // (the copies above were the block's)
    if (n > 0) {
        hipLaunchKernelGGL(k_build_nrec, dim3((n + 255u) / 256u), dim3(256), 0, s, (const int64_t *)c->ncpu.ptr, (const int64_t *)c->nmem.ptr,
                           taints ? (const uint64_t *)c->ntaint.ptr : nullptr, (const uint32_t *)c->nlab.ptr, n_keys, c->nrec.ptr, n);
        HIPCHK(c, hipGetLastError());
    }
    if (int rc = index_build(c, plan, true, cpu, mem, lab, taints)) return rc;
    return chg.commit(Stale::kEverything);
} KSCHED_ABI_CATCH(c)

int ksched_update_node_labels(ksched_ctx *c, uint32_t count, const uint32_t *node_index, const uint32_t *lab, const uint64_t *taints) try {
    if (!c) return KSCHED_E_INVAL;
    if (count > 0 && !node_index) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    const uint32_t n = c->n, nkeys = c->nkeys;
    if (count > 0 && nkeys > 0 && !lab) return KSCHED_E_INVAL;
    for (uint32_t i = 0; i < count; ++i)
        if (node_index[i] >= n) return KSCHED_E_INVAL;
    for (size_t i = 0; i < (size_t)nkeys * count; ++i)
        if (lab[i] == KSCHED_SEL_NEVER) return KSCHED_E_INVAL;
    if (count == 0) return KSCHED_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    fault_point(c);  // (nothing has changed yet)
    std::vector<uint32_t> keep, tiles;
    last_wins(node_index, count, keep, tiles);
    const uint32_t m = (uint32_t)keep.size();
    // Does the planned layout still hold?  Otherwise re-plan with the union of the old and the new maxima and bits, and rebuild the
    // whole index.  (The ctx's plan inputs change only once the change has begun.)
    uint32_t lab_max[KSCHED_MAX_KEYS];
    std::copy(c->plan_lab_max, c->plan_lab_max + KSCHED_MAX_KEYS, lab_max);
    uint64_t all_taints = c->plan_taints;
    const bool holds = label_layout_holds(lab_max, &all_taints, c->idx.built, c->idx.lay.ngroups, nkeys, count, keep.data(), m, lab, taints);
    SnapshotChange chg;
    if (int rc = chg.begin(c)) return rc;
    IndexPlan plan;
    if (holds) c->plan_taints = all_taints;  // (same groups)
    else index_plan(c, n, nkeys, lab_max, all_taints, plan);
    // the kept rows -> pinned staging -> one copy: [taints m][node m][ids nkeys x m][tiles]; the meta words (re-plan) lie after what
    // is copied and travel by index_reserve
    StageLayout f;
    const size_t o_taint = f.add<uint64_t>(taints ? m : 0), o_idx = f.add<uint32_t>(m), o_lab = f.add<uint32_t>((size_t)nkeys * m);
    const size_t o_tiles = f.add<uint32_t>(tiles.size()), b_dev = f.total, o_meta = f.add<uint32_t>(plan.indexed ? kPlanMetaWords : 0);
    uint8_t *h = nullptr;
    if (int rc = chg.stage(f.total, b_dev, &h)) return rc;
    uint64_t *ht = reinterpret_cast<uint64_t *>(h + o_taint);
    uint32_t *hi = reinterpret_cast<uint32_t *>(h + o_idx), *hl = reinterpret_cast<uint32_t *>(h + o_lab);
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t i = keep[j];
        hi[j] = node_index[i];
        if (taints) ht[j] = taints[i];
        for (uint32_t k = 0; k < nkeys; ++k) hl[(size_t)k * m + j] = lab[(size_t)k * count + i];
    }
    memcpy(h + o_tiles, tiles.data(), tiles.size() * 4);
    if (!holds)
        if (int rc = index_reserve(c, plan, h + o_meta)) return rc;
    if (int rc = chg.upload(b_dev)) return rc;
    if (taints && !c->have_taints) {  // taints on a snapshot set without them: every other node has none
        HIPCHK(c, hipMemsetAsync(c->ntaint.ptr, 0, (size_t)n * 8, change_stream(c)));
        c->have_taints = true;
    }
    PatchLabelsArgs pa{};
    pa.nlab = c->nlab.ptr;
    pa.ntaint = taints ? c->ntaint.ptr : nullptr;
    pa.nrec = c->nrec.ptr;
    const uint8_t *d = c->d_stage.ptr;
    pa.taints = taints ? reinterpret_cast<const uint64_t *>(d + o_taint) : nullptr;
    pa.idx = reinterpret_cast<const uint32_t *>(d + o_idx);
    pa.lab = reinterpret_cast<const uint32_t *>(d + o_lab);
    pa.count = m;
    pa.n = n;
    pa.nkeys = nkeys;
    hipLaunchKernelGGL(k_patch_labels, dim3((m + 255u) / 256u), dim3(256), 0, change_stream(c), pa);
    HIPCHK(c, hipGetLastError());
    if (holds) {
        // only the touched 1024-node tiles are re-indexed: their named rows and list slots (the fit part reads `available` only)
        const uint32_t *d_tiles = reinterpret_cast<const uint32_t *>(d + o_tiles);
        if (int rc = launch_build_named(c, d_tiles, (uint32_t)tiles.size())) return rc;
        if (int rc = launch_build_lists(c, d_tiles, (uint32_t)tiles.size())) return rc;
    } else {
        if (int rc = index_build(c, plan, false, nullptr, nullptr, nullptr, nullptr)) return rc;
    }
    return chg.commit(Stale::kLabels);  // the best-fit ORDER reads `available` only: the next PICK_BESTFIT request rebuilds the rows alone
} KSCHED_ABI_CATCH(c)

int ksched_update_nodes(ksched_ctx *c, uint32_t count, const uint32_t *node_index, const int64_t *cpu, const int64_t *mem) try {
    if (!c) return KSCHED_E_INVAL;
    if (count > 0 && (!node_index || !cpu || !mem)) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    for (uint32_t i = 0; i < count; ++i)
        if (node_index[i] >= c->n) return KSCHED_E_INVAL;
    if (count == 0) return KSCHED_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    fault_point(c);  // (nothing has changed yet: an exception up to snapshot_begin leaves the snapshot as it was)
    std::vector<uint32_t> keep, tiles;
    last_wins(node_index, count, keep, tiles);
    const uint32_t m = (uint32_t)keep.size();
    SnapshotChange chg;
    if (int rc = chg.begin(c)) return rc;
    PatchArgs pa{};
    pa.ncpu = c->ncpu.ptr;
    pa.nmem = c->nmem.ptr;
    pa.nrec = c->nrec.ptr;
    pa.count = m;
    const uint32_t *d_tiles = nullptr;
    if (m <= kPatchInline && tiles.size() <= kPatchInline) {
        // small updates (the watch-event case) travel in kernel arguments: no copy, no staging buffer
        for (uint32_t j = 0; j < m; ++j) {
            pa.idx_in[j] = node_index[keep[j]];
            pa.cpu_in[j] = cpu[keep[j]];
            pa.mem_in[j] = mem[keep[j]];
        }
    } else {
        StageLayout f;  // [node m][cpu m][mem m][tiles], one copy
        const size_t o_idx = f.add<uint32_t>(m), o_cpu = f.add<int64_t>(m), o_mem = f.add<int64_t>(m), o_tiles = f.add<uint32_t>(tiles.size());
        uint8_t *h = nullptr;
        if (int rc = chg.stage(f.total, f.total, &h)) return rc;
        uint32_t *hi = reinterpret_cast<uint32_t *>(h + o_idx);
        int64_t *hc = reinterpret_cast<int64_t *>(h + o_cpu), *hm = reinterpret_cast<int64_t *>(h + o_mem);
        for (uint32_t j = 0; j < m; ++j) {
            hi[j] = node_index[keep[j]];
            hc[j] = cpu[keep[j]];
            hm[j] = mem[keep[j]];
        }
        memcpy(h + o_tiles, tiles.data(), tiles.size() * 4);
        if (int rc = chg.upload(f.total)) return rc;
        const uint8_t *d = c->d_stage.ptr;
        pa.idx = reinterpret_cast<const uint32_t *>(d + o_idx);
        pa.cpu = reinterpret_cast<const int64_t *>(d + o_cpu);
        pa.mem = reinterpret_cast<const int64_t *>(d + o_mem);
        d_tiles = reinterpret_cast<const uint32_t *>(d + o_tiles);
    }
    if (c->idx.built && !d_tiles) {  // small update: the tile list rides in the patch kernel's arguments
        HIPCHK(c, c->d_stage.reserve(kPatchInline * 4));
        pa.tile_out = reinterpret_cast<uint32_t *>(c->d_stage.ptr);
        pa.ntiles = (uint32_t)tiles.size();
        for (size_t j = 0; j < tiles.size(); ++j) pa.tiles_in[j] = tiles[j];
        d_tiles = pa.tile_out;
    }
    hipLaunchKernelGGL(k_patch_nodes, dim3((m + 255u) / 256u), dim3(256), 0, change_stream(c), pa);
    HIPCHK(c, hipGetLastError());
    if (c->idx.built) {
        // only the touched 1024-node tiles are re-indexed (fit rows, search trees, cnt tables); label and taint rows are untouched
        if (int rc = launch_build_fit(c, d_tiles, (uint32_t)tiles.size())) return rc;
    }
    return chg.commit(Stale::kAvailable);
} KSCHED_ABI_CATCH(c)

int ksched_read_nodes(ksched_ctx *c, uint32_t first, uint32_t count, int64_t *out_cpu, int64_t *out_mem) try {
    if (!c) return KSCHED_E_INVAL;
    if (count > 0 && (!out_cpu || !out_mem)) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    if ((uint64_t)first + count > c->n) return KSCHED_E_INVAL;
    if (count == 0) return KSCHED_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    fault_point(c);
    HIPCHK(c, hipEventSynchronize(c->ev_build));  // the latest snapshot change, whichever stream carried it
    HIPCHK(c, hipMemcpy(out_cpu, c->ncpu.ptr + first, (size_t)count * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_mem, c->nmem.ptr + first, (size_t)count * 8, hipMemcpyDeviceToHost));
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_eval_device_pitched(ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel,
                               const uint64_t *ptol, const uint32_t *samples, uint32_t attempts, uint32_t flags,
                               uint64_t *out_feas, uint64_t *out_fit, int32_t *out_binding, uint32_t mask_pitch_words,
                               void *hip_stream) try {
    if (!c) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    const EvalRequest r{p, pcpu, pmem, psel, ptol, samples, attempts, flags, out_feas, out_fit, out_binding, mask_pitch_words, (hipStream_t)hip_stream};
    int rc = check_eval_args(r, /*combine_accepted=*/true);
    if (rc) return rc;
    if (mask_pitch_words < c->W) return KSCHED_E_INVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    return eval_on_device(c, r);
} KSCHED_ABI_CATCH(c)

int ksched_eval_device(ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel,
                       const uint64_t *ptol, const uint32_t *samples, uint32_t attempts, uint32_t flags,
                       uint64_t *out_feas, uint64_t *out_fit, int32_t *out_binding, void *hip_stream) try {
    return ksched_eval_device_pitched(c, p, pcpu, pmem, psel, ptol, samples, attempts, flags, out_feas, out_fit, out_binding,
                                      ksched_mask_words(ksched_num_nodes(c)), hip_stream);
} KSCHED_ABI_CATCH(c)

uint32_t ksched_mask_pitch(uint32_t n_nodes) { return (ksched_mask_words(n_nodes) + 15u) & ~15u; }

struct ksched_pipe {
    ksched_ctx *ctx = nullptr;
    uint32_t depth = 0;
    std::vector<hipStream_t> streams;  // by pipe_plan.hpp's index: 0 the mask stream, 1 the pick stream, 2 .. the alternate mode's further ones (created on first use)
    std::vector<hipEvent_t> mask_done, pick_done;
    std::vector<PipeSlot> slots;  // what plan_pipe_submit orders a slot's next submit by
};

int ksched_pipe_create(ksched_ctx *c, uint32_t depth, ksched_pipe **out) try {
    if (!c || !out || depth == 0 || depth > 64) return KSCHED_E_INVAL;  // (a slot is two events and the caller's buffers: 64 is plenty for "enough masks in flight to exceed the Infinity Cache")
    *out = nullptr;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    ksched_pipe *q = new (std::nothrow) ksched_pipe();
    if (!q) return KSCHED_E_NOMEM;
    q->ctx = c;
    q->depth = depth;
    q->slots.assign(depth, PipeSlot{});
    bool ok = true;
    for (int i = 0; ok && i <= kPipePickStream; ++i) {  // the mask stream and the pick stream
        hipStream_t s = nullptr;
        ok = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
        if (ok) q->streams.push_back(s);
    }
    for (uint32_t i = 0; ok && i < 2 * depth; ++i) {
        hipEvent_t e;
        ok = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (ok) (i < depth ? q->mask_done : q->pick_done).push_back(e);
    }
    if (!ok) {
        ksched_pipe_destroy(q);
        return KSCHED_E_HIP;
    }
    *out = q;
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

void ksched_pipe_destroy(ksched_pipe *q) try {
    if (!q) return;
    {
        DeviceGuard g(q->ctx->device);
        for (auto st : q->streams) (void)hipStreamSynchronize(st);
        {
            std::lock_guard<std::mutex> lk(q->ctx->mu);  // the ctx must not record events on streams that are about to go away
            for (auto st : q->streams) stream_forget(q->ctx, st);
        }
        for (auto e : q->mask_done) (void)hipEventDestroy(e);
        for (auto e : q->pick_done) (void)hipEventDestroy(e);
        for (auto st : q->streams) (void)hipStreamDestroy(st);
    }
    delete q;
} catch (...) {  // nothing unwinds across the C ABI
}

void *ksched_pipe_stream(ksched_pipe *q, int which) try {
    if (!q || which < 0) return nullptr;
    std::lock_guard<std::mutex> lk(q->ctx->mu);  // (ksched_pipe_submit grows `streams` under the same lock)
    return (size_t)which < q->streams.size() ? (void *)q->streams[(size_t)which] : nullptr;
} catch (...) {
    return nullptr;
}

// the stream that carried the slot's latest evaluation in the alternate mode / its pick in the split mode: what a consumer of the
// slot's bindings (the all-gather) has to be enqueued behind
void *ksched_pipe_slot_stream(ksched_pipe *q, uint32_t slot) try {
    if (!q || slot >= q->depth) return nullptr;
    std::lock_guard<std::mutex> lk(q->ctx->mu);
    return q->slots[slot].used() ? (void *)q->streams[(size_t)q->slots[slot].pick_stream] : nullptr;
} catch (...) {
    return nullptr;
}

// check, plan (pipe_plan.hpp: the streams, the waits and their reasons), execute
int ksched_pipe_submit(ksched_pipe *q, uint32_t slot, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel,
                       const uint64_t *ptol, const uint32_t *samples, uint32_t attempts, uint32_t flags, uint64_t *mask,
                       uint32_t mask_pitch_words, int32_t *binding) try {
    if (!q || slot >= q->depth) return KSCHED_E_INVAL;
    ksched_ctx *c = q->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    const uint32_t pick = flags & KSCHED_PICK_ANY;
    if (!pick || (flags & KSCHED_WANT_FIT_MASK) || !mask) return KSCHED_E_INVAL;
    EvalRequest r{p, pcpu, pmem, psel, ptol, samples, attempts, flags, mask, nullptr, binding, mask_pitch_words, nullptr};  // (the stream: the plan's)
    int rc = check_eval_args(r, /*combine_accepted=*/false, /*selop_accepted=*/false);
    if (rc) return rc;
    if (mask_pitch_words < c->W) return KSCHED_E_INVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    const bool reads_mask = pick_reads_mask(flags, c->opt_pick_from_mask, bf_rows_expected(c));
    const PipePlan pl = plan_pipe_submit(q->slots[slot], slot, c->opt_pipe_mode, reads_mask);
    const hipEvent_t mask_done = q->mask_done[slot], pick_done = q->pick_done[slot];
    while (q->streams.size() <= (size_t)pl.pick_stream) {  // a further stream of the alternate mode, on first use (pl.mask_stream is the same one, or stream 0)
        hipStream_t ns = nullptr;
        HIPCHK(c, hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
        q->streams.push_back(ns);
    }
    const hipStream_t sm = q->streams[(size_t)pl.mask_stream], sp = q->streams[(size_t)pl.pick_stream];
    if (pl.mask_waits_pick_done) HIPCHK(c, hipStreamWaitEvent(sm, pick_done, 0));
    if (pl.mask_waits_mask_done) HIPCHK(c, hipStreamWaitEvent(sm, mask_done, 0));
    if (pl.pick_waits_pick_done) HIPCHK(c, hipStreamWaitEvent(sp, pick_done, 0));
    q->slots[slot] = pl.next;
    r.stream = sp;
    if (pl.whole) {  // one launch when the pick rides in the mask kernel
        if ((rc = eval_on_device(c, r))) return rc;
    } else {
        if ((rc = eval_on_device(c, EvalRequest{p, pcpu, pmem, psel, ptol, nullptr, 0, flags & ~pick, mask, nullptr, nullptr, mask_pitch_words, sm}))) return rc;
        if (pl.record_mask_done) HIPCHK(c, hipEventRecord(mask_done, sm));
        if (pl.pick_waits_mask_done) HIPCHK(c, hipStreamWaitEvent(sp, mask_done, 0));
        r.out_feas = nullptr;  // (no mask kernel on the pick stream: the pick from the mask, or the bindings-only evaluation, which launches the pick kernel alone)
        if ((rc = reads_mask ? pick_from_mask(c, r, mask) : eval_on_device(c, r))) return rc;
    }
    HIPCHK(c, hipEventRecord(pick_done, sp));
    return KSCHED_OK;
} KSCHED_ABI_CATCH((q ? q->ctx : nullptr))

int ksched_pipe_wait(ksched_pipe *q, uint32_t slot, void *hip_stream) try {
    if (!q || slot >= q->depth) return KSCHED_E_INVAL;
    ksched_ctx *c = q->ctx;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    if (hip_stream) HIPCHK(c, hipStreamWaitEvent((hipStream_t)hip_stream, q->pick_done[slot], 0));
    else HIPCHK(c, hipEventSynchronize(q->pick_done[slot]));
    return KSCHED_OK;
} KSCHED_ABI_CATCH((q ? q->ctx : nullptr))

int ksched_pipe_wait_mask(ksched_pipe *q, uint32_t slot, void *hip_stream) try {
    if (!q || slot >= q->depth) return KSCHED_E_INVAL;
    ksched_ctx *c = q->ctx;
    std::lock_guard<std::mutex> lk(c->mu);  // (ksched_pipe_submit records the same events)
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    // The mask stream is in order: "everything enqueued on it so far" contains the slot's latest mask kernel.  Recorded here, on
    // demand, so that the submit path carries no event for consumers that never read the masks.
    const PipeSlot &sl = q->slots[slot];
    HIPCHK(c, hipEventRecord(q->mask_done[slot], q->streams[(size_t)(sl.used() ? sl.mask_stream : kPipeMaskStream)]));
    if (hip_stream) HIPCHK(c, hipStreamWaitEvent((hipStream_t)hip_stream, q->mask_done[slot], 0));
    else HIPCHK(c, hipEventSynchronize(q->mask_done[slot]));
    return KSCHED_OK;
} KSCHED_ABI_CATCH((q ? q->ctx : nullptr))

int ksched_pick_device(ksched_ctx *c, uint32_t p, const uint64_t *feasible, uint32_t mask_pitch_words, const int64_t *req_mem_bytes,
                       const uint32_t *samples, uint32_t attempts, uint32_t flags, int32_t *out_binding, void *hip_stream) try {
    if (!c) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    if (int rc = check_pick_args(c->n, p, feasible, req_mem_bytes, samples, attempts, flags, out_binding)) return rc;
    if (mask_pitch_words < c->W) return KSCHED_E_INVAL;
    if (p == 0) return KSCHED_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    return pick_from_mask(c, EvalRequest{p, nullptr, req_mem_bytes, nullptr, nullptr, samples, attempts, flags, nullptr, nullptr, out_binding, mask_pitch_words, (hipStream_t)hip_stream}, feasible);
} KSCHED_ABI_CATCH(c)

// The pick alone from HOST masks (packed rows of W words): copies in, ksched_pick_device on the ctx's stream, copies out, waits.
int ksched_pick(ksched_ctx *c, uint32_t p, const uint64_t *feasible, const int64_t *req_mem_bytes, const uint32_t *samples, uint32_t attempts,
                uint32_t flags, int32_t *out_binding) try {
    if (!c) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    // (pick_s: the pick reads draws -- sampled, uniform, spread or pack)
    const bool pick_s = flags & KSCHED_PICK_DRAWS, pick_b = flags & KSCHED_PICK_BESTFIT;
    if (int rc = check_pick_args(c->n, p, feasible, req_mem_bytes, samples, attempts, flags, out_binding)) return rc;
    if (p == 0) return KSCHED_OK;
    if (c->n == 0) {  // choose() on an empty store yields None on every attempt (src/main.rs:56,70)
        for (uint32_t i = 0; i < p; ++i) out_binding[i] = -1;
        return KSCHED_OK;
    }
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    fault_point(c);
    hipStream_t s = c->stream;
    if (pick_b)
        if (int rcb = ensure_bestfit(c)) return rcb;
    if (int rce = stream_enter(c, s)) return rce;  // behind the latest snapshot change
    const size_t W = c->W;
    HIPCHK(c, c->feas.reserve((size_t)p * W));
    HIPCHK(c, c->binding.reserve(p));
    HIPCHK(c, hipMemcpyAsync(c->feas.ptr, feasible, (size_t)p * W * 8, hipMemcpyHostToDevice, s));
    HostBatch h;
    h.pmem = req_mem_bytes;
    if (pick_s) h.samples = samples, h.attempts = attempts;
    if (int rc = stage_batch(c, p, h, s)) return rc;
    const EvalRequest r{p, nullptr, req_mem_bytes ? c->pmem.ptr : nullptr, nullptr, nullptr, pick_s ? c->psamples.ptr : nullptr, attempts, flags,
                        nullptr, nullptr, c->binding.ptr, (uint32_t)W, s};
    if (int rc = launch_pick(c, r, c->feas.ptr)) return rc;
    HIPCHK(c, hipMemcpyAsync(out_binding, c->binding.ptr, (size_t)p * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

// ---- the host-pointer evaluation in two halves (include/ksched.h "one host thread, several devices") -------------------------
// eval_begin_locked: copy the batch in, enqueue the evaluation and the copies of the masks back -- all on the ctx's own stream, no
// host wait.  The bindings stay in a ctx-owned device buffer of `capacity` >= p entries; entries [p, capacity) are -1 (the padding
// an all-gather of unequal shards needs).  The caller holds the ctx's mutex and has checked the arguments.  `h`: the batch as the
// caller gave it -- HOST pointers, selectors sel_stride entries per key apart, packed output masks.
namespace {
int eval_begin_locked(ksched_ctx *c, const EvalRequest &h, uint32_t sel_stride, uint32_t capacity, int32_t **binding_dev) {
    hipStream_t s = c->stream;
    const uint32_t p = h.p, flags = h.flags;
    uint64_t *const out_feas = h.out_feas, *const out_fit = h.out_fit;
    const size_t W = c->W;
    const size_t pitch = ksched_mask_pitch(c->n);
    const bool pick = flags & KSCHED_PICK_ANY;
    HostBatch b;  // what is uploaded: the requests always, selectors and tolerations where their term is active, the draws of a sampled, uniform, spread or pack pick
    b.pcpu = h.pcpu;
    b.pmem = h.pmem;
    if (h.sel(c->nkeys)) b.psel = h.psel, b.sel_stride = sel_stride, b.terms = sel_terms(flags);
    if (h.taint_flag()) b.ptol = h.ptol;
    if (flags & KSCHED_PICK_DRAWS) b.samples = h.samples, b.attempts = h.attempts;
    int32_t *d_bind = nullptr;
    if (pick) {
        const size_t cap = std::max<size_t>(capacity, p);
        HIPCHK(c, c->binding.reserve(cap));
        d_bind = c->binding.ptr;
        if (cap > p) HIPCHK(c, hipMemsetAsync(d_bind + p, 0xFF, (cap - p) * sizeof(int32_t), s));  // -1: "no node" rows past this shard's end
    }
    if (binding_dev) *binding_dev = d_bind;
    if (p == 0) return KSCHED_OK;  // (a rank whose shard is empty still takes part in the exchange with `capacity` rows of -1)

    if (int rc = stage_batch(c, p, b, s)) return rc;
    uint64_t *d_feas = nullptr, *d_fit = nullptr;
    // a mask is needed when the caller wants it, or when the pick reads it (uniform, spread and pack; best fit; sampled only with KSCHED_OPT_PICK_FROM_MASK)
    if (out_feas || pick_reads_mask(flags, c->opt_pick_from_mask, bf_rows_expected(c))) {
        HIPCHK(c, c->feas.reserve((size_t)p * pitch));
        d_feas = c->feas.ptr;
    }
    if (out_fit) {
        HIPCHK(c, c->fit.reserve((size_t)p * pitch));
        d_fit = c->fit.ptr;
    }
    if (int rc = eval_on_device(c, EvalRequest{p, c->pcpu.ptr, c->pmem.ptr, b.psel ? c->psel.ptr : nullptr, b.ptol ? c->ptol.ptr : nullptr, c->psamples.ptr,
                                               h.attempts, flags, d_feas, d_fit, d_bind, (uint32_t)pitch, s}))
        return rc;
    // device rows are line-aligned (pitch words apart); the caller's rows are packed (W words)
    if (out_feas && W)
        HIPCHK(c, hipMemcpy2DAsync(out_feas, W * 8, d_feas, pitch * 8, W * 8, p, hipMemcpyDeviceToHost, s));
    if (out_fit && W)
        HIPCHK(c, hipMemcpy2DAsync(out_fit, W * 8, d_fit, pitch * 8, W * 8, p, hipMemcpyDeviceToHost, s));
    return KSCHED_OK;
}
}  // namespace

int ksched_eval(ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel,
                const uint64_t *ptol, const uint32_t *samples, uint32_t attempts, uint32_t flags, uint64_t *out_feas,
                uint64_t *out_fit, int32_t *out_binding) try {
    if (!c) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    const EvalRequest h{p, pcpu, pmem, psel, ptol, samples, attempts, flags, out_feas, out_fit, out_binding, 0, c->stream};
    int rc = check_eval_args(h);
    if (rc) return rc;
    if (p == 0) return KSCHED_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    int32_t *d_bind = nullptr;
    rc = eval_begin_locked(c, h, p, p, &d_bind);
    if (rc) return rc;
    if (d_bind && out_binding) HIPCHK(c, hipMemcpyAsync(out_binding, d_bind, (size_t)p * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

void ksched_shard_bounds(uint32_t p, uint32_t nranks, uint32_t rank, uint32_t *lo, uint32_t *hi, uint32_t *count_per_rank) {
    // rank r owns pod rows [r * shard, min(p, (r + 1) * shard)), shard = ceil(p / nranks): the last ranks may own fewer rows, or none
    const uint64_t shard = nranks ? ((uint64_t)p + nranks - 1u) / nranks : p;
    const uint64_t l = std::min<uint64_t>(p, shard * rank), h = std::min<uint64_t>(p, l + shard);
    if (lo) *lo = (uint32_t)l;
    if (hi) *hi = (uint32_t)h;
    if (count_per_rank) *count_per_rank = (uint32_t)shard;
}

int ksched_eval_begin(ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel, uint32_t sel_stride,
                      const uint64_t *ptol, const uint32_t *samples, uint32_t attempts, uint32_t flags, uint64_t *out_feas,
                      uint64_t *out_fit, uint32_t binding_capacity, int32_t **binding_dev, void **hip_stream) try {
    if (!c || !binding_dev || !hip_stream) return KSCHED_E_INVAL;
    *binding_dev = nullptr;
    *hip_stream = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    if (psel && sel_stride < p) return KSCHED_E_INVAL;
    int32_t sentinel = 0;  // (the bindings stay on the device: check_eval_args only wants to know that a pick has somewhere to go)
    const EvalRequest h{p, pcpu, pmem, psel, ptol, samples, attempts, flags, out_feas, out_fit,
                        (flags & KSCHED_PICK_ANY) ? &sentinel : nullptr, 0, c->stream};
    int rc = check_eval_args(h);
    if (rc) return rc;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    rc = eval_begin_locked(c, h, sel_stride, binding_capacity, binding_dev);
    if (rc) return rc;
    *hip_stream = (void *)c->stream;
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

// ---- mask buffers owned by the library (mask_alloc.hpp; profiles/r06_mask_alloc.md) ---------------------------------------------
namespace {
// one buffer through one allocation path (never AUTO / PROBE).  *unsupported: a measurement path asked of the shipped library.
hipError_t mask_alloc_path(ksched_ctx *c, size_t bytes, uint32_t how, MaskAllocation &a, bool *unsupported = nullptr) {
    a = MaskAllocation();
    a.bytes = bytes;
    a.device = c->device;
    a.owner = c;
    a.how = how;
    if (how == KSCHED_MASK_ALLOC_PLAIN) return hipMalloc(&a.ptr, bytes);
    // VMM, VMM_MIN, CONTIGUOUS, SCATTER_*: tests/cpp/test_hooks.cpp, linked into the test build only (mask_alloc.hpp)
    if (ksched_test_mask_alloc == nullptr) {
        if (unsupported) *unsupported = true;
        return hipErrorNotSupported;
    }
    const int rc = ksched_test_mask_alloc(c->device, bytes, how, &a.ptr, &a.test_token);
    return rc == 0 ? hipSuccess : rc > 0 ? (hipError_t)rc : hipErrorInvalidValue;
}

// Probe-and-keep (KSCHED_MASK_ALLOC_PROBE).  The rate of the mask kernel into a buffer is a property of the buffer's physical placement
// (HBM-side write stalls, TCC_EA0_WRREQ_DRAM_CREDIT_STALL: profiles/r06_mask_alloc.md) that no allocation path selects and user space
// cannot see -- but it is sticky per allocation and the kernel itself measures it: `k` candidates over different paths, ALL alive at once
// (a freed buffer's pages come straight back), the fused mask kernel timed into each (fit only, zero requests: every pair feasible
// or not by the node's sign, the same 128-byte segments at the same addresses as any other instantiation), the fastest kept.
int mask_alloc_probe(ksched_ctx *c, uint32_t p, uint32_t pitch, size_t bytes, MaskAllocation &best) {
    // (hipMalloc only: the virtual-memory paths gave the same ladder of rates and showed stale reads on a mapping's first use after memory-pool
    // activity in the process -- profiles/r06_mask_alloc.md section 3; candidates kept alive side by side land on different physical blocks anyway)
    static const uint32_t paths[] = {KSCHED_MASK_ALLOC_PLAIN, KSCHED_MASK_ALLOC_PLAIN, KSCHED_MASK_ALLOC_PLAIN, KSCHED_MASK_ALLOC_PLAIN};  // (hipMalloc and nothing else)
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const uint32_t k = (uint32_t)std::max<size_t>(1, std::min<size_t>(c->opt_mask_probe, free_b / 4 / std::max<size_t>(bytes, 1)));
    std::vector<MaskAllocation> cand;
    auto release_all = [&](size_t keep) {
        for (size_t i = 0; i < cand.size(); ++i)
            if (i != keep) (void)mask_release(cand[i]);
    };
    for (uint32_t i = 0; i < k; ++i) {
        MaskAllocation a;
        hipError_t e = mask_alloc_path(c, bytes, paths[i % 4u], a);
        if (e != hipSuccess || !a.ptr) {
            (void)hipGetLastError();
            if (!cand.empty()) break;  // fewer candidates than asked for
            e = mask_alloc_path(c, bytes, KSCHED_MASK_ALLOC_PLAIN, a);
            if (e != hipSuccess || !a.ptr) {
                c->last_error = std::string("ksched_mask_alloc: ") + hipGetErrorString(e);
                (void)hipGetLastError();
                return e == hipErrorOutOfMemory ? KSCHED_E_NOMEM : KSCHED_E_HIP;
            }
        }
        cand.push_back(a);
    }
    size_t keep = 0;
    std::fill(std::begin(c->mask_probe_us), std::end(c->mask_probe_us), 0.0);
    if (cand.size() > 1) {
        // zero requests for `p` pods in the ctx's own operand scratch (the host-pointer path's; nothing else uses it while the ctx is locked)
        hipError_t e = c->pcpu.reserve(p);
        if (e == hipSuccess) e = c->pmem.reserve(p);
        if (e == hipSuccess) e = hipMemsetAsync(c->pcpu.ptr, 0, (size_t)p * 8u, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->pmem.ptr, 0, (size_t)p * 8u, c->stream);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (e == hipSuccess) e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        const uint32_t timing = c->opt_timing;
        const int kern = c->opt_kernel;
        c->opt_timing = 0;
        c->opt_kernel = KSCHED_KERNEL_FUSED;
        int rc = e == hipSuccess ? KSCHED_OK : KSCHED_E_HIP;
        double best_us = 0;
        constexpr int kReps = 4;
        for (int pass = 0; pass < 2 && rc == KSCHED_OK; ++pass)  // two passes: the first candidates of the first pass carry the warm-up
            for (size_t i = 0; i < cand.size() && rc == KSCHED_OK; ++i) {
                rc = eval_on_device(c, EvalRequest{p, c->pcpu.ptr, c->pmem.ptr, nullptr, nullptr, nullptr, 0, KSCHED_FIT, (uint64_t *)cand[i].ptr, nullptr, nullptr, pitch, c->stream});
                if (rc) break;
                if (hipEventRecord(e0, c->stream) != hipSuccess) rc = KSCHED_E_HIP;
                for (int r = 0; r < kReps && rc == KSCHED_OK; ++r)
                    rc = eval_on_device(c, EvalRequest{p, c->pcpu.ptr, c->pmem.ptr, nullptr, nullptr, nullptr, 0, KSCHED_FIT, (uint64_t *)cand[i].ptr, nullptr, nullptr, pitch, c->stream});
                if (rc == KSCHED_OK && (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) rc = KSCHED_E_HIP;
                float ms = 0;
                if (rc == KSCHED_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = KSCHED_E_HIP;
                if (rc == KSCHED_OK && pass == 1) {
                    const double us = (double)ms * 1e3 / kReps;
                    if (i < 16) c->mask_probe_us[i] = us;
                    if (i == 0 || us < best_us) {
                        best_us = us;
                        keep = i;
                    }
                }
            }
        c->opt_timing = timing;
        c->opt_kernel = kern;
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipStreamSynchronize(c->stream);
        if (rc != KSCHED_OK) {  // the probe could not run (no bitmap index for this snapshot, ...): the first candidate as it is
            (void)hipGetLastError();
            keep = 0;
        }
    }
    release_all(keep);
    best = cand[keep];
    return KSCHED_OK;
}
}  // namespace

int ksched_mask_alloc(ksched_ctx *c, uint32_t p, uint32_t how, uint64_t **out_mask, uint32_t *out_pitch_words) try {
    if (!c || !out_mask) return KSCHED_E_INVAL;
    *out_mask = nullptr;
    switch (how) {  // (3, 6, 7, 10: paths measured in round 6 and removed)
        case KSCHED_MASK_ALLOC_AUTO: case KSCHED_MASK_ALLOC_PLAIN: case KSCHED_MASK_ALLOC_PROBE: case KSCHED_MASK_ALLOC_VMM: case KSCHED_MASK_ALLOC_VMM_MIN:
        case KSCHED_MASK_ALLOC_CONTIGUOUS: case KSCHED_MASK_ALLOC_SCATTER_2M: case KSCHED_MASK_ALLOC_SCATTER_16M: break;
        default: return KSCHED_E_INVAL;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) {
        c->last_error = "ksched_mask_alloc before ksched_set_nodes: the row pitch follows the node count";
        return KSCHED_E_STATE;
    }
    fault_point(c);
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    const uint32_t pitch = ksched_mask_pitch(c->n);
    if (out_pitch_words) *out_pitch_words = pitch;
    const size_t bytes = std::max<size_t>((size_t)p * pitch * 8u, 128u);
    uint32_t eff = how;
    if (how == KSCHED_MASK_ALLOC_AUTO) eff = (bytes >= KSCHED_MASK_PROBE_MIN_BYTES && c->idx.built && c->opt_mask_probe > 1u) ? KSCHED_MASK_ALLOC_PROBE : KSCHED_MASK_ALLOC_PLAIN;
    MaskAllocation a;
    std::fill(std::begin(c->mask_probe_us), std::end(c->mask_probe_us), 0.0);
    if (eff == KSCHED_MASK_ALLOC_PROBE) {
        const int rc = mask_alloc_probe(c, p, pitch, bytes, a);
        if (rc) return rc;
    } else {
        bool unsupported = false;
        const hipError_t e = mask_alloc_path(c, bytes, eff, a, &unsupported);
        if (unsupported) {
            c->last_error = "ksched_mask_alloc: this allocation path is a measurement path of the test build of the library (tests/cpp/hooks); the shipped library allocates with hipMalloc only";
            return KSCHED_E_UNSUPPORTED;
        }
        if (e != hipSuccess || !a.ptr) {
            c->last_error = std::string("ksched_mask_alloc: ") + hipGetErrorString(e);
            (void)hipGetLastError();
            return e == hipErrorOutOfMemory ? KSCHED_E_NOMEM : KSCHED_E_HIP;
        }
    }
    {
        MaskRegistry &reg = mask_registry();
        std::lock_guard<std::mutex> rl(reg.mu);
        reg.live.push_back(a);
    }
    *out_mask = (uint64_t *)a.ptr;
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_mask_probe_report(ksched_ctx *c, double *out_us, uint32_t cap) try {
    if (!c || (cap && !out_us)) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    uint32_t n = 0;
    while (n < 16u && c->mask_probe_us[n] > 0.0) ++n;
    n = std::min(n, cap);
    for (uint32_t i = 0; i < n; ++i) out_us[i] = c->mask_probe_us[i];
    return (int)n;
} KSCHED_ABI_CATCH(c)

int ksched_mask_free(ksched_ctx *c, uint64_t *mask) try {
    if (!c) return KSCHED_E_INVAL;
    if (!mask) return KSCHED_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    MaskAllocation a;
    {
        MaskRegistry &reg = mask_registry();
        std::lock_guard<std::mutex> rl(reg.mu);
        auto it = std::find_if(reg.live.begin(), reg.live.end(), [&](const MaskAllocation &m) { return m.ptr == (void *)mask; });
        if (it == reg.live.end()) {
            c->last_error = "ksched_mask_free: not a pointer ksched_mask_alloc returned (or freed already)";
            return KSCHED_E_INVAL;
        }
        a = *it;
        reg.live.erase(it);
    }
    // evaluations still writing it (any stream of the device) finish first: unmapping under a running kernel is a fault
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, mask_release(a));
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_gather_buffer(ksched_ctx *c, uint32_t count, int32_t **dev) try {
    if (!c || !dev) return KSCHED_E_INVAL;
    *dev = nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    if (count > c->gathered.cap) HIPCHK(c, hipStreamSynchronize(c->stream));  // (growing frees the old table: nothing may still be reading it)
    HIPCHK(c, c->gathered.reserve(count));
    *dev = c->gathered.ptr;
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_eval_end(ksched_ctx *c, const int32_t *bindings_dev, uint32_t count, int32_t *out_host) try {
    if (!c) return KSCHED_E_INVAL;
    if (count > 0 && out_host && !bindings_dev) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    if (count > 0 && out_host) HIPCHK(c, hipMemcpyAsync(out_host, bindings_dev, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_reason(const uint64_t *feasible_row, const uint64_t *fit_row, uint32_t node, uint32_t flags) try {
    if (!feasible_row) return KSCHED_E_INVAL;
    const uint32_t w = node >> 6, b = node & 63u;
    if ((feasible_row[w] >> b) & 1ull) return KSCHED_REASON_OK;
    // reference order: resources first (src/predicates.rs:68-70), then the selector (:72-74)
    if ((flags & KSCHED_FIT) && fit_row && !((fit_row[w] >> b) & 1ull)) return KSCHED_REASON_NOT_ENOUGH_RESOURCES;
    if ((flags & KSCHED_SEL) && !(flags & KSCHED_TAINT)) return KSCHED_REASON_NODE_SELECTOR_MISMATCH;
    if ((flags & KSCHED_TAINT) && !(flags & KSCHED_SEL)) return KSCHED_REASON_TAINT_NOT_TOLERATED;
    // both extension and selector active: the two masks cannot tell them apart
    return KSCHED_REASON_NODE_SELECTOR_MISMATCH;
} KSCHED_ABI_CATCH(nullptr)

int ksched_explain(ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel, const uint64_t *ptol,
                   uint32_t count, const uint32_t *pair_pod, const uint32_t *pair_node, uint32_t flags, int32_t *out_reason) try {
    if (!c) return KSCHED_E_INVAL;
    if (flags & ~(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT)) return KSCHED_E_INVAL;
    if (count > 0 && (!pair_pod || !pair_node || !out_reason)) return KSCHED_E_INVAL;
    if (count > 0 && (flags & KSCHED_FIT) && (!pcpu || !pmem)) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    for (uint32_t i = 0; i < count; ++i)
        if (pair_pod[i] >= p || pair_node[i] >= c->n) return KSCHED_E_INVAL;
    if (count == 0) return KSCHED_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    fault_point(c);
    hipStream_t s = c->stream;
    if (int rce = stream_enter(c, s)) return rce;  // behind the latest snapshot change, whichever stream carried it
    EvalRequest h;  // (host pointers: the normalised terms are all that is read)
    h.psel = psel;
    h.flags = flags;
    const bool use_fit = h.fit(), use_sel = h.sel(c->nkeys), use_taint = h.taint(c->have_taints);
    HostBatch b;  // requests only with KSCHED_FIT, tolerations only when the snapshot has taints
    if (use_fit) b.pcpu = pcpu, b.pmem = pmem;
    if (use_sel) b.psel = psel, b.sel_stride = p;
    if (use_taint) b.ptol = ptol;
    if (int rc = stage_batch(c, p, b, s)) return rc;
    HIPCHK(c, c->xpairs.reserve((size_t)count * 2));
    HIPCHK(c, c->xreason.reserve(count));
    HIPCHK(c, hipMemcpyAsync(c->xpairs.ptr, pair_pod, (size_t)count * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->xpairs.ptr + count, pair_node, (size_t)count * 4, hipMemcpyHostToDevice, s));
    ExplainArgs q{};
    q.nrec = c->nrec.ptr;
    q.nlab = c->nlab.ptr;
    q.ntaint = use_taint ? c->ntaint.ptr : nullptr;
    q.pcpu = c->pcpu.ptr;
    q.pmem = c->pmem.ptr;
    q.psel = use_sel ? c->psel.ptr : nullptr;
    q.ptol = (use_taint && ptol) ? c->ptol.ptr : nullptr;
    q.pair_pod = c->xpairs.ptr;
    q.pair_node = c->xpairs.ptr + count;
    q.reason = c->xreason.ptr;
    q.count = count;
    q.p = p;
    q.n = c->n;
    q.nkeys = use_sel ? c->nkeys : 0u;
    q.do_fit = use_fit ? 1u : 0u;
    q.do_taint = use_taint ? 1u : 0u;
    hipLaunchKernelGGL(k_explain_pairs, dim3((count + 255u) / 256u), dim3(256), 0, s, q);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_reason, c->xreason.ptr, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

// ---- per-pod node counts by reason (kernels_summary.hpp) ------------------------------------------------------------------------
namespace {
int check_summary_args(const ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, uint32_t flags, const uint32_t *out) {
    if (!c) return KSCHED_E_INVAL;
    if ((flags & ~(KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT)) || !(flags & (KSCHED_FIT | KSCHED_SEL | KSCHED_TAINT))) return KSCHED_E_INVAL;
    if (p > 0 && (!pcpu || !pmem || !out)) return KSCHED_E_INVAL;
    return KSCHED_OK;
}

// device pointers; the caller holds the ctx's mutex, has checked the arguments and set the device
// (of the request: p, pcpu, pmem, psel, ptol, flags and the stream)
int summarize_on_device(ksched_ctx *c, const EvalRequest &r, uint32_t *out) {
    const hipStream_t s = r.stream;
    const uint32_t p = r.p;
    if (p == 0) return KSCHED_OK;
    if (int rce = stream_enter(c, s)) return rce;  // `s` waits for the latest snapshot change; remembered for the next one
    if (c->n == 0) {  // no nodes: nothing is feasible and nothing is rejected
        HIPCHK(c, hipMemsetAsync(out, 0, (size_t)p * KSCHED_SUMMARY_WORDS * sizeof(uint32_t), s));
        return KSCHED_OK;
    }
    fault_point(c);
    // kernel choice as for evaluations: over the bitmap index when the snapshot has one, else the always-applicable direct kernel
    const bool can_indexed = summary_indexed_applicable(c->idx);
    const int kern = choose_kernel(c->opt_kernel, can_indexed);
    if (kern == KSCHED_KERNEL_FUSED && !can_indexed) return fail_fused_not_applicable(c);
    TimingBracket t;
    if (int trc = timing_begin(c, s, true, t)) return trc;
    if (kern == KSCHED_KERNEL_FUSED) {
        // (KSCHED_OPT_DEBUG bit 30: the atomic cross-tile combine, for re-measuring the choice; it needs the table on an 8-byte boundary)
        const bool atomic = (c->opt_debug & 0x40000000u) && !(reinterpret_cast<uintptr_t>(out) & 7u);
        if (!atomic) {
            if (int rsc = scratch_enter(c, s)) return rsc;
            HIPCHK(c, c->sum_part.reserve(summary_partial_words(c->idx, p)));
        }
        hipError_t e = run_summary_indexed(c->idx, r, out, c->sum_part.ptr, atomic);
        if (e != hipSuccess) return fail_hip(c, e, "run_summary_indexed");
        c->last_kernel = "fused";
    } else {
        SummaryDirectArgs a{};
        a.n = c->n;
        a.p = p;
        a.nkeys = c->nkeys;
        a.do_fit = r.fit() ? 1u : 0u;
        a.aligned = (reinterpret_cast<uintptr_t>(out) & 15u) ? 0u : 1u;
        hipLaunchKernelGGL(k_summarize_direct, dim3((p + 63u) / 64u), dim3(64 * kSummaryDirectWaves), 0, s, c->ncpu.ptr, c->nmem.ptr, c->nlab.ptr,
                           r.taint(c->have_taints) ? c->ntaint.ptr : nullptr, r.pcpu, r.pmem, r.sel(c->nkeys) ? r.psel : nullptr, r.ptol, out, a);
        HIPCHK(c, hipGetLastError());
        c->last_kernel = "direct";
    }
    return timing_end(c, s, t);
}
}  // namespace

int ksched_summarize_device(ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel, const uint64_t *ptol,
                            uint32_t flags, uint32_t *out_counts, void *hip_stream) try {
    if (int rc = check_summary_args(c, p, pcpu, pmem, flags, out_counts)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    EvalRequest r;
    r.p = p, r.pcpu = pcpu, r.pmem = pmem, r.psel = psel, r.ptol = ptol, r.flags = flags, r.stream = (hipStream_t)hip_stream;
    return summarize_on_device(c, r, out_counts);
} KSCHED_ABI_CATCH(c)

int ksched_summarize(ksched_ctx *c, uint32_t p, const int64_t *pcpu, const int64_t *pmem, const uint32_t *psel, const uint64_t *ptol,
                     uint32_t flags, uint32_t *out_counts) try {
    if (int rc = check_summary_args(c, p, pcpu, pmem, flags, out_counts)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    if (p == 0) return KSCHED_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return KSCHED_E_HIP;
    hipStream_t s = c->stream;
    EvalRequest r;  // first with the caller's host pointers, for the terms; then with the staged ones
    r.p = p, r.psel = psel, r.flags = flags, r.stream = s;
    HostBatch b;
    b.pcpu = pcpu, b.pmem = pmem;
    if (r.sel(c->nkeys)) b.psel = psel, b.sel_stride = p;
    if (r.taint_flag()) b.ptol = ptol;
    HIPCHK(c, c->sum_out.reserve((size_t)p * KSCHED_SUMMARY_WORDS));
    if (int rc = stage_batch(c, p, b, s)) return rc;
    r.pcpu = c->pcpu.ptr, r.pmem = c->pmem.ptr, r.psel = b.psel ? c->psel.ptr : nullptr, r.ptol = b.ptol ? c->ptol.ptr : nullptr;
    if (int rc = summarize_on_device(c, r, c->sum_out.ptr)) return rc;
    HIPCHK(c, hipMemcpyAsync(out_counts, c->sum_out.ptr, (size_t)p * KSCHED_SUMMARY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

// ---- multi-GPU: RCCL all-gather of the bindings (comm_rccl.hpp) --------------------------------------------------

struct ksched_comm {
    ncclComm_t comm = nullptr;
    int device = 0, rank = 0, nranks = 1;
};

namespace {
thread_local std::string g_comm_error;

int comm_fail(const char *what, ncclResult_t r) {
    RcclApi &api = rccl_api();
    g_comm_error = std::string(what) + ": " + ((api.ok && api.GetErrorString) ? api.GetErrorString(r) : "RCCL unavailable");
    return KSCHED_E_RCCL;
}
int comm_unavailable() {
    g_comm_error = rccl_api().error;
    return KSCHED_E_RCCL;
}
int comm_caught(int code, const char *what) noexcept {
    try {
        g_comm_error = std::string("exception inside the library: ") + (what ? what : "?");
    } catch (...) {
    }
    return code;
}
#define KSCHED_ABI_CATCH_COMM                                                                 \
    catch (const std::bad_alloc &) { return comm_caught(KSCHED_E_NOMEM, "std::bad_alloc"); }  \
    catch (const std::exception &e_) { return comm_caught(KSCHED_E_INVAL, e_.what()); }        \
    catch (...) { return comm_caught(KSCHED_E_INVAL, "unknown exception"); }
}  // namespace

const char *ksched_comm_last_error(void) { return g_comm_error.c_str(); }
}  // extern "C"

namespace {
// One all-gather over comms[0..n) in ncclGroupStart/End (send[i], recv[i], streams[i] belong to comms[i]; streams == nullptr: default
// streams).  If any call or the group's end fails the collective is at best half issued: ranks that did enqueue it would wait for the
// others for ever, and whoever then synchronises their stream hangs with them.  The whole clique is given up -- ncclCommAbort takes its
// outstanding work down -- and the handles are left empty: every later call with them fails with KSCHED_E_INVAL, ksched_comm_destroy
// still frees them.
int group_allgather(ksched_comm *const *comms, int n, const void *const *send, void *const *recv, size_t count, ncclDataType_t type,
                    void *const *streams, const char *what) {
    RcclApi &api = rccl_api();
    if (!api.ok) return comm_unavailable();
    // one process drives every device: the per-device calls of one collective must be fused in a group
    ncclResult_t r = api.GroupStart();
    if (r != ncclSuccess) return comm_fail("ncclGroupStart", r);
    ncclResult_t first = ncclSuccess;
    for (int i = 0; i < n; ++i) {
        DeviceGuard g(comms[i]->device);
        r = api.AllGather(send[i], recv[i], count, type, comms[i]->comm, streams ? (hipStream_t)streams[i] : nullptr);
        if (r != ncclSuccess && first == ncclSuccess) first = r;
    }
    r = api.GroupEnd();
    if (first != ncclSuccess || r != ncclSuccess) {
        for (int i = 0; i < n; ++i) {
            DeviceGuard g(comms[i]->device);
            if (api.CommAbort) (void)api.CommAbort(comms[i]->comm);
            else (void)api.CommDestroy(comms[i]->comm);
            comms[i]->comm = nullptr;
        }
        const int rc = first != ncclSuccess ? comm_fail(what, first) : comm_fail("ncclGroupEnd", r);
        g_comm_error += " -- the communicator clique has been aborted; create a new one";
        return rc;
    }
    return KSCHED_OK;
}
}  // namespace

extern "C" {


int ksched_comm_unique_id(uint8_t *id) try {
    if (!id) return KSCHED_E_INVAL;
    RcclApi &api = rccl_api();
    if (!api.ok) return comm_unavailable();
    static_assert(sizeof(ncclUniqueId) == KSCHED_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = api.GetUniqueId(&u);
    if (r != ncclSuccess) return comm_fail("ncclGetUniqueId", r);
    memcpy(id, &u, sizeof u);
    return KSCHED_OK;
} KSCHED_ABI_CATCH_COMM

int ksched_comm_create(ksched_ctx *c, const uint8_t *id, int rank, int nranks, ksched_comm **out) try {
    if (!c || !id || !out || nranks <= 0 || rank < 0 || rank >= nranks) return KSCHED_E_INVAL;
    *out = nullptr;
    RcclApi &api = rccl_api();
    if (!api.ok) return comm_unavailable();
    DeviceGuard g(c->device);  // ncclCommInitRank binds the communicator to the current device
    if (!g.ok) return KSCHED_E_HIP;
    ksched_comm *q = new (std::nothrow) ksched_comm();
    if (!q) return KSCHED_E_NOMEM;
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclResult_t r = api.CommInitRank(&q->comm, nranks, u, rank);
    if (r != ncclSuccess) {
        delete q;
        return comm_fail("ncclCommInitRank", r);
    }
    q->device = c->device;
    q->rank = rank;
    q->nranks = nranks;
    *out = q;
    return KSCHED_OK;
} KSCHED_ABI_CATCH_COMM

int ksched_comm_create_local(ksched_ctx *const *ctxs, int n, ksched_comm **out) try {
    if (!ctxs || !out || n <= 0 || n > 64) return KSCHED_E_INVAL;
    for (int i = 0; i < n; ++i) {
        out[i] = nullptr;
        if (!ctxs[i]) return KSCHED_E_INVAL;
    }
    RcclApi &api = rccl_api();
    if (!api.ok) return comm_unavailable();
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) devs[i] = ctxs[i]->device;
    std::vector<ncclComm_t> comms(n, nullptr);
    ncclResult_t r = api.CommInitAll(comms.data(), n, devs.data());
    if (r != ncclSuccess) return comm_fail("ncclCommInitAll", r);
    for (int i = 0; i < n; ++i) {
        ksched_comm *q = new (std::nothrow) ksched_comm();
        if (!q) {
            for (int j = 0; j < n; ++j) {
                if (j < i) delete out[j];
                out[j] = nullptr;
                (void)api.CommDestroy(comms[j]);
            }
            return KSCHED_E_NOMEM;
        }
        q->comm = comms[i];
        q->device = devs[i];
        q->rank = i;
        q->nranks = n;
        out[i] = q;
    }
    return KSCHED_OK;
} KSCHED_ABI_CATCH_COMM

void ksched_comm_destroy(ksched_comm *q) try {
    if (!q) return;
    RcclApi &api = rccl_api();
    if (api.ok && q->comm) {
        DeviceGuard g(q->device);
        (void)api.CommDestroy(q->comm);
    }
    delete q;
} catch (...) {  // nothing unwinds across the C ABI
}

int ksched_comm_rank(const ksched_comm *q) { return q ? q->rank : -1; }
int ksched_comm_size(const ksched_comm *q) { return q ? q->nranks : 0; }

int ksched_allgather_bindings(ksched_comm *q, const int32_t *local, int32_t *gathered, uint32_t count_per_rank, void *hip_stream) try {
    if (!q || !q->comm) return KSCHED_E_INVAL;
    if (count_per_rank > 0 && (!local || !gathered)) return KSCHED_E_INVAL;
    if (count_per_rank == 0) return KSCHED_OK;
    RcclApi &api = rccl_api();
    if (!api.ok) return comm_unavailable();
    DeviceGuard g(q->device);
    if (!g.ok) return KSCHED_E_HIP;
    ncclResult_t r = api.AllGather(local, gathered, count_per_rank, ncclInt32, q->comm, (hipStream_t)hip_stream);
    return r == ncclSuccess ? KSCHED_OK : comm_fail("ncclAllGather", r);
} KSCHED_ABI_CATCH_COMM

int ksched_allgather_bindings_local(ksched_comm *const *comms, int n, const int32_t *const *local, int32_t *const *gathered,
                                    uint32_t count_per_rank, void *const *hip_streams) try {
    if (!comms || n <= 0 || !local || !gathered) return KSCHED_E_INVAL;
    for (int i = 0; i < n; ++i)
        if (!comms[i] || !comms[i]->comm || (count_per_rank > 0 && (!local[i] || !gathered[i]))) return KSCHED_E_INVAL;
    if (count_per_rank == 0) return KSCHED_OK;
    std::vector<const void *> send(local, local + n);
    std::vector<void *> recv(gathered, gathered + n);
    return group_allgather(comms, n, send.data(), recv.data(), count_per_rank, ncclInt32, hip_streams, "ncclAllGather");
} KSCHED_ABI_CATCH_COMM

}  // extern "C"

// ---- applying a batch's bindings (kernels_build.hpp "ksched_apply_bindings_device") ------------------------------------------------
// Request, plan, launchers: apply_plan.hpp decides what a call does -- the flag verdict, the scratch step, per
// rank the passes of each phase with their grids, per call the all-gathers -- and the functions here execute it.  One ApplyCall per
// rank; the single-ctx call is one rank without a communicator.  With one, each rank passes its own rows of a row-sharded batch, the
// claims and the partial sums are all-gathered between the phases, and the commit merges them.  Everything of one rank rides its
// ctx's change stream; the all-gathers are enqueued there too.  The runner takes each phase through every rank before the collective
// that joins them, so the one-process form issues the per-device calls of a collective together in one group.
namespace {

struct ApplyCall {
    ksched_ctx *c = nullptr;
    ksched_comm *q = nullptr;  // nullptr: the single-ctx call (no collectives)
    hipStream_t hs = nullptr;  // the caller's stream
    uint32_t count = 0;        // the rank's rows
    ApplyRankPlan plan;
    ApplyArgs a{};
    AdmitArgs w{};             // KSCHED_APPLY_WHILE_FIT: what keys and admit take, of `a`
    SnapshotChange chg;        // done when every rank's change has been committed (apply_run)
};

// the admit's arguments from the call's filled ApplyArgs (keys, k0 and idx follow the sort: apply_launch)
AdmitArgs admit_args_of(const ApplyArgs &a) {
    AdmitArgs w{};
    w.bindings = a.bindings;
    w.req_cpu = a.req_cpu;
    w.req_mem = a.req_mem;
    w.ok = a.ok;
    w.status = a.status;
    w.dirty = a.dirty;
    w.ncpu = a.ncpu;
    w.nmem = a.nmem;
    w.nrec = a.nrec;
    w.p = a.p;
    w.n = a.n;
    w.tiles = a.tiles;
    w.gen = a.gen;
    return w;
}

// argument checks of one rank of a sharded call that need no lock and no device
int sharded_check(ksched_ctx *c, ksched_comm *q, uint32_t count, uint32_t row_lo, const int32_t *bindings, const int64_t *req_cpu,
                  const int64_t *req_mem, uint32_t flags) {
    if (!c || !q || !q->comm) return KSCHED_E_INVAL;
    if (int rc = apply_flags_verdict(flags, true)) return rc;
    if (count > 0 && (!bindings || !req_cpu || !req_mem)) return KSCHED_E_INVAL;
    if (!apply_rows_in_range(row_lo, count)) return KSCHED_E_INVAL;
    if (q->device != c->device) return KSCHED_E_INVAL;
    return KSCHED_OK;
}

// the plan's launches of one phase, in order, on the change stream (the ctx's mutex held, its device current)
int apply_launch(ApplyCall &x, int phase) {
    ksched_ctx *c = x.c;
    const hipStream_t s = change_stream(c);
    SortScratch &sc = c->apply.admit_sort;
    for (const ApplyLaunch *l = x.plan.begin(phase); l != x.plan.end(phase); ++l) {
        const dim3 grid(l->grid), block(apply_pass_block(l->pass));
        switch (l->pass) {
        case ApplyPass::kClaim: hipLaunchKernelGGL(k_apply_claim, grid, block, 0, s, x.a); break;
        case ApplyPass::kClaimMerge: hipLaunchKernelGGL(k_apply_claim_merge, grid, block, 0, s, x.a); break;
        case ApplyPass::kAccumulate: hipLaunchKernelGGL(k_apply_accumulate, grid, block, 0, s, x.a); break;
        case ApplyPass::kKeys:  // into set 1, where a SortInto::kScratch plan reads them
            x.w.keys = sc.k0[1].ptr;
            hipLaunchKernelGGL(k_apply_keys, grid, block, 0, s, x.w);
            break;
        case ApplyPass::kSort: {  // (no second key, idx = position = the pod index); the admit reads where the last pass landed
            if (int rc = launch_merge_sort(c, x.plan.sort, sc, SortBuffers{})) return rc;
            const int b = x.plan.sort.landing == SortBuf::kSet1;
            x.w.k0 = sc.k0[b].ptr;
            x.w.idx = sc.idx[b].ptr;
            continue;
        }
        case ApplyPass::kCommitLocal: hipLaunchKernelGGL(k_apply_commit, grid, block, 0, s, x.a); break;
        case ApplyPass::kCommitGathered: hipLaunchKernelGGL(k_apply_commit_gathered, grid, block, 0, s, x.a); break;
        case ApplyPass::kCommitAdmit: hipLaunchKernelGGL(k_apply_admit, grid, block, 0, s, x.w); break;
        case ApplyPass::kReindex:
            if (int rc = launch_build_fit(c, nullptr, 0, c->apply.dirty.ptr)) return rc;
            continue;
        case ApplyPass::kStatus: hipLaunchKernelGGL(k_apply_status, grid, block, 0, s, x.a); break;
        }
        HIPCHK(c, hipGetLastError());
    }
    return KSCHED_OK;
}

// phase 0 (the ctx's mutex held, its device current): plan the rank, order the change, ready the scratch, fill the arguments, claim the
// rank's rows.  Evaluations already enqueued read the snapshot as it was (snapshot_begin); the change also waits for what the caller's
// stream holds (the evaluation that wrote `bindings`, typically).
int apply_begin(ApplyCall &x, const ApplyFacts &f, uint32_t row_lo, const int32_t *bindings, const int64_t *req_cpu,
                const int64_t *req_mem, const uint8_t *ok, int32_t *status_out) {
    ksched_ctx *c = x.c;
    ApplyState &st = c->apply;
    fault_point(c);  // (nothing has changed yet)
    x.plan = plan_apply_rank(f, ApplyRankFacts{x.count, status_out != nullptr, c->idx.built});
    if (x.plan.refused) {  // (the merge passes index records with 32 bits, as bestfit_sort)
        c->last_error = "ksched_apply_bindings_device: KSCHED_APPLY_WHILE_FIT with more than 2^31 pods";
        return KSCHED_E_INVAL;
    }
    if (x.plan.admit) HIPCHK(c, st.reserve_admit(x.plan));  // (BEFORE the change begins: a failed allocation leaves the snapshot as it was)
    if (int rc = x.chg.begin(c)) return rc;
    if (int rc = apply_order_begin(c, x.hs)) return rc;
    HIPCHK(c, st.ready(c->n, change_stream(c)));
    ApplyArgs &a = x.a;
    a.bindings = bindings;
    a.req_cpu = req_cpu;
    a.req_mem = req_mem;
    a.ok = ok;
    a.status = status_out;
    a.acc = st.acc.ptr;
    a.claim = st.claim.ptr;
    a.ovf = st.ovf.ptr;
    a.dirty = st.dirty.ptr;
    a.ncpu = c->ncpu.ptr;
    a.nmem = c->nmem.ptr;
    a.nrec = c->nrec.ptr;
    a.p = x.count;
    a.n = c->n;
    a.tiles = x.plan.tiles;
    a.gen = st.scratch.gen;
    a.first_per_node = (f.flags & KSCHED_APPLY_FIRST_PER_NODE) ? 1u : 0u;
    a.release = (f.flags & KSCHED_APPLY_RELEASE) ? 1u : 0u;
    if (x.q) {
        HIPCHK(c, st.gath.reserve(x.plan.gather_elems));
        a.row_lo = row_lo;
        a.sharded = 1;
        a.gathered = st.gath.ptr;
        a.nranks = (uint32_t)x.q->nranks;
        a.rank = (uint32_t)x.q->rank;
    }
    if (x.plan.admit) x.w = admit_args_of(a);
    return apply_launch(x, 0);
}

// phase 2 (with a communicator, after the partial sums' all-gather): commit, re-index, status; the caller's stream waits for the change
// (the caller reads status_out there) and has then met this generation
int apply_finish(ApplyCall &x) {
    if (int rc = apply_launch(x, 2)) return rc;
    if (int rc = x.chg.commit(Stale::kAvailable)) return rc;
    return apply_order_end(x.c, x.hs);
}

// one grouped all-gather, on the ranks' change streams, of every rank's claims (or sums) into its receive buffer
int apply_allgather(ApplyCall *v, int k, bool claims, size_t count, const char *what) {
    std::vector<ksched_comm *> comms(k);
    std::vector<const void *> send(k);
    std::vector<void *> recv(k), streams(k);
    for (int i = 0; i < k; ++i) {
        comms[i] = v[i].q;
        send[i] = claims ? (const void *)v[i].c->apply.claim.ptr : (const void *)v[i].c->apply.acc.ptr;
        recv[i] = v[i].c->apply.gath.ptr;
        streams[i] = change_stream(v[i].c);
    }
    return group_allgather(comms.data(), k, send.data(), recv.data(), count, ncclUint32, streams.data(), what);
}

// the whole call over the k ranks of `v` (their mutexes held): the phases of every rank, and between them the collectives the plan
// names.  Any failure leaves every ctx that entered the call invalidated (ApplyCall::chg).
int apply_run(ApplyCall *v, int k, const uint32_t *row_lo, const int32_t *const *bindings, const int64_t *const *req_cpu,
              const int64_t *const *req_mem, const uint8_t *const *ok, uint32_t flags, int32_t *const *status_out) {
    ApplyFacts f;
    f.flags = flags;
    f.comm = v[0].q != nullptr;
    f.nranks = f.comm ? (uint32_t)v[0].q->nranks : 1u;
    f.n = v[0].c->n;  // (replicas of one snapshot)
    const ApplyGathers gathers = plan_apply_gathers(f);
    for (int i = 0; i < k; ++i) {
        DeviceGuard g(v[i].c->device);
        if (!g.ok) return KSCHED_E_HIP;
        if (int rc = apply_begin(v[i], f, row_lo[i], bindings[i], req_cpu[i], req_mem[i], ok ? ok[i] : nullptr,
                                 status_out ? status_out[i] : nullptr))
            return rc;
    }
    if (gathers.claims_words)
        if (int rc = apply_allgather(v, k, true, gathers.claims_words, "ncclAllGather (claims)")) return rc;
    for (int i = 0; i < k; ++i) {
        DeviceGuard g(v[i].c->device);
        if (!g.ok) return KSCHED_E_HIP;
        if (int rc = apply_launch(v[i], 1)) return rc;
    }
    if (gathers.sums_words)  // the split sums as 32-bit words: 8 per node
        if (int rc = apply_allgather(v, k, false, gathers.sums_words, "ncclAllGather (sums)")) return rc;
    int rc = KSCHED_OK;
    for (int i = 0; i < k && !rc; ++i) {
        DeviceGuard g(v[i].c->device);
        rc = g.ok ? apply_finish(v[i]) : KSCHED_E_HIP;
    }
    if (rc)  // every replica is invalidated, also a rank whose own change is committed
        for (int i = 0; i < k; ++i) v[i].chg.done = false;
    return rc;
}

}  // namespace

extern "C" {

int ksched_apply_bindings_device(ksched_ctx *c, uint32_t p, const int32_t *bindings, const int64_t *req_cpu, const int64_t *req_mem,
                                 const uint8_t *ok, uint32_t flags, int32_t *status_out, void *hip_stream) try {
    if (!c) return KSCHED_E_INVAL;
    if (int rc = apply_flags_verdict(flags, false)) return rc;
    if (p > 0 && (!bindings || !req_cpu || !req_mem)) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    if (p == 0) return KSCHED_OK;
    const uint32_t row_lo = 0;
    ApplyCall x{c, nullptr, (hipStream_t)hip_stream, p};
    return apply_run(&x, 1, &row_lo, &bindings, &req_cpu, &req_mem, &ok, flags, &status_out);
} KSCHED_ABI_CATCH(c)

int ksched_apply_bindings_sharded(ksched_ctx *c, ksched_comm *q, uint32_t count, uint32_t row_lo, const int32_t *bindings,
                                  const int64_t *req_cpu, const int64_t *req_mem, const uint8_t *ok, uint32_t flags, int32_t *status_out,
                                  void *hip_stream) try {
    if (int rc = sharded_check(c, q, count, row_lo, bindings, req_cpu, req_mem, flags)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    ApplyCall x{c, q, (hipStream_t)hip_stream, count};
    return apply_run(&x, 1, &row_lo, &bindings, &req_cpu, &req_mem, &ok, flags, &status_out);
} KSCHED_ABI_CATCH_COMM

int ksched_apply_bindings_sharded_local(ksched_ctx *const *ctxs, ksched_comm *const *comms, int n, const uint32_t *count,
                                        const uint32_t *row_lo, const int32_t *const *bindings, const int64_t *const *req_cpu,
                                        const int64_t *const *req_mem, const uint8_t *const *ok, uint32_t flags,
                                        int32_t *const *status_out, void *const *hip_streams) try {
    if (!ctxs || !comms || n <= 0 || n > 64 || !count || !row_lo || !bindings || !req_cpu || !req_mem) return KSCHED_E_INVAL;
    for (int i = 0; i < n; ++i) {
        if (int rc = sharded_check(ctxs[i], comms[i], count[i], row_lo[i], bindings[i], req_cpu[i], req_mem[i], flags)) return rc;
        if (comms[i]->nranks != n) return KSCHED_E_INVAL;  // (the collective needs every rank of the clique, each once)
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i] || comms[j] == comms[i] || comms[j]->rank == comms[i]->rank) return KSCHED_E_INVAL;
    }
    // every ctx's mutex, in address order (two calls over the same ctxs in different orders cannot deadlock)
    std::vector<ksched_ctx *> order(ctxs, ctxs + n);
    std::sort(order.begin(), order.end(), std::less<ksched_ctx *>());
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve((size_t)n);
    for (ksched_ctx *c : order) locks.emplace_back(c->mu);
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]->have_nodes) return KSCHED_E_STATE;
    for (int i = 1; i < n; ++i)
        if (ctxs[i]->n != ctxs[0]->n) return KSCHED_E_INVAL;  // replicas of one snapshot
    std::vector<ApplyCall> v((size_t)n);  // (destroyed before the locks are released)
    for (int i = 0; i < n; ++i) {
        v[i].c = ctxs[i];
        v[i].q = comms[i];
        v[i].hs = hip_streams ? (hipStream_t)hip_streams[i] : nullptr;
        v[i].count = count[i];
    }
    return apply_run(v.data(), n, row_lo, bindings, req_cpu, req_mem, ok, flags, status_out);
} KSCHED_ABI_CATCH_COMM

int ksched_index_checksum(ksched_ctx *c, uint64_t *out) try {
    if (!c || !out) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_nodes) return KSCHED_E_STATE;
    out[0] = out[1] = 0;
    if (!c->idx.built) return KSCHED_OK;
    DeviceGuard g(c->device);
    fault_point(c);
    const IndexedLayout &l = c->idx.lay;
    std::vector<uint64_t> tab((size_t)l.tiles * l.rows * kTileWords), aux((size_t)l.tiles * kAuxWords);
    HIPCHK(c, hipEventSynchronize(c->ev_build));  // the latest snapshot change, whichever stream carried it
    HIPCHK(c, hipMemcpy(tab.data(), c->idx.d_tables, tab.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(aux.data(), c->idx.d_aux, aux.size() * 8, hipMemcpyDeviceToHost));
    auto fnv = [](const std::vector<uint64_t> &v) {
        uint64_t h = 0xCBF29CE484222325ull;
        for (uint64_t w : v) {
            h ^= w;
            h *= 0x100000001B3ull;
            h ^= h >> 29;
        }
        return h ? h : 1ull;
    };
    std::vector<uint64_t> lists((size_t)l.tiles * l.nlist * kListBytes / 8);
    if (!lists.empty()) HIPCHK(c, hipMemcpy(lists.data(), c->idx.d_list, lists.size() * 8, hipMemcpyDeviceToHost));
    out[0] = fnv(tab);
    out[1] = fnv(aux) ^ (lists.empty() ? 0ull : fnv(lists) * 0x9E3779B97F4A7C15ull);
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_trace_read(ksched_ctx *c, uint64_t *out, uint32_t max_blocks) try {
    if (!c || !out) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->trace.ptr) return 0;
    DeviceGuard g(c->device);
    HIPCHK(c, hipDeviceSynchronize());
    const uint32_t nb = std::min<uint32_t>(max_blocks, 8192u);
    HIPCHK(c, hipMemcpy(out, c->trace.ptr, (size_t)nb * KSCHED_TRACE_WORDS * 8, hipMemcpyDeviceToHost));
    return (int)nb;
} KSCHED_ABI_CATCH(c)

int ksched_kernel_time_ms(ksched_ctx *c, double *total_ms, uint64_t *launches) try {
    if (!c) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    double tot = 0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        HIPCHK(c, hipEventSynchronize(c->ev_pool[i].b));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].a, c->ev_pool[i].b));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = c->ev_used;
    c->ev_used = 0;
    return KSCHED_OK;
} KSCHED_ABI_CATCH(c)

int ksched_kernel_time_samples(ksched_ctx *c, double *out_ms, uint32_t cap) try {
    if (!c || (cap > 0 && !out_ms)) return KSCHED_E_INVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const size_t n = std::min<size_t>(c->ev_used, cap);
    for (size_t i = 0; i < n; ++i) {
        HIPCHK(c, hipEventSynchronize(c->ev_pool[i].b));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].a, c->ev_pool[i].b));
        out_ms[i] = ms;
    }
    c->ev_used = 0;
    return (int)n;
} KSCHED_ABI_CATCH(c)

}  // extern "C"
