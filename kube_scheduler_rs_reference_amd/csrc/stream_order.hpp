// stream_order.hpp -- every stream wait of a ctx, decided in one place: which stream carries a snapshot change, which streams wait for
// which event before an evaluation, a change or a use of ctx-owned scratch is enqueued, and which events are recorded for that.
//
// Host-only on purpose, like pipe_plan.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/stream_order_tests.cpp runs every sequence of up to five calls through a happens-before model without a GPU.  The
// helpers of ksched_api.hip (stream_enter, scratch_enter, stream_forget, snapshot_begin, snapshot_end, apply_begin / apply_finish)
// ask the questions below, issue exactly the HIP calls the answers name and report back what succeeded; no ordering decision is
// taken anywhere else.  An answer is a small struct of booleans and stream keys; a `plan_*` question changes nothing, and the state
// moves only when the executor says that the call went through (add, met, begin, drop, committed, scratch_taken, forget), so that a
// HIP call that fails leaves the state as it was and the next call asks again (begin names the change stream before the carrier's
// waits are issued: it is read only between a begin that succeeded and its committed).
//
// What is ordered.  The snapshot is built and patched by kernels; evaluations read it on the caller's streams.  No device-wide wait:
// every stream an evaluation was enqueued on is remembered with an event of its own (the executor's `Res`, which also holds the
// stream's other per-stream resources: one registry, one lookup), and with the generation of the snapshot it has waited for.
//   * A snapshot change first makes its stream wait for what the remembered streams hold (evaluations already enqueued read the
//     snapshot as it was), and an evaluation enqueued afterwards makes its stream wait for the change: ev_build, recorded behind
//     every change, whose generation is build_gen.  A stream whose generation is build_gen plans no wait.
//   * Where the change is enqueued: with exactly ONE caller stream known -- one scheduler loop on one stream, the common case -- onto
//     that stream itself: ordered behind the evaluations already there and ahead of the next ones by the stream, with no event and
//     no cross-stream wait at all (each costs ~5 us; on some hardware queues ~180 us, tools/stream_probe.py).  That stream is probed
//     first (a host-side query): a stream the caller destroyed without telling is not used.  Otherwise the ctx's own stream, which
//     catches up with ev_build (an earlier change may have ridden a caller's stream) and then waits for an event recorded on every
//     caller stream, in the order they were first seen; a stream whose record fails was destroyed and is dropped.
//     KSCHED_OPT_SNAPSHOT_STREAM = 1 keeps every change on the ctx's own stream.
//   * An apply (ksched_apply_bindings_*) is a change that also waits for what its caller's stream `hs` holds (ev_apply, recorded
//     there), and `hs` waits for ev_build behind it -- both only when the change rides another stream than `hs`.
//   * The ctx-owned device scratch that evaluations use (the best-fit hand-over, the scratch mask, the summary's partial counts, the
//     trace) belongs to one stream at a time: when another stream is about to use it, ev_scratch is recorded on the owner and the
//     newcomer waits for it (nothing on the common one-stream path).  A forgotten owner's last use stays ordered as a pending
//     record of ev_scratch, which the next user waits for once.
//
// The invariants (tests/cpp/stream_order_tests.cpp asks every sequence for them):
//   I1. an evaluation enqueued after change k runs after change k;
//   I2. an evaluation enqueued before change k, on any stream the ctx knows, runs before it;
//   I3. changes run in the order of their calls;
//   I4. successive uses of the scratch are ordered;
//   I5. what `hs` held before an apply runs before the apply's change;
//   I6. what is enqueued on `hs` after the apply runs after the change;
//   I7. after ksched_forget_stream, or after a failed probe or record, no answer names that stream until an evaluation enters it again.
// Two sequences are known NOT to hold (the test lists them by name as expected):
//   * I2: work left on the ctx's own stream with no host wait (ksched_eval_begin), then a change that rides the one caller stream: that
//     stream does not wait for the own stream;
//   * I7: a stream destroyed without notice while it owns the scratch stays the owner (only forget hands the scratch over): the next
//     use on another stream is told to record on it, and that record fails.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ksched {

using StreamKey = const void *;  // a hipStream_t to the executor; opaque here (NULL, the default stream, is a caller stream like any other)

// an evaluation is about to be enqueued on `s` (plan_enter)
struct EnterPlan {
    bool is_new = false;      // not known yet: create its event and add() it
    bool wait_build = false;  // `s` waits for ev_build, then met(s)
};
// a snapshot change begins (plan_probe, then begin with the probe's answer)
struct ProbePlan {
    bool probe = false;  // query `stream` on the host first: is it still alive?
    StreamKey stream = nullptr;
};
struct BeginPlan {
    StreamKey carrier = nullptr;       // the change is enqueued here
    bool carrier_waits_build = false;  // first it waits for ev_build, then met(carrier)
    bool record_callers = false;       // then, for caller(0) .. caller(callers() - 1): record its event on it, the carrier waits for that; failed: drop(i)
};
// an apply whose caller stream is `hs`, between begin and committed (plan_apply)
struct ApplyPlan {
    bool change_waits_hs = false;  // before the change: ev_apply recorded on `hs`, the carrier waits for it
    bool hs_waits_change = false;  // after committed(): `hs` waits for ev_build, then met(hs)
};
// work on `s` is about to use the ctx-owned scratch (plan_scratch; scratch_taken(s) when the calls went through)
enum class ScratchStep { kNothing, kRecordOwnerAndWait, kWaitPending };
struct ScratchPlan {
    ScratchStep step = ScratchStep::kNothing;  // kRecordOwnerAndWait: ev_scratch recorded on `owner`, `s` waits for it; kWaitPending: `s` waits for ev_scratch
    StreamKey owner = nullptr;
};
// `s` is forgotten (plan_forget, then forget with the record's outcome)
struct ForgetPlan {
    bool record_scratch = false;  // `s` owns the scratch: record ev_scratch on it
};

// Res: what the executor keeps per stream (its event, its per-stream buffers); moved, never looked at.
template <class Res>
class StreamOrder {
public:
    void set_own_stream(StreamKey s) { own_.s = change_ = s; }
    void set_opt_own_stream(bool on) { opt_own_stream_ = on; }  // KSCHED_OPT_SNAPSHOT_STREAM = 1
    StreamKey change_stream() const { return change_; }        // where the change in progress is enqueued (begin decides)

    // the per-stream resources of `s`: the own stream's, a known caller stream's, or null
    Res *res(StreamKey s) {
        Entry *e = find(s);
        return e ? &e->res : nullptr;
    }

    EnterPlan plan_enter(StreamKey s) const {
        const Entry *e = find(s);
        return EnterPlan{!e, (e ? e->gen : 0u) != build_gen_};  // (the own stream: in order by itself unless the latest change rode a caller's stream)
    }
    void add(StreamKey s, Res &&r) { callers_.push_back(Entry{s, 0, std::move(r)}); }
    // `s` has met the latest change: it carried it, or has just been made to wait for ev_build (a stream the ctx does not know has no generation to keep)
    void met(StreamKey s) {
        if (Entry *e = find(s)) e->gen = build_gen_;
    }

    ProbePlan plan_probe() const {
        const bool one = callers_.size() == 1 && !opt_own_stream_;
        return ProbePlan{one, one ? callers_[0].s : nullptr};
    }
    // alive: the probe's answer (ignored where plan_probe asked for none)
    BeginPlan begin(bool alive) {
        if (plan_probe().probe && alive) {  // (an earlier change may have gone onto the ctx's stream, and this stream not have met it yet)
            change_ = callers_[0].s;
            return BeginPlan{change_, callers_[0].gen != build_gen_, false};
        }
        change_ = own_.s;  // (a probe that failed: the record on that stream fails as well, and drops it)
        return BeginPlan{change_, own_.gen != build_gen_, true};
    }
    size_t callers() const { return callers_.size(); }
    StreamKey caller(size_t i) const { return callers_[i].s; }
    Res &caller_res(size_t i) { return callers_[i].res; }
    Res drop(size_t i) {  // the record on caller(i) failed: the caller destroyed that stream
        Res r = std::move(callers_[i].res);
        callers_.erase(callers_.begin() + (std::ptrdiff_t)i);
        return r;
    }
    // ev_build has been recorded on change_stream(), behind the change: the carrier is behind it by itself
    void committed() {
        ++build_gen_;
        met(change_);
    }

    ApplyPlan plan_apply(StreamKey hs) const { return ApplyPlan{change_ != hs, change_ != hs}; }

    ScratchPlan plan_scratch(StreamKey s) const {
        if (scratch_owned_ && scratch_stream_ != s) return ScratchPlan{ScratchStep::kRecordOwnerAndWait, scratch_stream_};
        if (!scratch_owned_ && scratch_ev_pending_) return ScratchPlan{ScratchStep::kWaitPending, nullptr};
        return ScratchPlan{};
    }
    void scratch_taken(StreamKey s) {
        scratch_stream_ = s;
        scratch_owned_ = true;
        scratch_ev_pending_ = false;
    }

    ForgetPlan plan_forget(StreamKey s) const { return ForgetPlan{scratch_owned_ && scratch_stream_ == s}; }
    // recorded: whether the record plan_forget asked for went through (if not, nothing is pending).  True with the stream's resources
    // in *out when `s` was a known caller stream; the own stream keeps its entry.
    bool forget(StreamKey s, bool recorded, Res *out) {
        if (plan_forget(s).record_scratch) {  // its last use of the scratch stays ordered: as an event
            scratch_ev_pending_ = recorded;
            scratch_owned_ = false;
            scratch_stream_ = nullptr;
        }
        for (size_t i = 0; i < callers_.size(); ++i)
            if (callers_[i].s == s) {
                *out = drop(i);
                return true;
            }
        return false;
    }

private:
    struct Entry {
        StreamKey s;
        uint64_t gen;  // snapshot generation this stream has waited for
        Res res;
    };
    Entry *find(StreamKey s) {
        if (s == own_.s) return &own_;
        for (auto &e : callers_)
            if (e.s == s) return &e;
        return nullptr;
    }
    const Entry *find(StreamKey s) const { return const_cast<StreamOrder *>(this)->find(s); }

    Entry own_{nullptr, 0, Res{}};  // the ctx's own stream
    std::vector<Entry> callers_;    // the caller streams evaluations were enqueued on, in the order they were first seen
    uint64_t build_gen_ = 0;        // generation of the latest committed change (ev_build's latest record)
    StreamKey change_ = nullptr;
    bool opt_own_stream_ = false;
    StreamKey scratch_stream_ = nullptr;
    bool scratch_owned_ = false, scratch_ev_pending_ = false;
};

}  // namespace ksched
