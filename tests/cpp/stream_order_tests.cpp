// stream_order_tests.cpp -- host-side check of the ctx's stream ordering (csrc/stream_order.hpp), no GPU and no HIP.
//
// (a) A happens-before model of what the answers are executed on: a stream is in order, a record snapshots what its stream has seen, a
//     wait joins the event's latest record at the time the wait is enqueued.  Every sequence of up to five calls runs through it and is
//     asked the invariants I1 .. I7 of stream_order.hpp.  What breaks one must be a hole listed in g_holes, by name.
// (b) The rules as ksched_api.hip had them before the header, transcribed literally over a fake ctx (OldCtx): the same sequences, and
//     every call must issue the same event and stream calls in the same order, with the same outcome.
// (c) The steady states, written out call by call, and the hot path's allocations counted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../kube_scheduler_rs_reference_amd/csrc/stream_order.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

// every allocation of the program is counted: the hot path must make none
static long g_allocs = 0;
void *operator new(size_t n) {
    ++g_allocs;
    if (void *p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void operator delete(void *p) noexcept { std::free(p); }
void operator delete(void *p, size_t) noexcept { std::free(p); }

// ---- the streams, the events and the fake runtime both executors call ------------------------------------------------------------
// kX: a stream the ctx never sees an evaluation on (an apply's caller stream)
constexpr int kOwn = 0, kA = 1, kB = 2, kX = 3, kStreams = 4;
constexpr int kEvBuild = 0, kEvApply = 1, kEvScratch = 2, kEvOf = 3, kEvents = kEvOf + kStreams;  // kEvOf + s: the event of caller stream s
static const char *const kStreamName[kStreams] = {"own", "A", "B", "X"};
static const char *const kEventName[kEvents] = {"ev_build", "ev_apply", "ev_scratch", "ev[own]", "ev[A]", "ev[B]", "ev[X]"};
static char g_stream_storage[kStreams];
static StreamKey key(int s) { return &g_stream_storage[s]; }
static int stream_of(StreamKey k) { return (int)((const char *)k - g_stream_storage); }

struct Call {
    char op;  // C create, Q query, R record, W wait, D destroy
    int8_t stream, ev;
    bool ok;
    bool operator==(const Call &o) const { return op == o.op && stream == o.stream && ev == o.ev && ok == o.ok; }
};

// A piece of device work is a bit; seen[s] is the set of pieces that have run once everything enqueued on stream s so far has.
struct Hw {
    uint32_t seen[kStreams] = {};
    uint32_t ev[kEvents] = {};     // what the latest record of each event saw (never recorded: nothing, a wait for it is a no-op)
    bool dead[kStreams] = {};      // destroyed by the caller without notice: queries and records on it fail
    Call log[24];                  // the calls of the current step
    int n = 0;
    void note(char op, int s, int e, bool ok) {
        if (n < 24) log[n] = Call{op, (int8_t)s, (int8_t)e, ok};
        ++n;
    }
    bool create(int e) {
        ev[e] = 0;
        note('C', -1, e, true);
        return true;
    }
    void destroy(int e) { note('D', -1, e, true); }
    bool query(int s) {
        note('Q', s, -1, !dead[s]);
        return !dead[s];
    }
    bool record(int e, int s) {
        if (!dead[s]) ev[e] = seen[s];
        note('R', s, e, !dead[s]);
        return !dead[s];
    }
    bool wait(int s, int e) {
        seen[s] |= ev[e];
        note('W', s, e, true);
        return true;
    }
    void launch(int s, uint32_t piece) { seen[s] |= piece; }
    std::string trace() const {
        std::string t;
        for (int i = 0; i < n && i < 24; ++i) {
            const Call &c = log[i];
            if (!t.empty()) t += ' ';
            switch (c.op) {
                case 'C': t += std::string("create(") + kEventName[c.ev] + ")"; break;
                case 'D': t += std::string("destroy(") + kEventName[c.ev] + ")"; break;
                case 'Q': t += std::string("query(") + kStreamName[c.stream] + ")"; break;
                case 'R': t += std::string("record(") + kEventName[c.ev] + "," + kStreamName[c.stream] + ")"; break;
                default: t += std::string("wait(") + kStreamName[c.stream] + "," + kEventName[c.ev] + ")";
            }
            if (!c.ok) t += '!';
        }
        return t;
    }
};

#define HWCHK(call)            \
    do {                       \
        if (!(call)) return 1; \
    } while (0)

// ---- the executors of the header's answers, as ksched_api.hip has them ----------------------------------------------------------------
struct Res {
    int ev = -1;
};

struct NewWorld {
    Hw hw;
    StreamOrder<Res> o;
    bool ev_apply = false;
    NewWorld() { o.set_own_stream(key(kOwn)); }

    int wait_build(int s) {
        HWCHK(hw.wait(s, kEvBuild));
        o.met(key(s));
        return 0;
    }
    int enter(int s) {
        const EnterPlan pl = o.plan_enter(key(s));
        if (pl.is_new) {
            Res r;
            r.ev = kEvOf + s;
            HWCHK(hw.create(r.ev));
            o.add(key(s), std::move(r));
        }
        return pl.wait_build ? wait_build(s) : 0;
    }
    int scratch(int s) {
        const ScratchPlan pl = o.plan_scratch(key(s));
        if (pl.step == ScratchStep::kRecordOwnerAndWait) HWCHK(hw.record(kEvScratch, stream_of(pl.owner)));
        if (pl.step != ScratchStep::kNothing) HWCHK(hw.wait(s, kEvScratch));
        o.scratch_taken(key(s));
        return 0;
    }
    void forget(int s) {
        bool recorded = false;
        if (o.plan_forget(key(s)).record_scratch) recorded = hw.record(kEvScratch, s);
        Res gone;
        if (o.forget(key(s), recorded, &gone)) hw.destroy(gone.ev);
    }
    int begin() {
        const ProbePlan pr = o.plan_probe();
        bool alive = false;
        if (pr.probe) alive = hw.query(stream_of(pr.stream));
        const BeginPlan pl = o.begin(alive);
        const int s = stream_of(pl.carrier);
        if (pl.carrier_waits_build)
            if (int rc = wait_build(s)) return rc;
        if (!pl.record_callers) return 0;
        for (size_t i = 0; i < o.callers();) {
            if (!hw.record(o.caller_res(i).ev, stream_of(o.caller(i)))) {
                const Res gone = o.drop(i);
                hw.destroy(gone.ev);
                continue;
            }
            HWCHK(hw.wait(s, o.caller_res(i).ev));
            ++i;
        }
        return 0;
    }
    int end() {
        HWCHK(hw.record(kEvBuild, change_stream()));
        o.committed();
        return 0;
    }
    int apply_begin(int hs) {
        if (!o.plan_apply(key(hs)).change_waits_hs) return 0;
        if (!ev_apply) {
            HWCHK(hw.create(kEvApply));
            ev_apply = true;
        }
        HWCHK(hw.record(kEvApply, hs));
        HWCHK(hw.wait(change_stream(), kEvApply));
        return 0;
    }
    int apply_end(int hs) { return o.plan_apply(key(hs)).hs_waits_change ? wait_build(hs) : 0; }
    void set_opt(bool on) { o.set_opt_own_stream(on); }
    int change_stream() const { return stream_of(o.change_stream()); }
};

// ---- (b) the rules as they were: ksched_api.hip's functions before stream_order.hpp, line for line ----------------------------------------
// (a stream is its index, no stream -1; a HIP call is the fake runtime's; the per-stream pick accumulators, which order nothing, are left out)
struct OldCtx {
    Hw hw;
    int stream = kOwn;
    bool ev_apply = false;
    struct UserStream {
        int s;
        int ev;
        uint64_t gen;
    };
    std::vector<UserStream> user_streams;
    uint64_t build_gen = 0;
    int change_stream = kOwn;
    uint64_t own_gen = 0;
    bool opt_own_stream = false;
    int scratch_stream = -1;
    bool scratch_owned = false, scratch_ev_pending = false;
};

static int stream_catch_up(OldCtx *c, int s, uint64_t &gen) {
    if (gen != c->build_gen) {
        HWCHK(c->hw.wait(s, kEvBuild));
        gen = c->build_gen;
    }
    return 0;
}

static void stream_met(OldCtx *c, int s) {
    if (s == c->stream) c->own_gen = c->build_gen;
    for (auto &u : c->user_streams)
        if (u.s == s) u.gen = c->build_gen;
}

static int stream_enter(OldCtx *c, int s) {
    if (s == c->stream) return stream_catch_up(c, s, c->own_gen);
    OldCtx::UserStream *u = nullptr;
    for (auto &x : c->user_streams)
        if (x.s == s) u = &x;
    if (!u) {
        OldCtx::UserStream n{s, kEvOf + s, 0};
        HWCHK(c->hw.create(n.ev));
        c->user_streams.push_back(n);
        u = &c->user_streams.back();
    }
    return stream_catch_up(c, s, u->gen);
}

static int scratch_enter(OldCtx *c, int s) {
    if (c->scratch_owned && c->scratch_stream != s) {
        HWCHK(c->hw.record(kEvScratch, c->scratch_stream));
        HWCHK(c->hw.wait(s, kEvScratch));
    } else if (!c->scratch_owned && c->scratch_ev_pending) {
        HWCHK(c->hw.wait(s, kEvScratch));
    }
    c->scratch_stream = s;
    c->scratch_owned = true;
    c->scratch_ev_pending = false;
    return 0;
}

static void stream_forget(OldCtx *c, int s) {
    if (c->scratch_owned && c->scratch_stream == s) {
        c->scratch_ev_pending = c->hw.record(kEvScratch, s);
        c->scratch_owned = false;
        c->scratch_stream = -1;
    }
    for (size_t i = 0; i < c->user_streams.size(); ++i)
        if (c->user_streams[i].s == s) {
            c->hw.destroy(c->user_streams[i].ev);
            c->user_streams.erase(c->user_streams.begin() + (std::ptrdiff_t)i);
            return;
        }
}

static int snapshot_begin(OldCtx *c) {
    c->change_stream = c->stream;
    if (c->user_streams.size() == 1 && !c->opt_own_stream) {
        auto &u = c->user_streams[0];
        if (c->hw.query(u.s)) {
            if (int rc = stream_catch_up(c, u.s, u.gen)) return rc;
            c->change_stream = u.s;
            return 0;
        }
    }
    if (int rc = stream_catch_up(c, c->stream, c->own_gen)) return rc;
    for (size_t i = 0; i < c->user_streams.size();) {
        auto &u = c->user_streams[i];
        if (!c->hw.record(u.ev, u.s)) {
            c->hw.destroy(u.ev);
            c->user_streams.erase(c->user_streams.begin() + (std::ptrdiff_t)i);
            continue;
        }
        HWCHK(c->hw.wait(c->stream, u.ev));
        ++i;
    }
    return 0;
}

static int snapshot_end(OldCtx *c) {
    HWCHK(c->hw.record(kEvBuild, c->change_stream));
    ++c->build_gen;
    stream_met(c, c->change_stream);
    return 0;
}

// apply_begin, behind SnapshotChange::begin
static int old_apply_begin(OldCtx *c, int hs) {
    const int s = c->change_stream;
    if (s != hs) {
        if (!c->ev_apply) {
            HWCHK(c->hw.create(kEvApply));
            c->ev_apply = true;
        }
        HWCHK(c->hw.record(kEvApply, hs));
        HWCHK(c->hw.wait(s, kEvApply));
    }
    return 0;
}

// apply_finish, behind SnapshotChange::commit
static int old_apply_finish(OldCtx *c, int hs) {
    const int s = c->change_stream;
    if (s != hs) {
        HWCHK(c->hw.wait(hs, kEvBuild));
        stream_met(c, hs);
    }
    return 0;
}

struct OldWorld {
    OldCtx c;
    Hw &hw;
    OldWorld() : hw(c.hw) {}
    OldWorld(const OldWorld &w) : c(w.c), hw(c.hw) {}
    OldWorld &operator=(const OldWorld &w) {
        c = w.c;
        return *this;
    }
    int enter(int s) { return stream_enter(&c, s); }
    int scratch(int s) { return scratch_enter(&c, s); }
    void forget(int s) { stream_forget(&c, s); }
    int begin() { return snapshot_begin(&c); }
    int end() { return snapshot_end(&c); }
    int apply_begin(int hs) { return old_apply_begin(&c, hs); }
    int apply_end(int hs) { return old_apply_finish(&c, hs); }
    void set_opt(bool on) { c.opt_own_stream = on; }
    int change_stream() const { return c.change_stream; }
};

// ---- the calls of a sequence, and what each is asked ----------------------------------------------------------------------------------
enum OpKind { kEval, kEvalScratch, kChange, kApply, kRebuildEval, kForget, kDestroy, kToggleOpt };
struct Op {
    OpKind kind;
    int s;
    const char *name;
};
static const Op kOps[] = {
    {kEval, kOwn, "eval(own)"},
    {kEval, kA, "eval(A)"},
    {kEval, kB, "eval(B)"},
    {kEvalScratch, kOwn, "eval+scratch(own)"},
    {kEvalScratch, kA, "eval+scratch(A)"},
    {kEvalScratch, kB, "eval+scratch(B)"},
    {kChange, -1, "set"},
    {kChange, -1, "update"},
    {kApply, kOwn, "apply(own)"},
    {kApply, kA, "apply(A)"},
    {kApply, kB, "apply(B)"},
    {kApply, kX, "apply(X)"},
    {kRebuildEval, kOwn, "rebuild+eval(own)"},  // ensure_bestfit's change in front of a PICK_BESTFIT evaluation
    {kRebuildEval, kA, "rebuild+eval(A)"},
    {kRebuildEval, kB, "rebuild+eval(B)"},
    {kForget, kA, "forget(A)"},
    {kDestroy, kA, "destroy(A)"},  // by the caller, without ksched_forget_stream
    {kToggleOpt, -1, "option"},    // KSCHED_OPT_SNAPSHOT_STREAM 0 <-> 1
};
constexpr int kNumOps = (int)(sizeof kOps / sizeof kOps[0]);
constexpr int kMaxOps = 5;

// the caller does not use a stream it has destroyed
static bool valid(const Op &op, bool a_dead) { return !(a_dead && op.s == kA && op.kind != kForget); }

constexpr unsigned I1 = 1u, I2 = 2u, I3 = 4u, I4 = 8u, I5 = 16u, I6 = 32u, I7 = 64u;

// What today's rules leave open, by name.  A fix of one flips its `expected_unordered` to false: from then on a
// sequence that shows it fails the test.
struct KnownHole {
    const char *name;
    unsigned invariant;
    bool expected_unordered;
    long hits;
};
enum { kHoleOwnWorkThenRidingChange, kHoleDestroyedScratchOwner, kNumHoles };
static KnownHole g_holes[kNumHoles] = {
    // work left on the ctx's own stream (ksched_eval_begin: no host wait), then a change that rides the one caller stream: that stream
    // does not wait for the own stream
    {"own_stream_work_then_change_rides_the_caller_stream", I2, true, 0},
    // a stream destroyed without notice while it owns the scratch stays the owner after a change has dropped it: the next use of the
    // scratch on another stream records on it, which fails (the evaluation returns the error)
    {"destroyed_scratch_owner_is_recorded_on_again", I7, true, 0},
};

struct StepResult {
    unsigned broken = 0;      // invariants this step breaks
    unsigned unexpected = 0;  // of those, the ones outside every expected hole
    int rc = 0;               // the call failed (a HIP call did): nothing of it was enqueued behind the failing call
};

template <class W>
struct Run {
    W w;
    bool tally_holes = true;  // (the old rules' run shows the same holes: counted once)
    bool opt = false;
    int pieces = 0;
    uint32_t changes = 0;             // every change so far
    uint32_t evals_on[kStreams] = {};  // the evaluations on each stream the ctx knows (forgotten or destroyed: none, the ctx cannot order them)
    uint32_t last_scratch = 0;        // the latest use of the scratch
    int last_scratch_stream = -1;
    bool banned[kStreams] = {};  // I7: forgotten, or failed a probe or record of snapshot_begin; until an evaluation enters it again

    uint32_t piece() { return 1u << pieces++; }

    void hole(StepResult &r, unsigned inv, int which) {
        r.broken |= inv;
        if (which >= 0 && g_holes[which].expected_unordered) g_holes[which].hits += tally_holes;
        else r.unexpected |= inv;
    }

    void eval(int s, bool scratch, StepResult &r) {
        Hw &hw = w.hw;
        if (w.enter(s) || (scratch && w.scratch(s))) {
            r.rc = 1;
            return;
        }
        const uint32_t e = piece();
        if ((hw.seen[s] & changes) != changes) hole(r, I1, -1);
        if (scratch) {
            if (last_scratch && !hw.dead[last_scratch_stream] && !(hw.seen[s] & last_scratch)) hole(r, I4, -1);
            last_scratch = e;
            last_scratch_stream = s;
        }
        hw.launch(s, e);
        evals_on[s] |= e;
    }

    // hs >= 0: an apply whose caller stream is hs
    void change(int hs, StepResult &r) {
        Hw &hw = w.hw;
        uint32_t before = 0;
        if (hs >= 0) hw.launch(hs, before = piece());  // what the caller's stream holds (the evaluation that wrote the bindings)
        if (w.begin() || (hs >= 0 && w.apply_begin(hs))) {
            r.rc = 1;
            return;
        }
        const int cs = w.change_stream();
        const uint32_t c = piece();
        uint32_t known = 0;
        for (int s = 0; s < kStreams; ++s) known |= evals_on[s];
        if (const uint32_t missing = known & ~hw.seen[cs])
            hole(r, I2, cs != kOwn && !(missing & ~evals_on[kOwn]) ? kHoleOwnWorkThenRidingChange : -1);
        if ((hw.seen[cs] & changes) != changes) hole(r, I3, -1);
        if (before && !(hw.seen[cs] & before)) hole(r, I5, -1);
        hw.launch(cs, c);
        changes |= c;
        if (w.end() || (hs >= 0 && w.apply_end(hs))) {
            r.rc = 1;
            return;
        }
        if (hs >= 0) {
            if (!(hw.seen[hs] & c)) hole(r, I6, -1);
            hw.launch(hs, piece());  // the caller reads status_out there
        }
    }

    StepResult step(const Op &op) {
        Hw &hw = w.hw;
        StepResult r;
        hw.n = 0;
        if (op.kind == kEval || op.kind == kEvalScratch || op.kind == kRebuildEval) banned[op.s] = false;
        bool was_banned[kStreams];
        std::memcpy(was_banned, banned, sizeof banned);
        switch (op.kind) {
            case kEval: eval(op.s, false, r); break;
            case kEvalScratch: eval(op.s, true, r); break;
            case kChange: change(-1, r); break;
            case kApply: change(op.s, r); break;
            case kRebuildEval:
                change(-1, r);
                if (!r.rc) eval(op.s, false, r);
                break;
            case kForget:
                w.forget(op.s);
                evals_on[op.s] = 0;
                banned[op.s] = true;
                break;
            case kDestroy:
                hw.dead[op.s] = true;
                evals_on[op.s] = 0;
                break;
            case kToggleOpt: w.set_opt(opt = !opt); break;
        }
        CHECK(hw.n <= 24);
        for (int i = 0; i < hw.n && i < 24; ++i) {
            const Call &c = hw.log[i];
            const int named = c.stream >= 0 ? c.stream : c.ev >= kEvOf ? c.ev - kEvOf : -1;
            if (named >= 0 && named != op.s && was_banned[named])  // (the stream a call is handed is the caller's to name)
                hole(r, I7, c.op == 'R' && c.ev == kEvScratch && hw.dead[named] ? kHoleDestroyedScratchOwner : -1);
            if (!c.ok && (c.op == 'Q' || (c.op == 'R' && c.ev >= kEvOf))) banned[c.stream] = true;  // snapshot_begin's probe, or its record
        }
        return r;
    }
};

// ---- (a) + (b): every sequence ------------------------------------------------------------------------------------------------------
struct Node {
    Run<NewWorld> now;
    Run<OldWorld> old;
    bool a_dead = false;
};

struct Tally {
    long sequences = 0, breaking = 0, unexpected = 0, differing = 0, failed_calls = 0;
    unsigned broken = 0;
    int path[kMaxOps];
};

static void print_path(const char *what, const Tally &t, int len) {
    std::printf("%s:", what);
    for (int i = 0; i < len; ++i) std::printf(" %s", kOps[t.path[i]].name);
    std::printf("\n");
}

static void walk(const Node &node, int depth, bool broke_before, Tally &t) {
    for (int k = 0; k < kNumOps; ++k) {
        const Op &op = kOps[k];
        if (!valid(op, node.a_dead)) continue;
        Node next = node;
        t.path[depth] = k;
        const StepResult ro = next.old.step(op);
        const StepResult rn = next.now.step(op);
        if (op.kind == kDestroy) next.a_dead = true;
        ++t.sequences;
        // (b) the same calls, in the same order, with the same outcome
        const Hw &a = next.now.w.hw, &b = next.old.w.hw;
        bool same = a.n == b.n && rn.rc == ro.rc && rn.broken == ro.broken && next.now.w.change_stream() == next.old.w.change_stream();
        for (int i = 0; same && i < a.n && i < 24; ++i) same = a.log[i] == b.log[i];
        if (!same && ++t.differing <= 5) {
            print_path("the header and the old rules differ", t, depth + 1);
            std::printf("  header:    %s\n  old rules: %s\n", a.trace().c_str(), b.trace().c_str());
        }
        // (a) the invariants
        const bool broke = broke_before || rn.broken;
        if (broke) ++t.breaking;
        t.broken |= rn.broken;
        if (rn.rc) ++t.failed_calls;
        if (rn.unexpected && ++t.unexpected <= 5) {
            print_path("breaks an invariant outside the known holes", t, depth + 1);
            std::printf("  mask 0x%x, calls: %s\n", rn.unexpected, a.trace().c_str());
        }
        if (depth + 1 < kMaxOps) walk(next, depth + 1, broke, t);
    }
}

// sequences of exactly `len` more calls, counted without running them
static long count_valid(int len, bool a_dead) {
    if (len == 0) return 1;
    long n = 0;
    for (int k = 0; k < kNumOps; ++k)
        if (valid(kOps[k], a_dead)) n += count_valid(len - 1, a_dead || kOps[k].kind == kDestroy);
    return n;
}

static void every_sequence_of_up_to_five_calls() {
    Tally t;
    Node root;
    root.old.tally_holes = false;
    walk(root, 0, false, t);
    long expect = 0;
    for (int len = 1; len <= kMaxOps; ++len) expect += count_valid(len, false);
    std::printf("stream_order: %ld sequences of up to %d calls out of %d; %ld differ from the old rules; %ld break an invariant (mask 0x%x), %ld outside the known holes; "
                "%ld calls returned an error\n",
                t.sequences, kMaxOps, kNumOps, t.differing, t.breaking, t.broken, t.unexpected, t.failed_calls);
    CHECK(t.sequences == expect && t.sequences > 1000000);
    CHECK(t.differing == 0);
    CHECK(t.unexpected == 0);
    unsigned allowed = 0;
    for (const auto &h : g_holes) {
        std::printf("  known hole %s (I%d): %s, shown %ld times\n", h.name, h.invariant == I2 ? 2 : 7, h.expected_unordered ? "expected" : "fixed", h.hits);
        if (h.expected_unordered) {
            CHECK(h.hits > 0);  // (a hole that no sequence shows any more is to be struck from the list)
            allowed |= h.invariant;
        }
    }
    CHECK((t.broken & ~allowed) == 0);
}

// ---- (c) the steady states, call by call ----------------------------------------------------------------------------------------------
struct Script {
    Run<NewWorld> run;
    StepResult last;
    // the calls `name` issues
    std::string operator()(const char *name) {
        for (const Op &op : kOps)
            if (!std::strcmp(op.name, name)) {
                last = run.step(op);
                return run.w.hw.trace();
            }
        CHECK(!"unknown call");
        return "?";
    }
};

static void the_one_stream_loop_needs_no_wait() {
    Script s;
    CHECK(s("eval(A)") == "create(ev[A])");
    for (int i = 0; i < 3; ++i) {
        // the change rides A: the host-side probe, and ev_build recorded behind it for whoever comes later; no wait, no caller event
        CHECK(s("update") == "query(A) record(ev_build,A)");
        CHECK(s.run.w.change_stream() == kA);
        CHECK(s("eval(A)") == "" && s.last.broken == 0);
        CHECK(s("eval+scratch(A)") == "");
        CHECK(s("rebuild+eval(A)") == "query(A) record(ev_build,A)");
    }
    // no caller stream at all: the own stream, in order by itself
    Script t;
    CHECK(t("set") == "record(ev_build,own)" && t("eval(own)") == "" && t("update") == "record(ev_build,own)" && t("eval+scratch(own)") == "");
}

static void two_caller_streams() {
    Script s;
    CHECK(s("eval(A)") == "create(ev[A])" && s("eval(B)") == "create(ev[B])");
    for (int i = 0; i < 2; ++i) {
        CHECK(s("update") == "record(ev[A],A) wait(own,ev[A]) record(ev[B],B) wait(own,ev[B]) record(ev_build,own)");
        CHECK(s.run.w.change_stream() == kOwn);
        CHECK(s("eval(B)") == "wait(B,ev_build)" && s("eval(A)") == "wait(A,ev_build)");
        CHECK(s("eval(A)") == "" && s("eval(B)") == "");
    }
    // the scratch changes hands with one record and one wait, and only then
    CHECK(s("eval+scratch(A)") == "" && s("eval+scratch(A)") == "");
    CHECK(s("eval+scratch(B)") == "record(ev_scratch,A) wait(B,ev_scratch)" && s("eval+scratch(B)") == "");
    CHECK(s("eval+scratch(own)") == "record(ev_scratch,B) wait(own,ev_scratch)");
}

static void the_option_keeps_changes_on_the_own_stream() {
    Script s;
    CHECK(s("eval(A)") == "create(ev[A])" && s("option") == "");
    for (int i = 0; i < 2; ++i) {
        CHECK(s("update") == "record(ev[A],A) wait(own,ev[A]) record(ev_build,own)");
        CHECK(s("eval(A)") == "wait(A,ev_build)" && s("eval(A)") == "");
    }
    // back at 0 the next change rides A again, which has met the latest change: no wait
    CHECK(s("option") == "" && s("update") == "query(A) record(ev_build,A)");
    // and a change on the own stream after one that rode A first catches up with it
    CHECK(s("option") == "" && s("update") == "wait(own,ev_build) record(ev[A],A) wait(own,ev[A]) record(ev_build,own)");
}

static void the_first_evaluation_on_a_stream_after_a_change_that_rode_another() {
    Script s;
    CHECK(s("eval(A)") == "create(ev[A])" && s("update") == "query(A) record(ev_build,A)");
    CHECK(s("eval(B)") == "create(ev[B]) wait(B,ev_build)" && s("eval(B)") == "");
    CHECK(s("eval(own)") == "wait(own,ev_build)" && s("eval(own)") == "");
    // two caller streams now: the own stream carries the next change, and has met the previous one already
    CHECK(s("update") == "record(ev[A],A) wait(own,ev[A]) record(ev[B],B) wait(own,ev[B]) record(ev_build,own)");
    // a caller stream that the ctx meets only after a change on the own stream, then carries the next one behind it
    Script t;
    CHECK(t("set") == "record(ev_build,own)" && t("eval(A)") == "create(ev[A]) wait(A,ev_build)");
    CHECK(t("update") == "query(A) record(ev_build,A)");
    Script u;  // ... or carries it at once, when it has not met that change yet
    CHECK(u("eval(A)") == "create(ev[A])" && u("option") == "" && u("update") == "record(ev[A],A) wait(own,ev[A]) record(ev_build,own)");
    CHECK(u("option") == "" && u("update") == "query(A) wait(A,ev_build) record(ev_build,A)");
}

static void an_apply_on_the_carrying_stream_adds_nothing() {
    Script s;
    CHECK(s("eval(A)") == "create(ev[A])");
    CHECK(s("apply(A)") == "query(A) record(ev_build,A)" && s.last.broken == 0);
    // from another stream: ev_apply before the change, ev_build behind it; the stream is not remembered for that
    CHECK(s("apply(X)") == "query(A) create(ev_apply) record(ev_apply,X) wait(A,ev_apply) record(ev_build,A) wait(X,ev_build)");
    CHECK(s("apply(X)") == "query(A) record(ev_apply,X) wait(A,ev_apply) record(ev_build,A) wait(X,ev_build)");
    CHECK(s("update") == "query(A) record(ev_build,A)");
    // a known stream that has been made to wait at the apply's end has met the change
    Script t;
    CHECK(t("eval(A)") == "create(ev[A])" && t("eval(B)") == "create(ev[B])");
    CHECK(t("apply(B)") == "record(ev[A],A) wait(own,ev[A]) record(ev[B],B) wait(own,ev[B]) create(ev_apply) record(ev_apply,B) wait(own,ev_apply) record(ev_build,own) wait(B,ev_build)");
    CHECK(t("eval(B)") == "" && t("eval(A)") == "wait(A,ev_build)");
    CHECK(t("apply(own)") == "record(ev[A],A) wait(own,ev[A]) record(ev[B],B) wait(own,ev[B]) record(ev_build,own)");
}

static void a_forgotten_owners_pending_event_is_consumed_once() {
    Script s;
    CHECK(s("eval+scratch(A)") == "create(ev[A])");
    CHECK(s("forget(A)") == "record(ev_scratch,A) destroy(ev[A])");
    CHECK(s("forget(A)") == "");
    CHECK(s("update") == "record(ev_build,own)");  // (no caller stream is known any more)
    CHECK(s("eval+scratch(B)") == "create(ev[B]) wait(B,ev_build) wait(B,ev_scratch)");
    CHECK(s("eval+scratch(B)") == "" && s("eval+scratch(own)") == "record(ev_scratch,B) wait(own,ev_scratch)");
    // a stream that does not own the scratch leaves nothing pending
    Script t;
    CHECK(t("eval+scratch(A)") == "create(ev[A])" && t("eval+scratch(B)") == "create(ev[B]) record(ev_scratch,A) wait(B,ev_scratch)");
    CHECK(t("forget(A)") == "destroy(ev[A])" && t("eval+scratch(B)") == "");
    // the record fails (the stream is gone already): nothing is pending
    Script u;
    CHECK(u("eval+scratch(A)") == "create(ev[A])" && u("destroy(A)") == "");
    CHECK(u("forget(A)") == "record(ev_scratch,A)! destroy(ev[A])");
    CHECK(u("eval+scratch(B)") == "create(ev[B])" && u.last.rc == 0);
}

static void a_stream_destroyed_without_notice_is_dropped() {
    Script s;
    CHECK(s("eval(A)") == "create(ev[A])" && s("destroy(A)") == "");
    CHECK(s("update") == "query(A)! record(ev[A],A)! destroy(ev[A]) record(ev_build,own)");
    CHECK(s("update") == "record(ev_build,own)" && s.last.broken == 0);
    Script t;  // one of two
    CHECK(t("eval(A)") == "create(ev[A])" && t("eval(B)") == "create(ev[B])" && t("destroy(A)") == "");
    CHECK(t("update") == "record(ev[A],A)! destroy(ev[A]) record(ev[B],B) wait(own,ev[B]) record(ev_build,own)");
    CHECK(t("update") == "query(B) wait(B,ev_build) record(ev_build,B)");  // B is the one caller stream now
}

// the two sequences of g_holes, spelt out
static void the_known_holes() {
    Script s;
    s("eval(A)");
    s("eval(own)");
    CHECK(s("update") == "query(A) record(ev_build,A)");  // A does not wait for what the own stream holds
    CHECK(s.last.broken == (g_holes[kHoleOwnWorkThenRidingChange].expected_unordered ? I2 : 0u) && s.last.unexpected == 0);
    Script o;  // with the option at 1 the own stream carries the change: in order
    o("eval(A)");
    o("eval(own)");
    o("option");
    o("update");
    CHECK(o.last.broken == 0);

    Script t;
    t("eval+scratch(A)");
    t("destroy(A)");
    CHECK(t("update") == "query(A)! record(ev[A],A)! destroy(ev[A]) record(ev_build,own)");
    CHECK(t("eval+scratch(B)") == (g_holes[kHoleDestroyedScratchOwner].expected_unordered ? "create(ev[B]) wait(B,ev_build) record(ev_scratch,A)!" : "create(ev[B]) wait(B,ev_build)"));
    CHECK(t.last.broken == (g_holes[kHoleDestroyedScratchOwner].expected_unordered ? I7 : 0u) && t.last.unexpected == 0);
    CHECK(t.last.rc == (g_holes[kHoleDestroyedScratchOwner].expected_unordered ? 1 : 0));
}

// a known stream at the current generation, and the scratch's owner: no HIP call planned, nothing allocated
static void the_hot_path_allocates_nothing() {
    NewWorld w;
    w.enter(kA);
    w.enter(kB);
    w.scratch(kA);
    w.begin();
    w.end();
    w.enter(kA);
    w.enter(kOwn);
    w.hw.n = 0;
    const long before = g_allocs;
    for (int i = 0; i < 100; ++i) {
        const EnterPlan a = w.o.plan_enter(key(kA)), own = w.o.plan_enter(key(kOwn));
        CHECK(!a.is_new && !a.wait_build && !own.is_new && !own.wait_build);
        CHECK(w.o.plan_scratch(key(kA)).step == ScratchStep::kNothing);
        CHECK(w.enter(kA) == 0 && w.enter(kOwn) == 0 && w.scratch(kA) == 0);
        CHECK(w.o.res(key(kA)) && w.o.res(key(kOwn)) && !w.o.res(key(kX)));
    }
    CHECK(g_allocs == before && w.hw.n == 0);
    // the one-stream loop's change as well
    NewWorld v;
    v.enter(kA);
    v.begin();
    v.end();
    const long before2 = g_allocs;
    for (int i = 0; i < 100; ++i) CHECK(v.begin() == 0 && v.end() == 0 && v.enter(kA) == 0);
    CHECK(g_allocs == before2);
}

int main() {
    every_sequence_of_up_to_five_calls();
    the_one_stream_loop_needs_no_wait();
    two_caller_streams();
    the_option_keeps_changes_on_the_own_stream();
    the_first_evaluation_on_a_stream_after_a_change_that_rode_another();
    an_apply_on_the_carrying_stream_adds_nothing();
    a_forgotten_owners_pending_event_is_consumed_once();
    a_stream_destroyed_without_notice_is_dropped();
    the_known_holes();
    the_hot_path_allocates_nothing();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
