// pipe_plan_tests.cpp -- host-side check of the pipe's submit plan (csrc/pipe_plan.hpp), no GPU and no HIP.
//
// A happens-before model of what the plan is executed on: streams are in order, a record snapshots what its stream has seen, a wait
// joins the event's latest record.  Every sequence of four submits on one slot runs through it, and every submit is asked the four
// invariants of pipe_plan.hpp.  The same model over the plan WITHOUT the wait that orders a split submit's mask kernel behind a whole
// submit's on another stream must report that hole and nothing else; the waits of the steady state and of the transitions the GPU
// tests state are written out wait by wait.
#include <cstdio>

#include "../../kube_scheduler_rs_reference_amd/csrc/pipe_plan.hpp"

using namespace ksched;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++g_fail < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)

constexpr int kStreams = (int)KSCHED_PIPE_MAX_STREAMS;
constexpr int kModes = (int)KSCHED_PIPE_MAX_STREAMS + 1;  // KSCHED_OPT_PIPE_MODE 0 .. KSCHED_PIPE_MAX_STREAMS

typedef PipePlan (*PlanFn)(const PipeSlot &, uint32_t, int, bool);

// the rules as they were before the split route's mask stream waited for a mask kernel that ran elsewhere
static PipePlan plan_without_the_new_wait(const PipeSlot &s, uint32_t slot, int mode, bool reads) {
    PipePlan pl = plan_pipe_submit(s, slot, mode, reads);
    if (!pl.whole) pl.mask_waits_pick_done = s.used() && (s.pick_stream != kPipePickStream || reads || s.pick_read_mask);
    return pl;
}

// One slot of a pipe.  A kernel is a bit; `seen[st]` is the set of kernels that have run once everything enqueued on stream st so far has.
struct Model {
    PlanFn plan;
    uint32_t slot;
    PipeSlot state;
    uint32_t seen[kStreams] = {};
    uint32_t mask_done = 0, pick_done = 0;  // what the latest record of each event saw (never recorded: nothing, a wait for it is a no-op)
    uint32_t prev_mask = 0, prev_pick = 0;  // the slot's latest mask kernel and pick (0: none yet)
    bool prev_pick_read_mask = false;
    int kernels = 0;

    Model(PlanFn f, uint32_t sl) : plan(f), slot(sl) {}

    // ksched_pipe_submit's executor over the model; returns the invariants this submit breaks (bit i - 1: invariant i)
    unsigned submit(int mode, bool reads, PipePlan *out = nullptr) {
        const PipePlan pl = plan(state, slot, mode, reads);
        if (out) *out = pl;
        unsigned broken = 0;
        const uint32_t mask = 1u << kernels++, pick = 1u << kernels++;
        const int sm = pl.mask_stream, sp = pl.pick_stream;
        CHECK(sm >= 0 && sm < kStreams && sp >= 0 && sp < kStreams && (!pl.whole || sm == sp));
        if (pl.mask_waits_pick_done) seen[sm] |= pick_done;
        if (pl.mask_waits_mask_done) seen[sm] |= mask_done;
        if (pl.pick_waits_pick_done) seen[sp] |= pick_done;
        // the mask kernel (a whole evaluation launches its pick before or inside its mask kernel: both start from what the stream has seen)
        if ((seen[sm] & prev_mask) != prev_mask) broken |= 1u;
        if (prev_pick_read_mask && (seen[sm] & prev_pick) != prev_pick) broken |= 2u;
        if (pl.whole) {
            CHECK(!reads && !pl.pick_waits_mask_done && !pl.record_mask_done);
            if ((seen[sp] & prev_pick) != prev_pick) broken |= 8u;
            seen[sm] |= mask | pick;
        } else {
            seen[sm] |= mask;
            if (pl.record_mask_done) mask_done = seen[sm];
            if (pl.pick_waits_mask_done) seen[sp] |= mask_done;
            if (reads && !(seen[sp] & mask)) broken |= 4u;
            if ((seen[sp] & prev_pick) != prev_pick) broken |= 8u;
            seen[sp] |= pick;
        }
        pick_done = seen[sp];
        // the state the plan hands on is what happened
        CHECK(pl.next.mask_stream == sm && pl.next.pick_stream == sp && pl.next.pick_read_mask == reads && pl.next.split() == !pl.whole);
        CHECK(pl.whole ? sm == sp : (sm == kPipeMaskStream && sp == kPipePickStream));
        state = pl.next;
        prev_mask = mask;
        prev_pick = pick;
        prev_pick_read_mask = reads;
        return broken;
    }

    // ksched_pipe_wait_mask: mask_done recorded again, on the stream of the slot's latest mask kernel
    void wait_mask() { mask_done = seen[state.used() ? state.mask_stream : kPipeMaskStream]; }
};

// every sequence of `submits` submits on each of slots 0 .. 8: a step is (mode, the pick reads the mask, ksched_pipe_wait_mask behind it).
// Returns the union of the broken invariants; `sequences` and `breaking` count.
static unsigned enumerate(PlanFn plan, int submits, long *sequences, long *breaking) {
    const int choices = kModes * 2 * 2;
    long total = 1;
    for (int i = 0; i < submits; ++i) total *= choices;
    unsigned all = 0;
    *sequences = *breaking = 0;
    for (uint32_t slot = 0; slot <= 8; ++slot) {
        for (long code = 0; code < total; ++code) {
            Model m(plan, slot);
            unsigned broken = 0;
            long c = code;
            for (int i = 0; i < submits; ++i, c /= choices) {
                const int step = (int)(c % choices);
                broken |= m.submit(step / 4, step & 1);
                if (step & 2) m.wait_mask();
            }
            ++*sequences;
            if (broken) ++*breaking;
            all |= broken;
        }
    }
    return all;
}

static void the_four_invariants_hold_over_every_sequence() {
    long sequences = 0, breaking = 0;
    const unsigned broken = enumerate(plan_pipe_submit, 4, &sequences, &breaking);
    std::printf("plan_pipe_submit: %ld sequences of four submits, %ld break an invariant (mask 0x%x)\n", sequences, breaking, broken);
    CHECK(sequences == 9L * 36 * 36 * 36 * 36);
    CHECK(breaking == 0 && broken == 0);
}

static void the_new_wait_is_needed() {
    // slot 1: whole at mode 2 (on stream 1 mod 2 = 1, the pick stream itself), then split: the old rules look at the pick's stream alone
    Model m(plan_without_the_new_wait, 1);
    PipePlan pl;
    CHECK(m.submit(2, false, &pl) == 0 && pl.whole && pl.mask_stream == kPipePickStream && pl.waits() == 0);
    CHECK(m.submit(0, false, &pl) == 1u);  // invariant 1 and nothing else
    CHECK(!pl.whole && pl.waits() == 0);
    // with it
    Model n(plan_pipe_submit, 1);
    CHECK(n.submit(2, false) == 0);
    CHECK(n.submit(0, false, &pl) == 0 && pl.mask_waits_pick_done && pl.waits() == 1);
    // and over every sequence the old rules break invariant 1 alone
    long sequences = 0, breaking = 0;
    const unsigned broken = enumerate(plan_without_the_new_wait, 3, &sequences, &breaking);
    std::printf("without the new wait: %ld sequences of three submits, %ld break an invariant (mask 0x%x)\n", sequences, breaking, broken);
    CHECK(broken == 1u && breaking > 0);
}

static bool waits_are(const PipePlan &pl, bool mask_pick_done, bool mask_mask_done, bool pick_pick_done, bool pick_mask_done) {
    return pl.mask_waits_pick_done == mask_pick_done && pl.mask_waits_mask_done == mask_mask_done && pl.pick_waits_pick_done == pick_pick_done &&
           pl.pick_waits_mask_done == pick_mask_done;
}

// the steady state plans no wait that the code before the plan did not issue: an event wait costs microseconds on the submit path
static void waits_per_submit() {
    for (uint32_t slot = 0; slot <= 8; ++slot) {
        for (int mode = 0; mode < kModes; ++mode) {
            for (int reads = 0; reads < 2; ++reads) {
                Model m(plan_pipe_submit, slot);
                PipePlan pl;
                m.submit(mode, reads, &pl);
                CHECK(reads ? waits_are(pl, false, false, false, true) : pl.waits() == 0);  // a fresh slot: no event has been recorded
                CHECK(pl.whole == (mode >= 1 && !reads) && pl.record_mask_done == !pl.whole);
                CHECK(pl.whole ? pl.mask_stream == (int)(slot % (uint32_t)(mode < 2 ? 2 : mode)) && pl.pick_stream == pl.mask_stream
                               : pl.mask_stream == 0 && pl.pick_stream == 1);
                for (int i = 0; i < 4; ++i) {
                    m.submit(mode, reads, &pl);
                    CHECK(reads ? waits_are(pl, true, false, false, true) : pl.waits() == 0);
                    if (i & 1) m.wait_mask();
                }
            }
        }
    }
}

// tests/test_gpu_uniform_pick.py, test_one_pipe_alternates_uniform_and_sampled_submits_on_the_same_slots: U reads the mask, S does not
static void the_transitions_the_gpu_tests_state() {
    PipePlan pl;
    for (uint32_t slot = 0; slot < 3; ++slot) {
        // mode 0: both split.  U -> S: the mask kernel waits for the pick that read the mask; S -> U: the uniform submit's own two waits
        Model a(plan_pipe_submit, slot);
        a.submit(0, true);
        a.submit(0, false, &pl);
        CHECK(!pl.whole && waits_are(pl, true, false, false, false));
        a.submit(0, true, &pl);
        CHECK(!pl.whole && waits_are(pl, true, false, false, true));
        for (int mode = 2; mode <= 3; ++mode) {
            const int st = (int)(slot % (uint32_t)mode);
            // U -> S: whole on stream slot mod k, which first waits for the split submit's pick and (from another stream) its mask kernel
            Model b(plan_pipe_submit, slot);
            b.submit(mode, true, &pl);
            CHECK(!pl.whole);
            b.submit(mode, false, &pl);
            CHECK(pl.whole && pl.mask_stream == st && waits_are(pl, true, st != kPipeMaskStream, false, false));
            // S -> U: both streams wait for that stream's pick, unless it was the pick stream itself -- then the mask stream alone
            b.submit(mode, true, &pl);
            CHECK(!pl.whole && waits_are(pl, true, false, st != kPipePickStream, true));
            // S -> S on the same stream, U -> U: the steady state
            Model c(plan_pipe_submit, slot);
            c.submit(mode, false);
            c.submit(mode, false, &pl);
            CHECK(pl.whole && pl.waits() == 0);
        }
    }
    // a change of mode between two sampled submits: the slot moves to another stream behind its previous pick
    Model d(plan_pipe_submit, 2);
    d.submit(2, false, &pl);  // stream 0
    CHECK(pl.whole && pl.mask_stream == 0);
    d.submit(3, false, &pl);  // stream 2
    CHECK(pl.whole && pl.mask_stream == 2 && waits_are(pl, true, false, false, false));
    d.submit(0, false, &pl);  // split: both streams behind stream 2's evaluation
    CHECK(!pl.whole && waits_are(pl, true, false, true, false));
    d.submit(1, false, &pl);  // whole on stream 0 again: behind the split submit's pick; its mask kernel ran on stream 0 itself
    CHECK(pl.whole && pl.mask_stream == 0 && waits_are(pl, true, false, false, false));
}

int main() {
    the_four_invariants_hold_over_every_sequence();
    the_new_wait_is_needed();
    waits_per_submit();
    the_transitions_the_gpu_tests_state();
    std::printf("%d failed check(s)\n", g_fail);
    return g_fail ? 1 : 0;
}
