// pipe_plan.hpp -- which streams one ksched_pipe_submit uses and which of the slot's two events they first wait for: a pure
// function of the slot's previous submit, the slot number, KSCHED_OPT_PIPE_MODE and whether the pick reads the mask.
//
// Host-only on purpose, like eval_plan.hpp: no HIP include, no ksched_ctx, so that plain g++ compiles it and
// tests/cpp/pipe_plan_tests.cpp runs every sequence of submits through a happens-before model without a GPU.  ksched_pipe_submit
// (ksched_api.hip) checks its arguments, calls plan_pipe_submit and executes the plan; no ordering decision is taken anywhere else.
//
// Streams are indices: 0 the mask stream, 1 the pick stream, 2 .. KSCHED_PIPE_MAX_STREAMS - 1 the alternate mode's further
// streams (ksched_pipe_stream's `which`).  A slot owns two events: mask_done, recorded behind its mask kernel by a split submit (and
// again, on the stream of its latest mask kernel, by ksched_pipe_wait_mask), and pick_done, recorded behind its pick by every submit.
//
// What a submit must be ordered behind -- a slot has ONE mask and ONE binding buffer, and a stream is in order by itself:
//   1. its mask kernel runs after the slot's previous mask kernel (both write the slot's mask);
//   2. its mask kernel runs after the slot's previous pick, if that pick read the mask;
//   3. its pick, if it reads the mask, runs after its own mask kernel;
//   4. its pick runs after the slot's previous pick (both write the slot's bindings).
//
// The rules.  By default the pick does not read the mask (eval_plan.hpp, pick_reads_mask: the uniform, spread and pack picks always do), so in the steady state the streams need
// no event at all: mask kernels of successive batches on one stream and picks on another, or a slot's whole evaluation on the same
// stream every time.  Events order a slot only where its previous use ran elsewhere, or where a pick reads the mask.
//
// WHOLE (mode >= 1 and the pick does not read the mask): the whole evaluation -- one launch when the pick rides in the mask kernel --
// on stream st = slot mod max(2, mode), then pick_done recorded on st.
//   * st waits for pick_done   if the slot has a previous pick and that pick ran on another stream (another mode's k, or the split
//                              submit's pick stream), or the previous submit was split;
//   * st waits for mask_done   if the previous submit was split and its mask kernel ran on another stream: the mask stream is
//                              ordered against nothing else, which is why a split submit records mask_done behind every mask kernel.
// SPLIT (otherwise): the mask kernel on stream 0, then mask_done recorded there; the pick on stream 1, then pick_done recorded there.
//   * streams 1 and 0 wait for pick_done   if the slot's previous pick ran on a stream other than 1 (a whole submit elsewhere);
//   * stream 0 waits for pick_done         if the slot's previous mask kernel ran on a stream other than 0 -- a whole submit, and when
//                                          that ran on stream 1 the line above does not fire: without this one the two mask kernels
//                                          are unordered (invariant 1);
//   * stream 0 waits for pick_done         if this pick or the slot's previous one reads the mask (invariant 2: this submit's pick
//                                          orders the slot's NEXT mask kernel, the previous submit's pick this one);
//   * stream 1 waits for mask_done, behind its record, if this pick reads the mask (invariant 3).
// A wait is planned at most once, and none for an event that was never recorded (a fresh slot).
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/ksched.h"

namespace ksched {

constexpr int kPipeMaskStream = 0, kPipePickStream = 1;
constexpr int kPipeNoStream = -1;  // the slot has not been submitted to

// What a slot remembers of its latest submit.  In every reachable state the mask kernel ran on stream 0 after a split submit and on
// the pick's stream after a whole one, and streams 0 and 1 differ: "was split" is mask_stream != pick_stream and needs no field.
struct PipeSlot {
    int8_t mask_stream = kPipeNoStream;  // the stream of the latest mask kernel: ksched_pipe_wait_mask records mask_done there
    int8_t pick_stream = kPipeNoStream;  // the stream of the latest pick: ksched_pipe_slot_stream
    bool pick_read_mask = false;         // the latest pick read the slot's mask
    bool used() const { return pick_stream != kPipeNoStream; }
    bool split() const { return mask_stream != pick_stream; }
};

struct PipePlan {
    bool whole = false;  // the evaluation goes whole onto mask_stream (== pick_stream); else mask kernel and pick go separately
    int mask_stream = kPipeMaskStream, pick_stream = kPipePickStream;
    // the waits, in the order the submit issues them: the first three before anything is enqueued, the fourth behind the record of mask_done
    bool mask_waits_pick_done = false, mask_waits_mask_done = false, pick_waits_pick_done = false, pick_waits_mask_done = false;
    bool record_mask_done = false;  // behind the mask kernel, on mask_stream (pick_done is always recorded, behind the pick)
    PipeSlot next;
    int waits() const { return (int)mask_waits_pick_done + (int)mask_waits_mask_done + (int)pick_waits_pick_done + (int)pick_waits_mask_done; }
};

inline PipePlan plan_pipe_submit(const PipeSlot &s, uint32_t slot, int opt_pipe_mode, bool pick_reads_mask) {
    PipePlan pl;
    if (opt_pipe_mode >= 1 && !pick_reads_mask) {
        const int st = (int)(slot % std::max(2u, (uint32_t)opt_pipe_mode));
        pl.whole = true;
        pl.mask_stream = pl.pick_stream = st;
        pl.mask_waits_pick_done = s.used() && (s.pick_stream != st || s.split());
        pl.mask_waits_mask_done = s.split() && s.mask_stream != st;
        pl.next = PipeSlot{(int8_t)st, (int8_t)st, false};
        return pl;
    }
    const bool pick_elsewhere = s.used() && s.pick_stream != kPipePickStream;
    const bool mask_elsewhere = s.used() && s.mask_stream != kPipeMaskStream;
    pl.pick_waits_pick_done = pick_elsewhere;
    pl.mask_waits_pick_done = pick_elsewhere || mask_elsewhere || (s.used() && (pick_reads_mask || s.pick_read_mask));
    pl.record_mask_done = true;
    pl.pick_waits_mask_done = pick_reads_mask;
    pl.next = PipeSlot{(int8_t)kPipeMaskStream, (int8_t)kPipePickStream, pick_reads_mask};
    return pl;
}

}  // namespace ksched
