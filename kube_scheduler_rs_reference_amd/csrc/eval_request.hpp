// eval_request.hpp -- one batch of pods on the device, as every evaluation entry point of ksched_api.hip hands it on.
//
// Built once per C entry point and passed by const reference to eval_on_device, launch_select, make_select_args, run_direct,
// launch_pick, run_fused and summarize_on_device (which reads the subset it needs).  The normalised terms -- is the selector
// term active, is the taint term -- are derived here and nowhere else.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ksched.h"

namespace ksched {

struct EvalRequest {
    uint32_t p = 0;
    const int64_t *pcpu = nullptr, *pmem = nullptr;
    const uint32_t *psel = nullptr;
    const uint64_t *ptol = nullptr;
    const uint32_t *samples = nullptr;
    uint32_t attempts = 0, flags = 0;
    uint64_t *out_feas = nullptr, *out_fit = nullptr;
    int32_t *out_binding = nullptr;
    uint32_t pitch = 0;  // words between consecutive pod rows of the output masks (>= W; W = packed)
    hipStream_t stream = nullptr;

    bool fit() const { return flags & KSCHED_FIT; }
    bool want_fit() const { return (flags & KSCHED_WANT_FIT_MASK) && out_fit; }
    // the selector term is active: asked for, selectors given, and the snapshot (or the index layout: run_fused) has `nkeys` > 0 label keys
    bool sel(uint32_t nkeys) const { return (flags & KSCHED_SEL) && psel && nkeys > 0; }
    // The taint term.  The call sites differ, and each keeps its rule:
    //  * taint_flag(): the flag alone -- run_direct selects its TAINT instantiation by it and passes a null taint column when the snapshot has none;
    //  * taint(have): ... and the snapshot has taints -- make_select_args, the best-fit rows, ksched_explain, the direct summary with `have_taints`,
    //    run_fused with the layout's `ngroups`.
    bool taint_flag() const { return flags & KSCHED_TAINT; }
    bool taint(bool have) const { return (flags & KSCHED_TAINT) && have; }
};

}  // namespace ksched
