// apply_admit.hpp -- the arithmetic of KSCHED_APPLY_WHILE_FIT's chunk walk (kernels_build.hpp k_apply_admit), readable by a host
// compiler too: the per-lane test, the first-failing-lane step and the carry of what is left of a node.
//
// The rule, per node: its eligible pods in ascending pod index, R = (R_cpu, R_mem) = the node's `available`; pod i is admitted iff
// req_cpu[i] <= R_cpu && req_mem[i] <= R_mem (signed compares: can_pod_fit, src/predicates.rs:37-42) and neither R - req passes
// INT64_MAX (a negative request only; such a pod reports OVERFLOW); an admitted pod gives R -= req; every other pod changes nothing and
// the walk goes on behind it.
//
// A wave takes 64 pods of the node at a time.  One STEP over the chunk's undecided lanes: lane j forms the exclusive prefix e_j of
// the undecided lanes' requests before it and tests its own request against R - e_j; the first failing lane f is decided (DEFERRED or
// OVERFLOW), the undecided lanes before f are admitted -- for them R - e_j IS the serial walk's state, by induction over j --, R
// becomes R - e_f, and the next step runs over the undecided lanes behind f.  A prefix of 64 int64 can leave int64, so the halves of
// every request (the split of k_apply_accumulate) are scanned apart and joined in 128 bits; R - e_j of a lane that counts is a state
// of the serial walk and so inside int64.  When no undecided lane has a negative request R cannot grow during the chunk: a lane whose
// own request does not fit R at a step's start would not fit when the serial walk reaches it either, and is DEFERRED at once.
//
// No HIP include on purpose: plain g++ compiles it, and tests/cpp/apply_admit_tests.cpp runs a 64-lane emulation of the walk over these
// functions against the serial rule.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KSCHED_ADMIT_HD __host__ __device__ __forceinline__
#else
#define KSCHED_ADMIT_HD inline
#endif

namespace ksched {

constexpr uint32_t kAdmitLanes = 64;  // a chunk: one pod per lane of a wave
enum AdmitVerdict : int { kAdmitPass = 0, kAdmitDefer = 1, kAdmitOverflow = 2 };

// req = hi * 2^32 + lo, hi signed and lo in [0, 2^32): 64 of either sum inside int64
KSCHED_ADMIT_HD int64_t admit_hi(int64_t req) { return req >> 32; }
KSCHED_ADMIT_HD int64_t admit_lo(int64_t req) { return (int64_t)((uint64_t)req & 0xFFFFFFFFull); }
KSCHED_ADMIT_HD __int128 admit_join(int64_t hi, int64_t lo) { return (__int128)hi * ((__int128)1 << 32) + (__int128)lo; }

// does a request fit what is left (the compares of can_pod_fit)
KSCHED_ADMIT_HD bool admit_fits(int64_t r_cpu, int64_t r_mem, int64_t req_cpu, int64_t req_mem) { return req_cpu <= r_cpu && req_mem <= r_mem; }

// the per-lane test: a request against what is left before it, R - e, e = the prefix of the undecided lanes before this one
KSCHED_ADMIT_HD AdmitVerdict admit_lane_test(int64_t r_cpu, int64_t r_mem, __int128 e_cpu, __int128 e_mem, int64_t req_cpu, int64_t req_mem) {
    const __int128 left_cpu = (__int128)r_cpu - e_cpu, left_mem = (__int128)r_mem - e_mem;
    if ((__int128)req_cpu > left_cpu || (__int128)req_mem > left_mem) return kAdmitDefer;
    if (left_cpu - (__int128)req_cpu > (__int128)INT64_MAX || left_mem - (__int128)req_mem > (__int128)INT64_MAX) return kAdmitOverflow;
    return kAdmitPass;
}

// the first failing lane of a step (`failing`: bit j = undecided lane j did not pass), kAdmitLanes when every undecided lane passed
KSCHED_ADMIT_HD uint32_t admit_first_failing(uint64_t failing) { return failing ? (uint32_t)__builtin_ctzll(failing) : kAdmitLanes; }

// what is left after a step: R - (the prefix before the first failing lane, or the step's whole sum); a state of the serial walk
KSCHED_ADMIT_HD int64_t admit_carry(int64_t r, __int128 prefix) { return (int64_t)((__int128)r - prefix); }

}  // namespace ksched
