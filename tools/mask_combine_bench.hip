// mask_combine_bench.hip -- k_mask_combine, its yardstick and k_mask_combine_soft as C functions, for tools/mask_combine_cost.py and
// tools/mask_combine_soft_cost.py (not part of the library).
//
// No entry point of the ABI launches the combine kernel alone (a combining call always evaluates first), so the cost tool loads this
// small shared object beside the library: mcb_combine enqueues run_mask_combine (csrc/kernels_combine.hpp: the library's own launch
// path, compiled here from the same header with the same flags), mcb_copy a device-to-device hipMemcpyAsync of the same buffer,
// mcb_combine_soft run_mask_combine_soft (csrc/kernels_combine_soft.hpp, likewise).  All
// enqueue on the caller's stream and return without waiting.  Built by `make tools` into tools/libmask_combine_bench.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kube_scheduler_rs_reference_amd/csrc/kernels_combine.hpp"
#include "../kube_scheduler_rs_reference_amd/csrc/kernels_combine_soft.hpp"

extern "C" {

// flag: KSCHED_COMBINE_AND / _OR / _ANDNOT; [p] rows of ceil(n / 64) words, `pitch` words apart in dst and src
int mcb_combine(uint64_t *dst, const uint64_t *src, uint32_t p, uint32_t n, uint32_t pitch, uint32_t flag, void *stream) {
    const uint32_t W = (n + 63u) / 64u;
    if (!dst || !src || !n || pitch < W) return (int)hipErrorInvalidValue;
    return (int)ksched::run_mask_combine(ksched::combine_op(flag), dst, src, p, n, W, pitch, (hipStream_t)stream);
}

// flag: KSCHED_COMBINE_AND or _ANDNOT (KSCHED_COMBINE_SOFT beside it or not: this IS the soft combine); read_twice: the form that reads a
// row twice also where the library would keep it in registers (the comparison of the two forms)
int mcb_combine_soft(uint64_t *dst, const uint64_t *src, uint32_t p, uint32_t n, uint32_t pitch, uint32_t flag, int read_twice, void *stream) {
    const uint32_t W = (n + 63u) / 64u;
    if (!dst || !src || !n || pitch < W) return (int)hipErrorInvalidValue;
    return (int)ksched::run_mask_combine_soft(ksched::combine_op(flag), dst, src, p, n, W, pitch, (hipStream_t)stream, read_twice != 0);
}

int mcb_copy(void *dst, const void *src, size_t bytes, void *stream) {
    return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

}  // extern "C"
