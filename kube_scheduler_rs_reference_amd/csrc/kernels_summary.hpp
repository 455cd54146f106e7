// kernels_summary.hpp -- per-pod node counts by reason (ksched_summarize*): for every pod of a batch, how many nodes of the
// snapshot check_node_validity (src/predicates.rs:63-77) accepts and how many it rejects for each InvalidNodeReason, with the
// precedence of the reference: resources first (:68-70), then the selector (:72-74), then the taint extension.  The answer to
// "why did no node take this pod" behind NoNodeFound (src/main.rs:116-118), and the first evaluation form whose output is O(P):
// no mask is stored.
//
// With F = fit (cpu AND memory), S = selector, T = taints as node sets (predicates not selected = every node):
//     ok    = |F & S & T|        resources = N - |F|        selector = |F & ~S|        taint = |F & S & ~T|
// the four are disjoint and cover the N nodes, so `resources` is taken as N - ok - selector - taint.
//
// k_summarize_indexed: the decomposition of the fused mask kernel (kernels_fused.hpp) over the same per-tile bitmap index
// (tile_index.hpp): a block owns one 1024-node tile and a share of the batch's rounds of 64 pods, stages the tile's rows and aux
// block into LDS, phase 1 (lane = pod) does the two rank searches, the cnt[rank] lookups and the selector-id -> row translation,
// phase 2 (8 lanes per pod, one 128-node chunk per lane) reads the row chunks.  Instead of ANDing everything into one word and
// storing it, the three terms stay apart and are population-counted.  Every row's padding bits (node >= N) are zero and every
// count has F as a factor, so padding never counts.  A lane's three counts (<= 128 each) go back into the pod's own record as
// one packed word; lane = pod then adds the eight and holds the tile's counts of its pod (<= 1024 each: 16-bit fields of one
// 64-bit word).
// Across tiles (SummaryArgs::atomic): 0 = the word is written to partial[tile][pod] with a plain coalesced store (512 bytes per
// wave), and k_summary_reduce adds a pod's `tiles` words: nothing to zero, every sum in a fixed order; 1 = two no-return 64-bit
// atomic adds per (pod, tile) into the caller's table behind k_summary_zero (integer adds commute: the same bits either way).
//
// k_summarize_direct: lanes = nodes, the compare is the ballot (the pattern of kernels_direct.hpp), for snapshots without an
// index.  A block of four waves owns 64 pods and walks every node, 256 at a time; pod operands are wave-uniform; the three
// ballots of a (pod, 64 nodes) step are population-counted on the scalar unit and added in lane `pod`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eval_request.hpp"
#include "kernarg.hpp"
#include "kernels_fused.hpp"  // u32x4
#include "tile_index.hpp"
#include "tile_launch.hpp"  // kFusedThreads, the LDS carve-up (every region), the launch geometry, the argument fill, with_predicates

namespace ksched {

constexpr uint32_t kSummaryThreads = kFusedThreads;
constexpr uint32_t kSummaryWaves = kSummaryThreads / 64;
static_assert(KSCHED_SUMMARY_WORDS == 4u && KSCHED_REASON_OK == 0 && KSCHED_REASON_NOT_ENOUGH_RESOURCES == 1 &&
                  KSCHED_REASON_NODE_SELECTOR_MISMATCH == 2 && KSCHED_REASON_TAINT_NOT_TOLERATED == 3,
              "out_counts[pod] is indexed by KSCHED_REASON_*");

struct SummaryArgs {
    uint32_t n, p, tiles, rows, nkeys, ngroups;
    uint32_t row_zero, row_valid, row_cpu, row_taint;
    uint32_t lab_off[8], lab_mx1[8];  // as FusedArgs: first eight label keys, byte offset of the row before id 1's and lab_max + 1
    const uint32_t *lab_meta;         // device copy of IndexedLayout::lab_base[32], lab_max[32]
    const uint64_t *zero64;           // eight zero bytes in device memory
    uint32_t chunks, rounds;          // blocks per tile, rounds of 64 pods in the batch
    uint32_t off_aux, off_fit, off_lab, off_trow, off_list, off_lrec;  // LDS byte offsets of the regions after the bitmap rows
    uint32_t nlist, list_mask8;
    uint32_t list_col[kMaxListKeys];
    uint32_t has_tol;
    uint32_t atomic;                  // cross-tile combine: 0 = partial words + k_summary_reduce, 1 = atomic adds into out_counts
};

__device__ __forceinline__ uint32_t popc4(const u32x4 v, uint32_t acc = 0u) {
    return __popc(v.x) + (__popc(v.y) + (__popc(v.z) + (__popc(v.w) + acc)));
}

template <bool FIT, bool SEL, bool TAINT, bool LIST>
__global__ __launch_bounds__(kSummaryThreads) void k_summarize_indexed(
    const uint64_t *__restrict__ g_tables, const uint64_t *__restrict__ g_aux, const int64_t *__restrict__ g_pcpu,
    const int64_t *__restrict__ g_pmem, const uint32_t *__restrict__ g_psel, const uint64_t *__restrict__ g_ptol,
    const uint8_t *__restrict__ g_list, uint64_t *__restrict__ g_partial, unsigned long long *__restrict__ g_counts, const SummaryArgs a) {
    static_assert(!LIST || SEL, "list keys only exist with the selector predicate");
    kernarg_warm<9 * 8 + sizeof(SummaryArgs)>();
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    lds_u8 *const lds = (lds_u8 *)smem;
    const uint32_t tile = blockIdx.x % a.tiles, chunk = blockIdx.x / a.tiles;  // neighbouring blocks: the tiles of one pod range
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // ---- stage the tile: global -> LDS without a VGPR round trip (as the fused kernel does) --------------------------------
    auto stage = [&](const void *gsrc, uint32_t lds_off, uint32_t bytes) {
        const uint8_t *g = static_cast<const uint8_t *>(gsrc);
        for (uint32_t off = wave * 1024u; off < bytes; off += kSummaryWaves * 1024u) {
            if (off + lane * 16u < bytes)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + off + lane * 16u),
                                                 (__attribute__((address_space(3))) void *)(lds + lds_off + off), 16, 0, 0);
        }
    };
    if (FIT) stage(g_aux + (size_t)tile * kAuxWords, a.off_aux, kAuxWords * 8u);
    if (LIST) stage(g_list + (size_t)tile * a.nlist * kListBytes, a.off_list, a.nlist * kListBytes);
    stage(g_tables + (size_t)tile * a.rows * kTileWords, 0u, a.rows * 128u);

    // round g of the batch (64 pods) belongs to block chunk g mod chunks, wave (g / chunks) mod waves: the rounds in flight
    // at any time are neighbours, and every tile-block of a chunk walks the same rounds
    uint32_t g = chunk + wave * a.chunks;
    const uint32_t g_stride = a.chunks * kSummaryWaves;

    // ---- pod operands of a round, lane = pod (clamped: lanes past the batch's end read a valid row and are masked at the end) ----
    int64_t rc = 0, rm = 0;
    uint32_t sv[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint64_t tol = 0;
    auto load_ops = [&](uint32_t round) {
        const uint32_t pc = min(round * 64u + lane, a.p - 1u);
        if (FIT) {
            rc = g_pcpu[pc];
            rm = g_pmem[pc];
        }
        if (SEL) {
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) sv[k] = k < a.nkeys ? g_psel[(size_t)k * a.p + pc] : 0u;
        }
        if (TAINT) tol = a.has_tol ? g_ptol[pc] : 0ull;
    };
    if (g < a.rounds) load_ops(g);
    __builtin_amdgcn_s_waitcnt(0);  // this wave's staging pieces have landed
    __syncthreads();

    const int64_t *s_cpu = reinterpret_cast<const int64_t *>(smem + a.off_aux);
    const int64_t *s_mem = s_cpu + kAuxTreeWords;
    const uint2 *s_cnt_cpu = reinterpret_cast<const uint2 *>(s_cpu + 2u * kAuxTreeWords);
    const uint2 *s_cnt_mem = s_cnt_cpu + kCntEntries;
    uint4 *s_fit = reinterpret_cast<uint4 *>(smem + a.off_fit) + wave * 64u;    // cnt[rank]: 8 bytes of cpu, 8 of memory; afterwards the counts of chunks 0..3
    uint4 *s_lab = reinterpret_cast<uint4 *>(smem + a.off_lab) + wave * 64u;    // row offsets of the pod's constrained keys 1..8; afterwards the counts of chunks 4..7
    uint2 *s_trow = reinterpret_cast<uint2 *>(smem + a.off_trow) + wave * 64u;  // four taint row offsets per pod
    uint2 *s_lrec = reinterpret_cast<uint2 *>(smem + a.off_lrec) + wave * 64u;  // LIST: per list key (first entry | count << 16); count 0xFFFF = unconstrained

    // phase-2 lane layout: 8 lanes per pod, lane `wp` owns chunk (sub-tile) wp of every row = 16 bytes = 128 nodes
    const uint32_t wp = lane & 7u, sub = lane >> 3;
    const uint8_t *Tb = smem + wp * 16u;  // this lane's chunk of row 0
    auto ldoff = [&](uint32_t off) -> u32x4 { return *reinterpret_cast<const u32x4 *>(Tb + off); };  // off = row * 128
    auto ldrow = [&](uint32_t row) -> u32x4 { return ldoff(row * 128u); };
    const bool taint_inline = a.ngroups <= 4u;
    const uint32_t rv = a.row_valid * 128u;

    // LIST: the nodes of this tile that carry the pod's value of a list key sit at entries [first, first + count) of the key's
    // sorted list; the lane sets the bits of the entries that fall into its sub-tile
    auto list_mask = [&](uint32_t j, uint32_t rec) -> u32x4 {
        const uint32_t noff = a.off_list + j * kListBytes + kTileNodes * 4u;  // LDS byte offset of the key's node numbers
        const uint32_t first = rec & 0xFFFFu, count = rec >> 16;
        if (count == 0xFFFFu) return u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // the pod does not constrain this key
        u32x4 m = {0u, 0u, 0u, 0u};
        for (uint32_t e = 0; e < count; ++e) {
            const uint32_t node = *(const __attribute__((address_space(3))) uint16_t *)(lds + noff + min(first + e, (uint32_t)kTileNodes - 1u) * 2u);
            const uint32_t bit = ((node >> 7) == wp) ? (1u << (node & 31u)) : 0u, w = (node >> 5) & 3u;
            m.x |= (w == 0u) ? bit : 0u;
            m.y |= (w == 1u) ? bit : 0u;
            m.z |= (w == 2u) ? bit : 0u;
            m.w |= (w == 3u) ? bit : 0u;
        }
        return m;
    };

    while (g < a.rounds) {  // wave-uniform
        const uint32_t pod0 = g * 64u;
        // ================= phase 1: lane = pod pod0 + lane (the fused kernel's, without its pipelining) =================
        if (FIT) {
            // r = #sorted values < req: two interleaved descents of the tile's breadth-first search trees (tile_index.hpp)
            uint32_t kc = 1, km = 1;
#pragma unroll
            for (uint32_t level = 0; level < 10; ++level) {
                const int64_t vc = s_cpu[kc], vm = s_mem[km];
                kc = 2u * kc + ((vc < rc) ? 1u : 0u);
                km = 2u * km + ((vm < rm) ? 1u : 0u);
            }
            uint32_t lc = kc - (uint32_t)kTileNodes, lm = km - (uint32_t)kTileNodes;
            lc += (lc == (uint32_t)kTileNodes - 1u && s_cpu[0] < rc) ? 1u : 0u;  // slot 0 holds sorted[1023]: 1023 -> 1024
            lm += (lm == (uint32_t)kTileNodes - 1u && s_mem[0] < rm) ? 1u : 0u;
            const uint2 cc = s_cnt_cpu[lc], cm = s_cnt_mem[lm];
            s_fit[lane] = make_uint4(cc.x, cc.y, cm.x, cm.y);
        }
        uint32_t cnt = 0;
        if (SEL) {
            // the record starts as eight times the all-valid row; the pod's j-th constrained key overwrites slot j
            const uint32_t rv2 = rv | (rv << 16);
            s_lab[lane] = make_uint4(rv2, rv2, rv2, rv2);
            uint16_t *const slots = reinterpret_cast<uint16_t *>(s_lab + lane);
            uint16_t *slot = slots;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t s = sv[k];
                if (s != 0u && !(LIST && ((a.list_mask8 >> k) & 1u)))
                    // value id s of key k -> its row; ids no node carries (KSCHED_SEL_NEVER, unknown) clamp to the key's all-zero row
                    *slot++ = (uint16_t)(min(s, a.lab_mx1[k]) * 128u + a.lab_off[k]);
            }
            cnt = (uint32_t)(slot - slots);
            if (a.nkeys > 8u) {  // keys 9.. : any constraint there sends the pod down the walk over every key
                const uint32_t pc = min(pod0 + lane, a.p - 1u);
                for (uint32_t k = 8; k < a.nkeys; ++k) {
                    if (LIST && a.lab_meta[k] == kLabList) continue;
                    cnt += (g_psel[(size_t)k * a.p + pc] != 0u) ? 9u : 0u;
                }
            }
        }
        bool list_any = false;
        if (LIST) {
            // list keys: the pod's id -> the range of the tile's sorted list that carries it (two lower bounds over 1024 entries)
            uint32_t rec[kMaxListKeys];
            bool any = false;
#pragma unroll
            for (uint32_t j = 0; j < kMaxListKeys; ++j) {
                rec[j] = 0xFFFF0000u;  // unconstrained
                if (j >= a.nlist) continue;
                const uint32_t col = a.list_col[j];
                uint32_t s;
                if (col < 8u) {
                    s = sv[0];
#pragma unroll
                    for (uint32_t k = 1; k < 8; ++k) s = (col == k) ? sv[k] : s;
                } else {
                    s = g_psel[(size_t)col * a.p + min(pod0 + lane, a.p - 1u)];
                }
                if (s != 0u) {
                    const uint32_t voff = a.off_list + j * kListBytes;  // LDS byte offset of the key's sorted ids
                    auto val_at = [&](uint32_t e) -> uint32_t { return *(const __attribute__((address_space(3))) uint32_t *)(lds + voff + e * 4u); };
                    auto lower = [&](uint32_t key) -> uint32_t {  // number of entries below `key`
                        uint32_t base = 0;
#pragma unroll
                        for (uint32_t half = (uint32_t)kTileNodes / 2u; half >= 1u; half >>= 1) base += (val_at(base + half - 1u) < key) ? half : 0u;
                        return base + ((val_at(base) < key) ? 1u : 0u);
                    };
                    const uint32_t lo = lower(s);
                    // (ids are < KSCHED_SEL_NEVER on nodes; SEL_NEVER itself is carried by none: both bounds are 1024, the range is empty)
                    const uint32_t hi = (s == KSCHED_SEL_NEVER) ? lo : lower(s + 1u);
                    rec[j] = lo | ((hi - lo) << 16);
                    any = true;
                }
            }
            s_lrec[lane] = make_uint2(rec[0], rec[1]);
            list_any = __ballot(any) != 0ull;
        }
        if (TAINT) {
            uint32_t t[4];
#pragma unroll
            for (uint32_t gg = 0; gg < 4; ++gg)
                t[gg] = (gg < a.ngroups) ? (a.row_taint + 16u * gg + (uint32_t)((tol >> (4u * gg)) & 15ull)) * 128u : rv;
            s_trow[lane] = make_uint2(t[0] | (t[1] << 16), t[2] | (t[3] << 16));
        }
        const bool extra_any = __ballot(cnt > 4u) != 0ull;  // some pod of the round needs label rows 5..8
        const uint64_t over = __ballot(cnt > 8u);          // more than eight row keys constrained
        // the next round's operands: in flight during phase 2
        const uint32_t g_next = g + g_stride;
        if (g_next < a.rounds) load_ops(g_next);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ================= phase 2: 8 lanes per pod, pod row it * 8 + sub of the round =================
        const bool plain = over == 0ull && (!TAINT || taint_inline) && !(LIST && list_any);  // wave-uniform
        auto one_row = [&](uint32_t it, bool checked) {
            const uint32_t pl = it * 8u + sub;
            const uint4 fr = s_fit[pl];
            const uint4 lr = s_lab[pl];
            u32x4 F, S = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, T = S;
            if (FIT) {
                // this lane's cnt byte of each resource: the row {lr >= cnt[rank][wp]}
                const uint32_t sh = (wp & 3u) * 8u;
                const uint32_t cc = ((wp < 4u ? fr.x : fr.y) >> sh) & 0xFFu, cm = ((wp < 4u ? fr.z : fr.w) >> sh) & 0xFFu;
                F = ldrow(a.row_cpu + cc) & ldrow(a.row_cpu + (uint32_t)kFitRows + cm);  // src/predicates.rs:42, both resources
            } else {
                F = ldoff(rv);
            }
            if (SEL) {  // src/predicates.rs:45-61
                if (checked && ((over >> pl) & 1ull)) {
                    const uint32_t pod = min(pod0 + pl, a.p - 1u);
                    for (uint32_t k = 0; k < a.nkeys; ++k) {
                        if (LIST && a.lab_meta[k] == kLabList) continue;  // list keys have no rows (applied below)
                        const uint32_t s = g_psel[(size_t)k * a.p + pod];
                        if (s != 0u) S &= ldrow((s <= a.lab_meta[32u + k]) ? (a.lab_meta[k] + s - 1u) : a.row_zero);
                    }
                } else {
                    S = (ldoff(lr.x & 0xFFFFu) & ldoff(lr.x >> 16)) & (ldoff(lr.y & 0xFFFFu) & ldoff(lr.y >> 16));
                    if (extra_any) S &= (ldoff(lr.z & 0xFFFFu) & ldoff(lr.z >> 16)) & (ldoff(lr.w & 0xFFFFu) & ldoff(lr.w >> 16));
                }
                if (LIST && checked) {
                    const uint2 rec = s_lrec[pl];
                    if (0u < a.nlist) S &= list_mask(0u, rec.x);
                    if (1u < a.nlist) S &= list_mask(1u, rec.y);
                }
            }
            if (TAINT) {
                if (taint_inline) {
                    const uint2 tr = s_trow[pl];
                    T = (ldoff(tr.x & 0xFFFFu) & ldoff(tr.x >> 16)) & (ldoff(tr.y & 0xFFFFu) & ldoff(tr.y >> 16));
                } else {
                    const uint64_t t = a.has_tol ? g_ptol[min(pod0 + pl, a.p - 1u)] : 0ull;
                    for (uint32_t gg = 0; gg < a.ngroups; ++gg) T &= ldrow(a.row_taint + 16u * gg + (uint32_t)((t >> (4u * gg)) & 15ull));
                }
            }
            // check_node_validity's precedence: a node short of resources counts there whatever its labels and taints
            // (N - the three below); a node that fits and misses the selector counts there whatever its taints
            const u32x4 FS = F & S;
            const uint32_t c_ok = popc4(FS & T), c_sel = popc4(F & ~S), c_taint = popc4(FS & ~T);
            // back into the pod's own records (every lane of the pod has read them above; LDS operations of a wave execute in order)
            uint32_t *dst = wp < 4u ? reinterpret_cast<uint32_t *>(s_fit + pl) + wp : reinterpret_cast<uint32_t *>(s_lab + pl) + (wp - 4u);
            *dst = c_ok | (c_sel << 8) | (c_taint << 16);  // each <= 128
        };
        if (plain) {
#pragma unroll
            for (uint32_t it = 0; it < 8; ++it) one_row(it, false);
        } else {
#pragma unroll 1
            for (uint32_t it = 0; it < 8; ++it) one_row(it, true);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ================= lane = pod again: the tile's counts of pod pod0 + lane =================
        {
            const uint4 x = s_fit[lane], y = s_lab[lane];
            const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
            uint32_t c_ok = 0, c_sel = 0, c_taint = 0;
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) {
                c_ok += w[i] & 0xFFu;
                c_sel += (w[i] >> 8) & 0xFFu;
                c_taint += w[i] >> 16;
            }
            const uint32_t pod = pod0 + lane;
            if (pod < a.p) {
                if (!a.atomic) {
                    g_partial[(size_t)tile * a.p + pod] = (uint64_t)c_ok | ((uint64_t)c_sel << 16) | ((uint64_t)c_taint << 32);
                } else {
                    // out_counts[pod] = {ok, resources | selector, taint}: two 64-bit adds, no field can carry (every total is <= N < 2^32)
                    const uint32_t m_tile = min((uint32_t)kTileNodes, a.n - tile * (uint32_t)kTileNodes);
                    const uint32_t c_res = m_tile - c_ok - c_sel - c_taint;
                    __hip_atomic_fetch_add(g_counts + 2u * (size_t)pod, (unsigned long long)c_ok | ((unsigned long long)c_res << 32), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(g_counts + 2u * (size_t)pod + 1u, (unsigned long long)c_sel | ((unsigned long long)c_taint << 32),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the records are free for the next round
        g = g_next;
    }
}

// one pod's four words; `aligned` = the table starts on a 16-byte boundary (wave-uniform)
__device__ __forceinline__ void store_counts(uint32_t *__restrict__ out, uint32_t pod, uint32_t n, uint32_t c_ok, uint32_t c_sel, uint32_t c_taint,
                                             bool aligned) {
    const uint4 v = make_uint4(c_ok, n - c_ok - c_sel - c_taint, c_sel, c_taint);
    if (aligned) {
        reinterpret_cast<uint4 *>(out)[pod] = v;
    } else {
        out[4u * (size_t)pod] = v.x;
        out[4u * (size_t)pod + 1u] = v.y;
        out[4u * (size_t)pod + 2u] = v.z;
        out[4u * (size_t)pod + 3u] = v.w;
    }
}

// partial[tile][pod] (16-bit fields ok | selector | taint) -> out_counts[pod][4]; a pod's words are added in tile order
__global__ __launch_bounds__(256) void k_summary_reduce(const uint64_t *__restrict__ partial, uint32_t *__restrict__ out, uint32_t p, uint32_t tiles,
                                                        uint32_t n, uint32_t aligned) {
    const uint32_t pod = blockIdx.x * 256u + threadIdx.x;
    if (pod >= p) return;
    uint32_t c_ok = 0, c_sel = 0, c_taint = 0;
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint64_t w = partial[(size_t)t * p + pod];
        c_ok += (uint32_t)w & 0xFFFFu;
        c_sel += (uint32_t)(w >> 16) & 0xFFFFu;
        c_taint += (uint32_t)(w >> 32) & 0xFFFFu;
    }
    store_counts(out, pod, n, c_ok, c_sel, c_taint, aligned != 0u);
}

__global__ __launch_bounds__(256) void k_summary_zero(unsigned long long *__restrict__ out, uint32_t p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 2u * p) out[i] = 0ull;
}

struct SummaryLaunch {
    const IndexedSnapshot *snap;
    const int64_t *pcpu, *pmem;
    const uint32_t *psel;
    const uint64_t *ptol;
    uint64_t *partial;
    uint32_t *out;
    dim3 grid;
    uint32_t lds;
    hipStream_t stream;
};

template <bool FIT, bool SEL, bool TAINT, bool LIST>
inline hipError_t launch_summary_k(const SummaryLaunch &q, const SummaryArgs &a) {
    auto kern = k_summarize_indexed<FIT, SEL, TAINT, LIST>;
    hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.lds);
    if (e != hipSuccess) return e;
    const IndexedSnapshot &s = *q.snap;
    hipLaunchKernelGGL(kern, q.grid, dim3(kSummaryThreads), q.lds, q.stream, s.d_tables, s.d_aux, q.pcpu, q.pmem, q.psel, q.ptol,
                       (const uint8_t *)s.d_list, q.partial, reinterpret_cast<unsigned long long *>(q.out), a);
    return hipGetLastError();
}

// (true of every indexed snapshot: tile_launch.hpp's static_assert on what indexed_plan has checked)
inline bool summary_indexed_applicable(const IndexedSnapshot &s) { return s.built && tile_lds_layout(s.lay, kLdsEveryRegion).bytes <= kLdsBudget; }

// words of ctx-owned scratch the partial form needs
inline size_t summary_partial_words(const IndexedSnapshot &s, uint32_t p) { return (size_t)s.lay.tiles * p; }

// out: [p][KSCHED_SUMMARY_WORDS]; partial: [tiles][p], or unused with atomic = true (`out` must then sit on an 8-byte boundary)
// (of the request: p, pcpu, pmem, psel, ptol, flags and the stream)
inline hipError_t run_summary_indexed(const IndexedSnapshot &s, const EvalRequest &r, uint32_t *out, uint64_t *partial, bool atomic) {
    const IndexedLayout &l = s.lay;
    const uint32_t p = r.p;
    const TileTerms t = tile_terms(r, l);
    const TileLds lds = tile_lds_layout(l, kLdsEveryRegion);
    if (lds.bytes > kLdsBudget) return hipErrorInvalidValue;
    const SummaryGeometry g = summary_geometry(p, l.tiles, lds.bytes);
    SummaryArgs a{};
    fill_tile_args(a, s, lds, t, r);
    a.n = l.n;
    a.chunks = g.chunks;
    a.rounds = g.rounds;
    a.atomic = atomic ? 1u : 0u;
    const SummaryLaunch q{&s, r.pcpu, r.pmem, r.psel, r.ptol, partial, out, dim3(g.grid), lds.bytes, r.stream};
    hipError_t e;
    if (atomic) {
        if (reinterpret_cast<uintptr_t>(out) & 7u) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_summary_zero, dim3((2u * p + 255u) / 256u), dim3(256), 0, r.stream, reinterpret_cast<unsigned long long *>(out), p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = with_predicates(t.fit, t.sel, t.taint, [&](auto F, auto S, auto T) {
        constexpr bool kF = decltype(F)::value, kS = decltype(S)::value, kT = decltype(T)::value;
        return (kS && t.list) ? launch_summary_k<kF, kS, kT, kS>(q, a) : launch_summary_k<kF, kS, kT, false>(q, a);
    });
    if (e != hipSuccess) return e;
    if (!atomic) {
        hipLaunchKernelGGL(k_summary_reduce, dim3((p + 255u) / 256u), dim3(256), 0, r.stream, partial, out, p, l.tiles, l.n,
                           (reinterpret_cast<uintptr_t>(out) & 15u) ? 0u : 1u);
        e = hipGetLastError();
    }
    return e;
}

// ---- direct path ----------------------------------------------------------------------------------------------------------
struct SummaryDirectArgs {
    uint32_t n, p, nkeys;
    uint32_t do_fit;
    uint32_t aligned;  // `out` starts on a 16-byte boundary
};

constexpr uint32_t kSummaryDirectWaves = 4;

// Pointers are separate __restrict__ parameters so that the wave-uniform pod loads stay on the scalar unit (kernels_direct.hpp).
__global__ __launch_bounds__(64 * kSummaryDirectWaves) void k_summarize_direct(
    const int64_t *__restrict__ g_ncpu, const int64_t *__restrict__ g_nmem, const uint32_t *__restrict__ g_nlab,
    const uint64_t *__restrict__ g_ntaint, const int64_t *__restrict__ g_pcpu, const int64_t *__restrict__ g_pmem,
    const uint32_t *__restrict__ g_psel, const uint64_t *__restrict__ g_ptol, uint32_t *__restrict__ out, const SummaryDirectArgs a) {
    __shared__ uint32_t s_acc[kSummaryDirectWaves][3][64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t p0 = blockIdx.x * 64u;
    const uint32_t jmax = min(64u, a.p - p0);
    uint32_t c_ok = 0, c_sel = 0, c_taint = 0;  // of pod p0 + lane, over this wave's nodes
    for (uint32_t base = wave * 64u; base < a.n; base += kSummaryDirectWaves * 64u) {
        const uint32_t node = base + lane;
        const bool in = node < a.n;
        const uint32_t nc = in ? node : a.n - 1u;
        const int64_t ncpu = g_ncpu[nc], nmem = g_nmem[nc];
        const uint64_t ntaint = g_ntaint ? g_ntaint[nc] : 0ull;
        for (uint32_t j = 0; j < jmax; ++j) {
            const uint32_t pod = p0 + j;  // wave-uniform -> scalar loads
            uint64_t F = __ballot(in);
            if (a.do_fit) F &= __ballot(g_pcpu[pod] <= ncpu) & __ballot(g_pmem[pod] <= nmem);  // src/predicates.rs:42
            uint64_t S = ~0ull;
            if (g_psel) {
                for (uint32_t k = 0; k < a.nkeys; ++k) {  // src/predicates.rs:48-57
                    const uint32_t s = g_psel[(size_t)k * a.p + pod];
                    if (s != 0u) S &= __ballot(s == g_nlab[(size_t)k * a.n + nc]);  // wave-uniform branch
                }
            }
            uint64_t T = ~0ull;
            if (g_ntaint) T = __ballot((ntaint & ~(g_ptol ? g_ptol[pod] : 0ull)) == 0ull);
            // precedence of check_node_validity: resources (src/predicates.rs:68-70), selector (:72-74), taints
            const uint32_t d_ok = (uint32_t)__popcll(F & S & T), d_sel = (uint32_t)__popcll(F & ~S), d_taint = (uint32_t)__popcll(F & S & ~T);
            if (lane == j) {
                c_ok += d_ok;
                c_sel += d_sel;
                c_taint += d_taint;
            }
        }
    }
    s_acc[wave][0][lane] = c_ok;
    s_acc[wave][1][lane] = c_sel;
    s_acc[wave][2][lane] = c_taint;
    __syncthreads();
    if (wave == 0u && lane < jmax) {
        uint32_t t_ok = 0, t_sel = 0, t_taint = 0;
#pragma unroll
        for (uint32_t w = 0; w < kSummaryDirectWaves; ++w) {
            t_ok += s_acc[w][0][lane];
            t_sel += s_acc[w][1][lane];
            t_taint += s_acc[w][2][lane];
        }
        store_counts(out, p0 + lane, a.n, t_ok, t_sel, t_taint, a.aligned != 0u);
    }
}

}  // namespace ksched
