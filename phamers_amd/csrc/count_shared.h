// count_shared.h -- what the count units share: the control block's words, the device helpers of the slot / plan / sort /
// wave-per-contig kernels, the route of one phk_launch_count call (count_route: pure host code) and the launchers the
// driver (count.hip) chains.  Kernels: count_wave.hip, count_slots.hip.
#pragma once
#include "phk_common.h"

// Control block of a call (uint32 words; the count kernels take a pointer to word 0 as `long_count`); what fills it:
// phk_count_plan_kernel, count_slots.hip
#define SORT_KEYS 2048
#define CTL_LONG 0      // hand-over items appended by the slot kernels (contigs >> mean, in pieces)
#define CTL_ITEMS 1     // work items of a sorted batch
#define CTL_STATS 2     // two uint64: padded windows, counted windows
#define CTL_TICKET 6
#define CTL_CURSOR 16   // SORT_KEYS words: key histogram, then the scatter's cursors
#define CTL_WORDS (16 + SORT_KEYS)
#define PLAN_PER_BLOCK 2048   // contigs per block and round (a multiple of 32: groups never straddle blocks)
#define COUNT_PIECE_W 32768u  // windows per piece of a contig that a sorted batch cuts up

// Batch statistics for the slot kernel's stand-down rule.  A slot workgroup runs as many 1024-window stages
// as the longest of its 32 contigs needs; stats[0] = sum over groups of 32 x that padded maximum, stats[1] =
// windows actually counted.  Below 60 % the wave-per-contig kernel is the faster one and takes the whole batch.
__device__ __forceinline__ bool phk_slots_apply(const unsigned long long *stats) { return stats[1] * 10ull >= stats[0] * 6ull; }

// key of a work item of w windows (the counting sort of ragged batches, count_slots.hip)
__device__ __forceinline__ uint32_t phk_windows_key(uint64_t w) {
    const uint64_t key = (w + 1023) >> 10;
    return (uint32_t)(key < SORT_KEYS - 1 ? key : SORT_KEYS - 1);
}
// windows of contig c and the number of items it is cut into (1: counted whole)
__device__ __forceinline__ uint64_t phk_contig_windows(const uint64_t *offsets, uint64_t c, int k, uint32_t long_thr,
                                                       uint32_t piece_w, uint32_t &pieces) {
    const uint64_t len = offsets[c + 1] - offsets[c];
    const uint64_t w = len >= (uint64_t)k ? len - k + 1 : 0;
    pieces = (w > long_thr && piece_w) ? (uint32_t)((w + piece_w - 1) / piece_w) : 1u;
    return w;
}
// windows of piece pc of a contig of w windows cut into `pieces`
__device__ __forceinline__ uint64_t phk_piece_windows(uint64_t w, uint32_t pieces, uint32_t pc, uint32_t piece_w) {
    if (pieces == 1) return w;
    return pc + 1 < pieces ? (uint64_t)piece_w : w - (uint64_t)(pieces - 1) * piece_w;
}
// LDS-only workgroup barrier: waits for this wave's LDS operations, NOT for its global loads
__device__ __forceinline__ void phk_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Workgroups of `lds` bytes a CU holds: by the 160 KiB of LDS less `reserve`, `cap` at the most, one at the least.
static inline unsigned phk_wgs_per_cu(size_t lds, unsigned reserve, unsigned cap) {
    const unsigned fit = (unsigned)((160u * 1024u - reserve) / lds);
    return fit > cap ? cap : (fit < 1 ? 1 : fit);
}
// grid of a kernel that walks `groups` work groups with `per_cu` workgroups resident per CU
static inline unsigned phk_count_grid(const phk_ctx *ctx, uint64_t groups, unsigned per_cu) {
    const uint64_t cap = (uint64_t)ctx->num_cus * per_cu;
    return (unsigned)(groups > cap ? cap : groups);
}

// The route of one phk_launch_count call: everything the launches need, decided on the host before the first of them.
// Without `slot_path` the call is ONE launch of the wave-per-contig kernel (no list, no plan kernel, no workspace) and
// the fields after max_word stay zero.
struct CountRoute {
    int k = 0;
    bool masked = false;
    uint64_t n = 0;
    uint64_t max_word = 0;       // last word holding a base; word max_word + 1 exists (pad)
    bool slot_path = false;      // 3 <= k <= 5, more than 1024 bases, n < 2^32, not count_lanes 0, dynamic LDS at address 0
    uint32_t slots = 0;          // contigs per slot workgroup: 16 at k = 5, else 32
    bool forced = false;         // count_lanes f q Q: the plan kernel sees no contig, so the statistics stand nothing down
    bool sorted = false;         // count_sort and not forced: the sort-scatter kernel and the ordered instances are launched
    uint32_t piece_w = 0;        // COUNT_PIECE_W if sorted: contigs above long_thr are counted in pieces of this many windows
    uint32_t long_thr = 0;       // windows above which a contig leaves the slot kernels
    uint64_t max_items = 0;      // bound on the work items (contigs + pieces): what WS_LONG is sized by
    uint64_t plan_n = 0;         // the plan kernel's `n` (0 when forced)
    unsigned plan_blocks = 0, sort_blocks = 0;          // grids of 256 threads; sort_blocks 0: not launched
    unsigned pairs_threads = 0, pairs_per_cu = 0;       // the two-windows-per-add kernel; threads 0: not launched
    size_t pairs_lds = 0;
    bool skip_plain = false;     // the pairs kernel counts the batches the statistics do not call ragged
    unsigned direct_threads = 0, direct_per_cu = 0;
    size_t direct_lds = 0;
    uint64_t pairs_groups = 0, direct_groups = 0;       // workgroup-sized groups each kernel walks (its grid: phk_count_grid)
};

static inline unsigned count_small_grid(uint64_t blocks) { return (unsigned)(blocks > 1024 ? 1024 : (blocks < 1 ? 1 : blocks)); }

// T > 0, n > 0.  mean_bases: the batch's mean contig length when the offsets address a sub-range of the stream, 0 = T / n.
static inline CountRoute count_route(const PhkKnobs &knobs, bool slots_lds0, int k, bool masked, uint64_t n, uint64_t T,
                                     uint64_t mean_bases) {
    const PhkCountLanes &lanes = knobs.count_lanes;
    CountRoute r;
    r.k = k;
    r.masked = masked;
    r.n = n;
    r.max_word = (T - 1) >> 4;
    r.slot_path = k >= 3 && k <= 5 && r.max_word >= 64 && n < (1ull << 32) && !lanes.wave_only && slots_lds0;
    if (!r.slot_path) return r;
    r.slots = k == 5 ? 16u : 32u;
    r.forced = lanes.forced;
    r.sorted = knobs.count_sort && !r.forced;
    // contigs much longer than the batch mean leave the slot kernels (a workgroup runs as many stages as its longest
    // contig): in a sorted batch as PIECES, each a work item of its own adding onto the zeroed row, so that one 500 kb
    // contig is shared by 15 columns or waves instead of pinning one
    r.piece_w = r.sorted ? COUNT_PIECE_W : 0u;
    uint64_t thr = 4 * ((mean_bases ? mean_bases : T / n) + 1) + 1024;
    if (r.sorted && thr < 2ull * r.piece_w) thr = 2ull * r.piece_w;
    r.long_thr = thr < 0xFFFFFFFFull ? (uint32_t)thr : 0xFFFFFFFFu;
    r.max_items = n + (r.piece_w ? T / r.piece_w : 0) + 16;
    r.plan_n = r.forced ? 0 : n;
    r.plan_blocks = count_small_grid(phk_div_up(r.forced ? 1 : n, PLAN_PER_BLOCK));
    r.sort_blocks = r.sorted ? count_small_grid(phk_div_up(n, 2048)) : 0u;
    if (k == 4 && !masked && lanes.pairs) {   // 2 workgroups per CU either way: 32 / 16 waves
        r.pairs_threads = lanes.pairs;
        r.pairs_lds = (size_t)512 * 32 * 4 + 32 * 4;
        r.pairs_per_cu = phk_wgs_per_cu(r.pairs_lds, 1024, 2048u / r.pairs_threads);
        r.pairs_groups = phk_div_up(n, 32);
        r.skip_plain = true;
    }
    // shapes, measured (1M contigs, ms): k = 3 unmasked 0.70 (slot kernel 0.79); k = 4 masked 1.00 with 512 threads, 1.22 with 1024
    // (slot kernel 1.13-1.15); k = 5 masked 2.68 with 1024 (slot kernel 3.87); ragged k = 4 / k = 5: 0.94 / 1.12 (0.92 / 1.58)
    r.direct_threads = (k == 3 || lanes.direct == 512 || (k == 4 && lanes.direct != 1024)) ? 512u : 1024u;
    r.direct_lds = (size_t)phk_pow4(k) * r.slots * 4 + 2 * r.slots * 4;
    r.direct_per_cu = phk_wgs_per_cu(r.direct_lds, 1024, 2048u / r.direct_threads);   // (at most 32 waves per CU)
    r.direct_groups = phk_div_up(r.sorted ? r.max_items : n, r.slots);
    return r;
}

// One call's device pointers: the caller's, and what the workspace stage carved out of WS_LONG and WS_CTL (slot path only).
struct CountCall {
    const uint32_t *packed = nullptr, *mask = nullptr;
    const uint64_t *offsets = nullptr;
    uint32_t *counts = nullptr, *nwin = nullptr;
    uint2 *long_list = nullptr;    // hand-over items (contig, piece) for the wave-per-contig kernel
    uint2 *order = nullptr;        // the sorted work items of a ragged batch; NULL unless the route is sorted
    uint32_t *ctl = nullptr, *ctl_next = nullptr;   // this call's control block and the next call's
};

// ---- launchers, one per kernel family; each launches what the route says and nothing else ----
// count_slots.hip
int phk_launch_count_plan(phk_ctx *ctx, const CountRoute &r, const CountCall &c, const PhkStepLink *link);
int phk_launch_sort_scatter(phk_ctx *ctx, const CountRoute &r, const CountCall &c);
int phk_launch_count_pairs(phk_ctx *ctx, const CountRoute &r, const CountCall &c);
// (sets link->prep8.written: it chooses the one kernel that writes the scorer's int8 operand)
int phk_launch_count_direct(phk_ctx *ctx, const CountRoute &r, const CountCall &c, PhkStepLink *link);
// count_wave.hip
int phk_launch_count_wave(phk_ctx *ctx, const CountRoute &r, const CountCall &c);
