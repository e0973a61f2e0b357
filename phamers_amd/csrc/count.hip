// count.hip -- the driver of per-contig 4^k histograms: route -> workspace -> launches.  It holds no kernel: the
// wave-per-contig kernel is in count_wave.hip, the slot kernels with their plan and sort kernels in count_slots.hip, and
// the route (count_route, pure host code) with everything the units share in count_shared.h.
//
// Replaces kmer.count_string's window loop (scripts/kmer.py:47-50).  Packed-stream layout: include/phamers_hip.h.
#include "count_shared.h"

// Workspace of a slot-path call: hand-over items (contig, piece) and the sorted work items in WS_LONG, then the control
// block (CTL_* words, count_shared.h) in WS_CTL.  WS_CTL holds TWO blocks used in turn (ctl_epoch's parity picks this
// call's): the plan kernel of a call zeroes the block of the next, so no launch is preceded by a memset -- except after
// a call that failed half way, or when the allocation moved.  From here until count_ctl_done the blocks count as dirty.
static int count_workspace(phk_ctx *ctx, const CountRoute &r, CountCall &c) {
    void *ws, *ctlv;
    PHK_TRY(phk_ws(ctx, WS_LONG, (4 * r.max_items + 16) * sizeof(uint32_t), &ws));
    PHK_TRY(phk_ws(ctx, WS_CTL, 2 * CTL_WORDS * sizeof(uint32_t), &ctlv));
    if (ctx->ctl_dirty || ctx->ctl_gen != ctx->ws[WS_CTL].gen) {
        PHK_HIP(hipMemsetAsync(ctlv, 0, 2 * CTL_WORDS * sizeof(uint32_t), ctx->stream));
        ctx->ctl_gen = ctx->ws[WS_CTL].gen;
    }
    ctx->ctl_dirty = true;
    c.ctl = (uint32_t *)ctlv + (ctx->ctl_epoch & 1) * CTL_WORDS;
    c.ctl_next = (uint32_t *)ctlv + ((ctx->ctl_epoch + 1) & 1) * CTL_WORDS;
    c.long_list = (uint2 *)ws;
    c.order = r.sorted ? (uint2 *)((uint32_t *)ws + 2 * r.max_items) : nullptr;
    return PHK_OK;
}
// every launch of the call is out: the next call finds the block its plan kernel zeroed
static void count_ctl_done(phk_ctx *ctx) { ctx->ctl_dirty = false; }

// The slot path's chain: plan, [sort-scatter], [pairs], direct (0 - 2 instances), wave-per-contig with the hand-over list.
static int count_slot_launches(phk_ctx *ctx, const CountRoute &r, const CountCall &c, PhkStepLink *link) {
    PHK_TRY(phk_launch_count_plan(ctx, r, c, link));
    ctx->ctl_epoch += 1;               // (the block that kernel zeroes is the next call's)
    if (link) link->planned = true;    // (the words a caller's next stage wanted zeroed, see PhkStepLink)
    if (r.sorted) PHK_TRY(phk_launch_sort_scatter(ctx, r, c));
    if (r.pairs_threads) PHK_TRY(phk_launch_count_pairs(ctx, r, c));
    PHK_TRY(phk_launch_count_direct(ctx, r, c, link));
    return phk_launch_count_wave(ctx, r, c);
}

// mean_bases: the batch's mean contig length when `d_offsets` addresses a sub-range of the stream (T then only bounds
// the loads); 0 = T / n
int phk_launch_count(phk_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t T,
                     const uint64_t *d_offsets, uint64_t n, int k, uint32_t *d_counts,
                     uint32_t *d_nwin, uint64_t mean_bases, PhkStepLink *link) {
    PHK_REQUIRE(k >= 1, "phk_count: k must be >= 1 (got %d)", k);
    if (k > PHK_MAX_K) {
        phk_set_error("phk_count: k=%d is above PHK_MAX_K=%d (4^k bins no longer fit LDS)", k, PHK_MAX_K);
        return PHK_ERR_UNSUPPORTED;
    }
    if (n == 0) return PHK_OK;
    PHK_REQUIRE(d_packed && d_offsets && d_counts, "phk_count: NULL device pointer");
    PHK_REQUIRE(((uintptr_t)d_counts & 15) == 0, "phk_count: counts must be 16-byte aligned");
    if (T == 0) {  // only empty contigs: all-zero rows, nothing to read
        PHK_HIP(hipMemsetAsync(d_counts, 0, n * phk_pow4(k) * sizeof(uint32_t), ctx->stream));
        if (d_nwin) PHK_HIP(hipMemsetAsync(d_nwin, 0, n * sizeof(uint32_t), ctx->stream));
        return PHK_OK;
    }
    const CountRoute r = count_route(ctx->knobs, ctx->slots_lds0, k, d_mask != nullptr, n, T, mean_bases);
    CountCall c{d_packed, d_mask, d_offsets, d_counts, d_nwin};
    if (!r.slot_path) return phk_launch_count_wave(ctx, r, c);
    PHK_TRY(count_workspace(ctx, r, c));
    PHK_TRY(count_slot_launches(ctx, r, c, link));
    count_ctl_done(ctx);
    return PHK_OK;
}
