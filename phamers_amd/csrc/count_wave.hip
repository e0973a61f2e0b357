// count_wave.hip -- the wave-per-contig count kernel and its launcher (gfx950).
//
// Replaces kmer.count_string's window loop (scripts/kmer.py:47-50).  Serves every k; after the slot kernels (count_slots.hip)
// it counts what they handed over.  Packed-stream layout: include/phamers_hip.h.
#include "count_shared.h"

// ------------------------------------------------------------------------------------
// count: one wavefront per contig; per-wave LDS histogram replicated over COPIES lanes
// ------------------------------------------------------------------------------------
// Lane l of a wave-iteration owns packed word w = w0 + l (16 window starts) and reads word
// w+1 for the K-1 bases a window may reach into; the 64-bit funnel X = w:w+1 makes window i
// the bit field X[63-2i .. 64-2K-2i], which IS the reference's bin index
// int(window, 4) (first base most significant, scripts/kmer.py:50).
//
// LDS layout per wave: lane l adds into copy l % COPIES of each bin, so the 32 lanes of an LDS
// group spread over COPIES banks per bin (random bins then collide ~2-way, which the 4-cycle
// ds_add data path hides).
//   PACK16 = false (k <= 4): bins[4^K][COPIES] uint32.
//   PACK16 = true  (k >= 5): rows[4^K/2][COPIES] uint32, row r = bins 2r (low half) and 2r+1 (high
//     half); at most 63 wave iterations (64512 windows) go between flushes, so no half can carry.
// A flush sums the copies with 16-byte LDS reads, clears them, and stores / accumulates uint32.
// atomic: the row receives the partial histograms of several pieces of one long contig (global atomic adds onto a
// zeroed row) instead of being stored
template <int K, int COPIES, bool PACK16>
__device__ __forceinline__ void phk_flush_bins(uint32_t *bins, uint32_t *row_out, bool first, int lane, bool atomic = false) {
    constexpr int D = 1 << (2 * K);
    constexpr int ROWS = PACK16 ? D / 2 : D;
    constexpr int W = ROWS * COPIES;        // dwords per wave
    constexpr int PER = PACK16 ? 2 : 1;     // output bins per row
    for (int base = 0; base < W; base += 256) {
        const int i4 = base + lane * 4;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i4 < W) {
            v = *reinterpret_cast<uint4 *>(bins + i4);
            *reinterpret_cast<uint4 *>(bins + i4) = make_uint4(0, 0, 0, 0);
        }
        if (COPIES >= 4) {  // 4 copies of one row per lane; COPIES/4 neighbouring lanes share the row
            uint32_t sum = v.x + v.y + v.z + v.w;
#pragma unroll
            for (int m = 1; m < COPIES / 4; m <<= 1) sum += __shfl_xor(sum, m);
            const int row = i4 / COPIES;
            if (i4 < W && (lane % (COPIES >= 4 ? COPIES / 4 : 1)) == 0) {
                uint32_t *dst = row_out + PER * row;
                if (atomic) {   // consecutive lanes hold consecutive rows: one wave instruction adds a contiguous run
                    if (PACK16) {
                        if (sum & 0xFFFFu) atomicAdd(dst, sum & 0xFFFFu);
                        if (sum >> 16) atomicAdd(dst + 1, sum >> 16);
                    } else if (sum) {
                        atomicAdd(dst, sum);
                    }
                } else if (PACK16) {
                    uint2 o = make_uint2(sum & 0xFFFFu, sum >> 16);
                    if (!first) {
                        const uint2 old = *reinterpret_cast<uint2 *>(dst);
                        o.x += old.x;
                        o.y += old.y;
                    }
                    *reinterpret_cast<uint2 *>(dst) = o;
                } else {
                    *dst = first ? sum : *dst + sum;
                }
            }
        } else if (!PACK16) {  // COPIES 1 or 2, plain uint32 bins: 4 or 2 bins per lane
            if (i4 < W && atomic) {
                if (COPIES == 1) {
                    const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (vv[e]) atomicAdd(row_out + i4 + e, vv[e]);
                } else {
                    if (v.x + v.y) atomicAdd(row_out + i4 / 2, v.x + v.y);
                    if (v.z + v.w) atomicAdd(row_out + i4 / 2 + 1, v.z + v.w);
                }
            } else if (i4 < W) {
                if (COPIES == 1) {
                    uint4 *dst = reinterpret_cast<uint4 *>(row_out + i4);
                    if (!first) {
                        const uint4 o = *dst;
                        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                    }
                    *dst = v;
                } else {
                    uint2 o = make_uint2(v.x + v.y, v.z + v.w);
                    uint2 *dst = reinterpret_cast<uint2 *>(row_out + i4 / 2);
                    if (!first) {
                        const uint2 old = *dst;
                        o.x += old.x; o.y += old.y;
                    }
                    *dst = o;
                }
            }
        } else {  // COPIES == 1 (k = 7, PACK16): four rows per lane -> bins 2*i4 .. 2*i4+7
            if (i4 < W && atomic) {
                const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (vv[e] & 0xFFFFu) atomicAdd(row_out + 2 * (i4 + e), vv[e] & 0xFFFFu);
                    if (vv[e] >> 16) atomicAdd(row_out + 2 * (i4 + e) + 1, vv[e] >> 16);
                }
            } else if (i4 < W) {
                uint4 o0 = make_uint4(v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16);
                uint4 o1 = make_uint4(v.z & 0xFFFFu, v.z >> 16, v.w & 0xFFFFu, v.w >> 16);
                uint4 *dst = reinterpret_cast<uint4 *>(row_out + 2 * i4);
                if (!first) {
                    const uint4 a0 = dst[0], a1 = dst[1];
                    o0.x += a0.x; o0.y += a0.y; o0.z += a0.z; o0.w += a0.w;
                    o1.x += a1.x; o1.y += a1.y; o1.z += a1.z; o1.w += a1.w;
                }
                dst[0] = o0;
                dst[1] = o1;
            }
        }
    }
}

// one wave-iteration: 16 window starts per lane from the funnel a:b of packed word wc
template <int K, int COPIES, bool PACK16, bool MASK>
__device__ __forceinline__ uint32_t phk_count_word(uint32_t *mybins, uint32_t a, uint32_t b, bool active, uint64_t wc,
                                                   uint64_t start, uint64_t last,
                                                   const uint32_t *__restrict__ mask) {
    constexpr uint32_t D = 1u << (2 * K);
    constexpr int LOGC = COPIES == 16 ? 4 : COPIES == 8 ? 3 : COPIES == 4 ? 2 : COPIES == 2 ? 1 : 0;
    const uint64_t X = ((uint64_t)a << 32) | b;
    const uint64_t g0 = wc << 4;
    // window starts i in [lo, hi] of this word belong to the contig
    const int lo = start > g0 ? (int)(start - g0) : 0;
    const int hi = last - g0 < 15 ? (int)(last - g0) : 15;
    uint32_t okbits = active ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;  // bit i = window i counted
    if (MASK) {
        const uint64_t mi = wc >> 1;
        const uint64_t V = ((uint64_t)mask[mi] << 32) | mask[mi + 1];
        const uint32_t vb = (uint32_t)(V >> (32 - 16 * (int)(wc & 1)));  // bit 31-i = base g0+i valid
        // window i is valid iff bases i .. i+K-1 are: AND the K shifted copies
        uint32_t wv = vb;
#pragma unroll
        for (int j = 1; j < K; ++j) wv &= vb << j;  // bit 31-i = window i valid
        okbits &= __brev(wv);
    }
    if (!MASK && __all(okbits == 0xFFFFu)) {
        // every lane holds 16 counted windows: no predicates at all
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t idx = (uint32_t)(X >> (64 - 2 * K - 2 * i)) & (D - 1);
            if (PACK16)
                atomicAdd(mybins + ((idx >> 1) << LOGC), 1u + __umul24(idx & 1u, 0xFFFFu));
            else
                atomicAdd(mybins + (idx << LOGC), 1u);
        }
        return 16;
    }
    // edge / masked words: uncounted windows add 0 (no exec-mask churn)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t idx = (uint32_t)(X >> (64 - 2 * K - 2 * i)) & (D - 1);
        const uint32_t ok = (okbits >> i) & 1u;
        if (PACK16)
            atomicAdd(mybins + ((idx >> 1) << LOGC), ok + __umul24(ok & idx, 0xFFFFu));
        else
            atomicAdd(mybins + (idx << LOGC), ok);
    }
    return __popc(okbits);
}

// The kernel is latency-bound unless loads run ahead of the LDS work, so it is software pipelined
// at the contig level: offsets are fetched two contigs ahead, the first PF wave-iterations of
// packed words one contig ahead (a register ring; longer contigs refill the ring as they go).
template <int K, int COPIES, bool PACK16, bool MASK>
__global__ __launch_bounds__(256) void phk_count_kernel(const uint32_t *__restrict__ packed,
                                                        const uint32_t *__restrict__ mask,
                                                        const uint64_t *__restrict__ offsets,
                                                        uint64_t n, uint64_t max_word,
                                                        uint32_t *__restrict__ counts,
                                                        uint32_t *__restrict__ nwin,
                                                        const uint2 *__restrict__ list,
                                                        const uint32_t *__restrict__ list_count,
                                                        uint32_t piece_w) {
    static_assert(COPIES >= 4 || !PACK16 || COPIES == 1, "unsupported replication");
    // with `list`: count the work items list[0 .. *list_count) the slot kernel handed over, item = (contig, piece):
    // the windows [piece * piece_w, (piece + 1) * piece_w) of the contig, added atomically onto its zeroed row
    // (piece_w == 0: whole contigs, stored).  Legacy stand-down (count_sort off): when the batch statistics behind
    // list_count say the slot kernel stood down (ragged batch), everything is counted here instead.
    const bool pieces = list && piece_w != 0;
    if (list && (pieces || phk_slots_apply(reinterpret_cast<const unsigned long long *>(list_count + CTL_STATS)))) n = *list_count;
    else list = nullptr;
    auto cid = [&](uint64_t i) { return list ? (uint64_t)list[i].x : i; };
    // stream range [s, e) whose windows item i counts (a window is identified by its first base)
    auto bounds = [&](uint64_t i, uint64_t &s, uint64_t &e) {
        const uint64_t c = cid(i);
        s = offsets[c];
        e = offsets[c + 1];
        if (pieces) {
            s += (uint64_t)list[i].y * piece_w;
            const uint64_t pe = s + piece_w + (K - 1);
            e = pe < e ? pe : e;
        }
    };
    constexpr uint32_t D = 1u << (2 * K);
    constexpr int W = (int)(PACK16 ? D / 2 : D) * COPIES;
    constexpr int SEG_ITERS = 63;  // wave iterations between flushes (PACK16 carry bound)
    constexpr int PF = 5;          // prefetched wave-iterations (5120 bases) per contig
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wpb = blockDim.x >> 6;
    uint32_t *bins = lds + (size_t)wave * W;
    for (int b = lane * 4; b < W; b += 256) *reinterpret_cast<uint4 *>(bins + b) = make_uint4(0, 0, 0, 0);
    uint32_t *mybins = bins + (lane & (COPIES - 1));  // this lane's copy

    const uint64_t S = (uint64_t)gridDim.x * wpb;
    uint64_t c = (uint64_t)blockIdx.x * wpb + wave;
    if (c >= n) return;

    uint32_t ra[PF], rb[PF], na[PF], nb[PF];
    // words of wave-iterations 0..PF-1 of contig [st, en) into (xa, xb).  The loads are
    // UNCONDITIONAL (indices clamped into the stream) so that they issue back to back: a load under
    // its own branch gets a vmcnt(0) at the join and the prefetch degenerates into serial round trips.
    auto issue = [&](uint64_t st, uint64_t en, uint32_t (&xa)[PF], uint32_t (&xb)[PF]) {
        const uint64_t wb = st >> 4;
        uint64_t we = en >= st + K ? (en - K) >> 4 : wb;
        we = we < max_word ? we : max_word;
#pragma unroll
        for (int t = 0; t < PF; ++t) {
            const uint64_t w = wb + 64ull * t + lane;
            const uint64_t wc = w <= we ? w : we;
            xa[t] = packed[wc];
            xb[t] = packed[wc + 1];
        }
    };
    // count one contig whose first PF iterations sit in (xa, xb); later iterations (contigs longer
    // than 1024*PF bases) are loaded as they come
    auto process = [&](uint64_t cc, uint64_t start, uint64_t end, uint32_t (&xa)[PF], uint32_t (&xb)[PF]) {
        uint32_t *row_out = counts + cc * D;
        uint32_t cnt = 0;
        bool first = true;
        if (end >= start + K) {
            const uint64_t last = end - K;  // last window start
            const uint64_t wb = start >> 4, we = last >> 4;
            const uint64_t niter = (we - wb) / 64 + 1;
            int since_flush = 0;
            for (uint64_t t = 0; t < niter; ++t) {
                const uint64_t w = wb + 64 * t + lane;
                const bool active = w <= we;
                const uint64_t wc = active ? w : we;
                uint32_t a, b;
                if (t < PF) {  // wave-uniform: pick ring slot t (select chain keeps the ring in registers)
                    a = xa[0];
                    b = xb[0];
#pragma unroll
                    for (int j = 1; j < PF; ++j) {
                        a = (t == (uint64_t)j) ? xa[j] : a;
                        b = (t == (uint64_t)j) ? xb[j] : b;
                    }
                } else {
                    a = packed[wc];
                    b = packed[wc + 1];
                }
                cnt += phk_count_word<K, COPIES, PACK16, MASK>(mybins, a, b, active, wc, start, last, mask);
                if (++since_flush == SEG_ITERS && t + 1 < niter) {  // keep 16-bit halves from carrying
                    phk_flush_bins<K, COPIES, PACK16>(bins, row_out, first, lane, pieces);
                    first = false;
                    since_flush = 0;
                }
            }
        }
        phk_flush_bins<K, COPIES, PACK16>(bins, row_out, first, lane, pieces);
        if (nwin) {
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
            if (lane == 0) {
                if (pieces) { if (cnt) atomicAdd(nwin + cc, cnt); }
                else nwin[cc] = cnt;
            }
        }
    };

    // two rings in ping-pong: while item c is counted out of one, item c+S streams into the other
    uint64_t s0, e0;
    bounds(c, s0, e0);
    uint64_t s1 = 0, e1 = 0;
    if (c + S < n) bounds(c + S, s1, e1);
    issue(s0, e0, ra, rb);
    for (;;) {
        // --- even phase: process (s0,e0) from ra/rb, stream item c+S into na/nb
        uint64_t s2 = 0, e2 = 0;
        if (c + 2 * S < n) bounds(c + 2 * S, s2, e2);
        if (c + S < n) issue(s1, e1, na, nb);
        process(cid(c), s0, e0, ra, rb);
        c += S;
        if (c >= n) break;
        // --- odd phase: process (s1,e1) from na/nb, stream item c+S into ra/rb
        uint64_t s3 = 0, e3 = 0;
        if (c + 2 * S < n) bounds(c + 2 * S, s3, e3);
        if (c + S < n) issue(s2, e2, ra, rb);
        process(cid(c), s1, e1, na, nb);
        c += S;
        if (c >= n) break;
        s0 = s2; e0 = e2;
        s1 = s3; e1 = e3;
    }
}

// replication / packing per k: keep a wave's bins <= 32 KiB
template <int K> struct PhkCountCfg {
    static constexpr bool pack16 = K >= 6;
    static constexpr int copies = K <= 4 ? 4 : 1;  // measured best, profiles/r01/count_lds_study.md
};

template <int K>
static int launch_count_wave(phk_ctx *ctx, const CountRoute &r, const CountCall &c) {
    constexpr int COPIES = PhkCountCfg<K>::copies;
    constexpr bool P16 = PhkCountCfg<K>::pack16;
    constexpr uint32_t D = 1u << (2 * K);
    constexpr size_t wave_bytes = (size_t)(P16 ? D / 2 : D) * COPIES * 4u;
    // waves per block so that a block's bins stay <= 64 KiB
    const int wpb = wave_bytes * 4 <= 65536 ? 4 : (wave_bytes * 2 <= 65536 ? 2 : 1);
    const size_t lds = wave_bytes * wpb;
    const unsigned blocks = phk_count_grid(ctx, phk_div_up(r.n, wpb), phk_wgs_per_cu(lds, 0, 8));
    if (blocks == 0) return PHK_OK;
    // after the slot kernels: the hand-over list, its count (word CTL_LONG of the control block) and the piece width
    if (c.mask) {
        PHK_LAUNCH(ctx, "phk_count_kernel",
                   phk_count_kernel<K, COPIES, P16, true><<<dim3(blocks), dim3(64 * wpb), lds, ctx->stream>>>(
                       c.packed, c.mask, c.offsets, r.n, r.max_word, c.counts, c.nwin, c.long_list, c.ctl, r.piece_w));
    } else {
        PHK_LAUNCH(ctx, "phk_count_kernel",
                   phk_count_kernel<K, COPIES, P16, false><<<dim3(blocks), dim3(64 * wpb), lds, ctx->stream>>>(
                       c.packed, c.mask, c.offsets, r.n, r.max_word, c.counts, c.nwin, c.long_list, c.ctl, r.piece_w));
    }
    return PHK_OK;
}

// (the replication / packing of a k was settled by the LDS study of round 1, profiles/r01/count_lds_study.md; the knob that
// selected other built variants -- 60 kernel instances -- is gone since round 5)
int phk_launch_count_wave(phk_ctx *ctx, const CountRoute &r, const CountCall &c) {
    switch (r.k) {
        case 1: return launch_count_wave<1>(ctx, r, c);
        case 2: return launch_count_wave<2>(ctx, r, c);
        case 3: return launch_count_wave<3>(ctx, r, c);
        case 4: return launch_count_wave<4>(ctx, r, c);
        case 5: return launch_count_wave<5>(ctx, r, c);
        case 6: return launch_count_wave<6>(ctx, r, c);
        default: return launch_count_wave<7>(ctx, r, c);
    }
}
