// windows.hip -- sliding-window k-mer counts along sequences: the rows of a phk_batch are the overlapping windows
// [jS, jS + W) of every sequence of a batch (kmer.count_windows, phamers_amd/windows.py).
//
// A window differs from its predecessor by S k-mer starts entering at the front and S leaving at the back, so the kernels
// keep ONE running histogram per walker in LDS, add at a leading cursor, subtract at a trailing cursor, and emit a row
// after every step: every base is touched twice whatever W / S is, and no base is uploaded or packed more than once.
// The unit of work is a SEGMENT of consecutive windows of one sequence (PhkWinSeg): its first window is counted in full
// (the warm-up), every later one is derived.  When S >= W - k + 1 consecutive windows share no k-mer and every window is
// simply counted.  DESIGN.md section 4.12.
#include <string.h>

#include <vector>

#include "phk_common.h"

// ---- launch constants (phk_windows_grid_pass reports them to the tests) ----
#define PHK_WIN_SLOTS 32              // segments (histogram columns) per wave of the k = 4 kernel
#define PHK_WIN_LANE_BLOCKS_MAX 1280  // k = 4: one-wave workgroups per launch (5 x 32 KiB of LDS per CU x 256 CUs), grid-stride beyond
#define PHK_WIN_WAVE_BLOCKS_MAX 2048  // other k: workgroups per launch, one segment per wave
#define PHK_WIN_SEGMENT_MAX 4096      // windows per segment at most (automatic choice)

struct PhkWinSeg {
    uint64_t pos;   // first k-mer start of the segment's first window, in bases of the packed stream
    uint64_t row;   // output row of that window
    uint32_t nw;    // windows of the segment
    uint32_t pad;
};

// LDS operations of one wave are executed in order; this only keeps the compiler from moving them across the point where
// the lanes of a wave hand data to each other through LDS
__device__ __forceinline__ void win_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bit i = the k-mer starting at base 16 w + i is counted: inside [lo, hi) and, with a mask, free of invalid bases
template <bool MASK>
__device__ __forceinline__ uint32_t win_okbits(const uint32_t *__restrict__ mask, uint64_t w, uint64_t lo, uint64_t hi, bool act, int K) {
    const uint64_t g0 = w << 4;
    const int li = lo > g0 ? (int)(lo - g0) : 0;
    const int hi_i = hi - 1 - g0 < 15 ? (int)(hi - 1 - g0) : 15;
    uint32_t ok = act ? ((2u << hi_i) - 1u) & ~((1u << li) - 1u) : 0u;
    if (MASK) {
        const uint64_t mi = w >> 1;
        const uint64_t V = ((uint64_t)mask[mi] << 32) | mask[mi + 1];
        const uint32_t vb = (uint32_t)(V >> (32 - 16 * (int)(w & 1)));   // bit 31 - i = base 16 w + i valid
        uint32_t wv = vb;
        for (int j = 1; j < K; ++j) wv &= vb << j;                        // bit 31 - i = k-mer i valid
        ok &= __brev(wv);
    }
    return ok;
}

// ------------------------------------------------------------------------------------
// k = 4: a lane PAIR walks its own segment.  bins[code][slot]: the LDS bank of an add is its slot, so the
// 32 columns never conflict; lane l < 32 is the leading cursor of slot l (adds), lane l + 32 the trailing cursor of the
// same slot (subtracts: an add of 2^32 - 1) -- the two halves of a wave are separate LDS lane groups.  During the warm-up
// the two lanes count one half of the first window each.  After every step the wave flushes the 32 columns together.
// ------------------------------------------------------------------------------------
template <bool MASK>
__device__ __forceinline__ int win_walk4(uint32_t *col, const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask,
                                         uint64_t wlast, uint64_t lo, uint64_t hi, uint32_t delta) {
    bool act = hi > lo;
    uint64_t w = act ? lo >> 4 : 0;
    const uint64_t we = act ? (hi - 1) >> 4 : 0;
    // the words are loaded one iteration ahead of their use (indices clamped to the stream's pad word: loads unconditional)
    uint32_t a = packed[w], b = packed[w + 1 < wlast ? w + 1 : wlast];
    int cnt = 0;
    while (__any(act)) {
        const uint32_t nx = packed[w + 2 < wlast ? w + 2 : wlast];
        const uint32_t ok = win_okbits<MASK>(mask, w, lo, hi, act, 4);
        const uint64_t X = ((uint64_t)a << 32) | b;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t idx = (uint32_t)(X >> (56 - 2 * i)) & 255u;
            atomicAdd(col + idx * PHK_WIN_SLOTS, (0u - ((ok >> i) & 1u)) & delta);
        }
        cnt += __popc(ok);
        a = b;
        b = nx;
        act = act && w < we;   // (w never passes the lane's last word: the mask words of a later one need not exist)
        if (act) ++w;
    }
    return delta == 1u ? cnt : -cnt;
}

// The 32 columns -> 32 rows.  Lane (q = lane & 7, g = lane >> 3) reads, per round, four codes x four slots (4q .. 4q + 3)
// with 16-byte LDS reads and stores, per slot, the four codes with one 16-byte store: lanes of equal q write 128
// contiguous bytes of a row.  A lane's four codes start at a multiple of four, i.e. at an even bin row, so the 16 lanes of
// a ds_read_b128 group would meet on 8 of its 16 bank quads; odd g read their codes pairwise swapped (and swap back in
// registers), which spreads a group over all 64 banks.
__device__ __forceinline__ void win_flush4(uint32_t *bins, const unsigned long long *rows_s, uint32_t *__restrict__ counts,
                                           int lane, bool clear) {
    const int q = lane & 7, g = lane >> 3;
    const bool sw = g & 1;
    unsigned long long r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = rows_s[4 * q + i];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int c0 = 4 * (8 * t + g);
        uint4 R[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 *p = reinterpret_cast<uint4 *>(bins + (c0 + (j ^ (int)sw)) * PHK_WIN_SLOTS + 4 * q);
            R[j] = *p;
            if (clear) *p = make_uint4(0, 0, 0, 0);
        }
        // code c0 + j is in R[j ^ sw]
        uint4 A[4];
        A[0].x = sw ? R[1].x : R[0].x; A[0].y = sw ? R[1].y : R[0].y; A[0].z = sw ? R[1].z : R[0].z; A[0].w = sw ? R[1].w : R[0].w;
        A[1].x = sw ? R[0].x : R[1].x; A[1].y = sw ? R[0].y : R[1].y; A[1].z = sw ? R[0].z : R[1].z; A[1].w = sw ? R[0].w : R[1].w;
        A[2].x = sw ? R[3].x : R[2].x; A[2].y = sw ? R[3].y : R[2].y; A[2].z = sw ? R[3].z : R[2].z; A[2].w = sw ? R[3].w : R[2].w;
        A[3].x = sw ? R[2].x : R[3].x; A[3].y = sw ? R[2].y : R[3].y; A[3].z = sw ? R[2].z : R[3].z; A[3].w = sw ? R[2].w : R[3].w;
        if (r[0] != ~0ull) *reinterpret_cast<uint4 *>(counts + r[0] * 256 + c0) = make_uint4(A[0].x, A[1].x, A[2].x, A[3].x);
        if (r[1] != ~0ull) *reinterpret_cast<uint4 *>(counts + r[1] * 256 + c0) = make_uint4(A[0].y, A[1].y, A[2].y, A[3].y);
        if (r[2] != ~0ull) *reinterpret_cast<uint4 *>(counts + r[2] * 256 + c0) = make_uint4(A[0].z, A[1].z, A[2].z, A[3].z);
        if (r[3] != ~0ull) *reinterpret_cast<uint4 *>(counts + r[3] * 256 + c0) = make_uint4(A[0].w, A[1].w, A[2].w, A[3].w);
    }
}

template <bool MASK>
__global__ __launch_bounds__(64) void phk_windows_lanes_kernel(const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask,
                                                              uint64_t wlast, const PhkWinSeg *__restrict__ segs, uint64_t nseg,
                                                              uint32_t nk,   // k-mer starts per window, W - k + 1
                                                              uint64_t S, int overlap, uint32_t *__restrict__ counts,
                                                              uint32_t *__restrict__ nwin) {
    __shared__ __attribute__((aligned(16))) uint32_t bins[256 * PHK_WIN_SLOTS];
    __shared__ unsigned long long rows_s[PHK_WIN_SLOTS];
    const int lane = threadIdx.x;
    const int slot = lane & (PHK_WIN_SLOTS - 1), half = lane >> 5;
    for (int b = lane * 4; b < 256 * PHK_WIN_SLOTS; b += 256) *reinterpret_cast<uint4 *>(bins + b) = make_uint4(0, 0, 0, 0);
    win_wave_sync();
    uint32_t *col = bins + slot;
    for (uint64_t batch = blockIdx.x; batch * PHK_WIN_SLOTS < nseg; batch += gridDim.x) {
        const uint64_t si = batch * PHK_WIN_SLOTS + slot;
        const bool have = si < nseg;
        const uint64_t pos = have ? segs[si].pos : 0, row0 = have ? segs[si].row : 0;
        const uint32_t nw = have ? segs[si].nw : 0;
        uint32_t maxnw = nw;
#pragma unroll
        for (int sh = 16; sh > 0; sh >>= 1) {
            const uint32_t o = __shfl_xor(maxnw, sh);
            maxnw = o > maxnw ? o : maxnw;
        }
        int cnt = 0;
        for (uint32_t j = 0; j < maxnw; ++j) {
            const bool live = j < nw;
            const uint64_t p = pos + (uint64_t)j * S;   // the window's first k-mer start
            uint64_t lo = 0, hi = 0;
            uint32_t delta = 1u;
            if (live) {
                if (j == 0 || !overlap) {               // the whole window, one half per lane of the pair
                    const uint64_t mid = p + nk / 2;
                    lo = half ? mid : p;
                    hi = half ? p + nk : mid;
                } else if (half) {                      // trailing cursor: the starts the previous window had and this one has not
                    lo = p - S;
                    hi = p;
                    delta = 0xFFFFFFFFu;
                } else {                                // leading cursor: the starts past the previous window's last
                    lo = p - S + nk;
                    hi = p + nk;
                }
            }
            cnt += win_walk4<MASK>(col, packed, mask, wlast, lo, hi, delta);
            const int total = cnt + __shfl_xor(cnt, 32);
            if (!half) {
                rows_s[slot] = live ? row0 + j : ~0ull;
                if (live) nwin[row0 + j] = (uint32_t)total;
            }
            win_wave_sync();
            // a finished segment's column stays as it is (its row is written no more) until the wave's last step clears all
            win_flush4(bins, rows_s, counts, lane, !overlap || j + 1 == maxnw);
            if (!overlap) cnt = 0;
            win_wave_sync();
        }
    }
}

// ------------------------------------------------------------------------------------
// every other k (1..3, 5..7): a wave per segment on one uint32 histogram of 4^k bins in LDS; the lanes of the wave share
// each cursor's words.  Simple rather than fast: a step costs the whole wave a flush of 4^k words.
// ------------------------------------------------------------------------------------
template <bool MASK>
__device__ __forceinline__ int win_wave_range(uint32_t *hist, const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask,
                                              uint64_t lo, uint64_t hi, uint32_t delta, int K, int lane) {
    if (hi <= lo) return 0;   // (wave-uniform)
    const uint32_t dmask = (1u << (2 * K)) - 1u;
    const uint64_t wlo = lo >> 4, whi = (hi - 1) >> 4;
    int cnt = 0;
    for (uint64_t wb = wlo; wb <= whi; wb += 64) {
        const uint64_t w = wb + lane;
        const bool act = w <= whi;
        const uint64_t wc = act ? w : whi;
        const uint32_t a = packed[wc], b = packed[wc + 1];
        const uint32_t ok = win_okbits<MASK>(mask, wc, lo, hi, act, K);
        const uint64_t X = ((uint64_t)a << 32) | b;
        if (ok) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t idx = (uint32_t)(X >> (64 - 2 * K - 2 * i)) & dmask;
                atomicAdd(hist + idx, (0u - ((ok >> i) & 1u)) & delta);
            }
        }
        cnt += __popc(ok);
    }
    return cnt;
}

template <bool MASK>
__global__ __launch_bounds__(256) void phk_windows_wave_kernel(const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask,
                                                              const PhkWinSeg *__restrict__ segs, uint64_t nseg, int K, uint32_t nk,
                                                              uint64_t S, int overlap, uint32_t *__restrict__ counts,
                                                              uint32_t *__restrict__ nwin) {
    extern __shared__ __attribute__((aligned(16))) uint32_t win_lds[];   // one histogram per wave
    const uint32_t D = 1u << (2 * K);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    uint32_t *hist = win_lds + (size_t)wave * D;
    for (uint32_t b = lane * 4; b < D; b += 256) *reinterpret_cast<uint4 *>(hist + b) = make_uint4(0, 0, 0, 0);
    win_wave_sync();
    for (uint64_t si = (uint64_t)blockIdx.x * wpb + wave; si < nseg; si += (uint64_t)gridDim.x * wpb) {
        const uint64_t pos = segs[si].pos, row0 = segs[si].row;
        const uint32_t nw = segs[si].nw;
        int cnt = 0;   // this lane's share of the running row sum
        for (uint32_t j = 0; j < nw; ++j) {
            const uint64_t p = pos + (uint64_t)j * S;
            if (j == 0 || !overlap) {
                cnt += win_wave_range<MASK>(hist, packed, mask, p, p + nk, 1u, K, lane);
            } else {
                cnt += win_wave_range<MASK>(hist, packed, mask, p - S + nk, p + nk, 1u, K, lane);
                cnt -= win_wave_range<MASK>(hist, packed, mask, p - S, p, 0xFFFFFFFFu, K, lane);
            }
            int total = cnt;
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) total += __shfl_xor(total, sh);
            win_wave_sync();
            const bool clear = !overlap || j + 1 == nw;
            uint32_t *row = counts + (row0 + j) * D;
            for (uint32_t b = lane * 4; b < D; b += 256) {
                uint4 *hp = reinterpret_cast<uint4 *>(hist + b);
                *reinterpret_cast<uint4 *>(row + b) = *hp;
                if (clear) *hp = make_uint4(0, 0, 0, 0);
            }
            if (lane == 0) nwin[row0 + j] = (uint32_t)total;
            if (!overlap) cnt = 0;
            win_wave_sync();
        }
    }
}

// ------------------------------------------------------------------------------------
// launch
// ------------------------------------------------------------------------------------
// windows of a sequence of `len` bases
static inline uint64_t win_rows_of(uint64_t len, uint64_t W, uint64_t S) { return len >= W ? (len - W) / S + 1 : 0; }

uint64_t phk_windows_rows(const uint64_t *offsets, uint64_t n, uint64_t W, uint64_t S) {
    uint64_t rows = 0;
    for (uint64_t c = 0; c < n; ++c) rows += win_rows_of(offsets[c + 1] - offsets[c], W, S);
    return rows;
}

// segments one launch takes in a single pass of its grid (more are taken by the grid-stride loops)
static uint64_t win_grid_pass(int k) {
    if (k == 4) return (uint64_t)PHK_WIN_LANE_BLOCKS_MAX * PHK_WIN_SLOTS;
    return (uint64_t)PHK_WIN_WAVE_BLOCKS_MAX * (k <= 6 ? 4 : 1);
}

extern "C" int phk_windows_grid_pass(int k, uint64_t *segments) {
    PHK_REQUIRE(segments && k >= 1 && k <= PHK_MAX_K, "phk_windows_grid_pass: bad argument");
    *segments = win_grid_pass(k);
    return PHK_OK;
}

// Windows per segment when the caller leaves the choice to the launch.  The warm-up of a segment repeats work a longer
// segment would have shared (W / (segment * S) of the cursor work), but a segment is walked by ONE lane pair (k = 4) or
// wave, so few long sequences need short segments to fill the machine: as many segments as four waves per CU can walk at
// once, longer ones only when there are more windows than that.
static uint32_t win_auto_segment(const phk_ctx *ctx, int k, uint64_t rows) {
    const uint64_t walkers = k == 4 ? (uint64_t)ctx->num_cus * 4 * PHK_WIN_SLOTS : (uint64_t)ctx->num_cus * 16;
    uint64_t g = phk_div_up(rows, walkers);
    g = g < 1 ? 1 : (g > PHK_WIN_SEGMENT_MAX ? PHK_WIN_SEGMENT_MAX : g);
    return (uint32_t)g;
}

// d_packed / d_mask (NULL: every base valid): the packed stream of the sequences `offsets` (host) describes;
// d_counts[rows][4^k], d_nwin[rows] with rows = phk_windows_rows(...) > 0.  Returns with the rows written.
int phk_launch_windows(phk_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t T, const uint64_t *offsets,
                       uint64_t n, int k, uint64_t W, uint64_t S, uint32_t segment, uint32_t *d_counts, uint32_t *d_nwin) {
    PHK_REQUIRE(k >= 1 && k <= PHK_MAX_K && W >= (uint64_t)k && S >= 1, "phk_windows: bad k / window / step");
    PHK_REQUIRE(W - k + 1 <= 0xFFFFFFFFull, "phk_windows: a window of %llu bases does not fit the 32-bit row sums", (unsigned long long)W);
    const uint64_t rows = phk_windows_rows(offsets, n, W, S);
    PHK_REQUIRE(rows > 0, "phk_windows: no sequence is as long as the window");
    const uint32_t nk = (uint32_t)(W - k + 1);
    const int overlap = S < nk ? 1 : 0;
    const uint32_t seg = segment ? segment : win_auto_segment(ctx, k, rows);
    std::vector<PhkWinSeg> segs;
    segs.reserve(rows / seg + n);
    uint64_t row = 0;
    for (uint64_t c = 0; c < n; ++c) {
        const uint64_t nw = win_rows_of(offsets[c + 1] - offsets[c], W, S);
        for (uint64_t j = 0; j < nw; j += seg) {
            PhkWinSeg s;
            s.pos = offsets[c] + j * S;
            s.row = row + j;
            s.nw = (uint32_t)(nw - j < seg ? nw - j : seg);
            s.pad = 0;
            segs.push_back(s);
        }
        row += nw;
    }
    const uint64_t nseg = segs.size();
    void *d_segs;
    PHK_TRY(phk_ws(ctx, WS_LONG, nseg * sizeof(PhkWinSeg), &d_segs));
    PHK_HIP(hipMemcpyAsync(d_segs, segs.data(), nseg * sizeof(PhkWinSeg), hipMemcpyHostToDevice, ctx->stream));
    const uint64_t wlast = phk_div_up(T, 16);   // the pad word: the last one that exists
    if (k == 4) {
        uint64_t blocks = phk_div_up(nseg, PHK_WIN_SLOTS);
        if (blocks > PHK_WIN_LANE_BLOCKS_MAX) blocks = PHK_WIN_LANE_BLOCKS_MAX;
        if (d_mask)
            PHK_LAUNCH(ctx, "phk_windows_lanes_kernel",
                       phk_windows_lanes_kernel<true><<<dim3((unsigned)blocks), dim3(64), 0, ctx->stream>>>(
                           d_packed, d_mask, wlast, (const PhkWinSeg *)d_segs, nseg, nk, S, overlap, d_counts, d_nwin));
        else
            PHK_LAUNCH(ctx, "phk_windows_lanes_kernel",
                       phk_windows_lanes_kernel<false><<<dim3((unsigned)blocks), dim3(64), 0, ctx->stream>>>(
                           d_packed, d_mask, wlast, (const PhkWinSeg *)d_segs, nseg, nk, S, overlap, d_counts, d_nwin));
    } else {
        const unsigned wpb = k <= 6 ? 4 : 1;   // 4^k words per wave: 64 KiB of dynamic LDS at most
        uint64_t blocks = phk_div_up(nseg, wpb);
        if (blocks > PHK_WIN_WAVE_BLOCKS_MAX) blocks = PHK_WIN_WAVE_BLOCKS_MAX;
        const size_t lds = (size_t)wpb * phk_pow4(k) * sizeof(uint32_t);
        if (d_mask)
            PHK_LAUNCH(ctx, "phk_windows_wave_kernel",
                       phk_windows_wave_kernel<true><<<dim3((unsigned)blocks), dim3(64 * wpb), lds, ctx->stream>>>(
                           d_packed, d_mask, (const PhkWinSeg *)d_segs, nseg, k, nk, S, overlap, d_counts, d_nwin));
        else
            PHK_LAUNCH(ctx, "phk_windows_wave_kernel",
                       phk_windows_wave_kernel<false><<<dim3((unsigned)blocks), dim3(64 * wpb), lds, ctx->stream>>>(
                           d_packed, d_mask, (const PhkWinSeg *)d_segs, nseg, k, nk, S, overlap, d_counts, d_nwin));
    }
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // (the segment table is a host vector)
    return PHK_OK;
}

// ------------------------------------------------------------------------------------
// C ABI: the windows of a batch of sequences as the rows of a phk_batch (ingest as phk_batch_from_ascii: batch.hip)
// ------------------------------------------------------------------------------------
static int windows_check(const char *fname, int k, uint64_t window, uint64_t step) {
    PHK_REQUIRE(k >= 1, "%s: k must be >= 1 (got %d)", fname, k);
    if (k > PHK_MAX_K) {
        phk_set_error("%s: k=%d is above PHK_MAX_K=%d", fname, k, PHK_MAX_K);
        return PHK_ERR_UNSUPPORTED;
    }
    PHK_REQUIRE(window >= (uint64_t)k, "%s: window %llu is shorter than k=%d", fname, (unsigned long long)window, k);
    PHK_REQUIRE(step >= 1, "%s: step must be >= 1", fname);
    return PHK_OK;
}

extern "C" int phk_batch_windows_from_ascii(phk_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n, int k,
                                            const char *symbols4, uint64_t window, uint64_t step, uint32_t segment,
                                            phk_batch **out) {
    PHK_ENTER(ctx, "phk_batch_windows_from_ascii");
    PHK_REQUIRE(out && offsets, "phk_batch_windows_from_ascii: NULL argument");
    PHK_TRY(windows_check("phk_batch_windows_from_ascii", k, window, step));
    const PhkWindowSpec spec = {window, step, segment};
    return phk_batch_build(ctx, bases, nullptr, offsets, n, k, symbols4, out, &spec);
}
