// evaluate.hip -- evaluation of score vectors on the device (gfx950): what PhaMers' scripts/learning.py:185-243 computes
// with scikit-learn's roc_curve / auc and NumPy comparisons, and the sort under it.
//   phk_argsort_f64 / _dev : the stable permutation that orders n float64 keys (least-significant-digit radix sort)
//   phk_roc_curve / _dev   : scikit-learn's roc_curve(..., drop_intermediate) in integers: fps, tps, thresholds, 2 P N AUC
//   phk_truth_counts       : tp, fp, fn, tn at a threshold (>= / <), one reduction
//   phk_compare_*          : C score vectors over the same rows: DeLong placements and Gram matrices, a stratified bootstrap
//                            (the last part of this file)
//
// The sort.  A key's IMAGE is the 64-bit integer that orders as the double does (-0.0 taken as +0.0 first:
// sign bit set -> all bits flipped, else sign bit flipped); a descending sort orders the complemented images, so ties stay
// in index order both ways.  Eight passes of 8-bit digits at most: the prepare kernel folds (image ^ image of key 0) over all
// keys with OR, and a pass whose byte of that word is zero -- every key has the same digit there -- is not run (two-valued
// knn / svm scores sort in one or two passes).  A pass is three launches over EV_TILE-key tiles, workgroup b owning the
// contiguous tiles [tiles b / G, tiles (b + 1) / G), G <= PHK_SORT_MAX_BLOCKS:
//   histogram : digit counts of the workgroup's keys          -> hist[digit][b]
//   scan      : exclusive scan of hist in (digit, b) order    (one workgroup; 256 G <= 131072 words)
//   scatter   : per tile, every key's rank among the tile's keys of its digit, the tile reordered by digit in LDS, then
//               written out in runs of consecutive addresses per digit.
// Ranks come from wave ballots, not from atomics (an LDS atomic returns ranks in arrival order: not stable): the 8 ballots of
// a digit's bits give each lane the mask of its peers -- the lanes holding the same digit -- and its rank among them is
// the population count below it; the first peer adds the peer count to the wave's row of counters.  A wave takes its 16 x 64
// keys in index order, so rank order is index order, and equal scores cost what distinct ones do (no contended counter).
// Keys of the last, partial tile's tail take digit 255 behind every real key and are never written out.
#include "phk_common.h"

#include <algorithm>

#define EV_THREADS 256
#define EV_WAVES (EV_THREADS / PHK_WAVE)
#define EV_ITEMS 16
#define EV_TILE PHK_SORT_TILE
static_assert(EV_TILE == EV_THREADS * EV_ITEMS, "tile = threads x items");
#define EV_SCAN_THREADS 1024
#define EV_ROC_BLOCKS 1024u   // workgroups of the curve's passes, each a contiguous range of elements

// ---- key images ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ev_image(double x, bool descending, bool *bad) {
    uint64_t b = (uint64_t)__double_as_longlong(x);
    *bad = ((b >> 52) & 0x7ffull) == 0x7ffull;           // NaN or infinite
    if (b == 0x8000000000000000ull) b = 0;              // -0.0 == +0.0
    b ^= (b >> 63) ? ~0ull : 0x8000000000000000ull;
    return descending ? ~b : b;
}

__device__ __forceinline__ uint64_t ev_wave_or(uint64_t v) {
#pragma unroll
    for (int o = 1; o < PHK_WAVE; o <<= 1) v |= __shfl_xor(v, o);
    return v;
}

// keys -> images, values = 0 .. n - 1; meta[0] |= image ^ image of key 0 (the bits in which the keys differ), meta[1] = 1
// when some key is not finite
__global__ __launch_bounds__(256) void phk_ev_prepare_kernel(const double *__restrict__ x, uint64_t n, int descending,
                                                            uint64_t *__restrict__ img, uint32_t *__restrict__ val,
                                                            unsigned long long *__restrict__ meta) {
    bool bad0;
    const uint64_t first = ev_image(x[0], descending, &bad0);
    uint64_t diff = 0;
    bool anybad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        bool bad;
        const uint64_t m = ev_image(x[i], descending, &bad);
        img[i] = m;
        val[i] = (uint32_t)i;
        diff |= m ^ first;
        anybad |= bad;
    }
    diff = ev_wave_or(diff);
    const unsigned long long nb = __ballot(anybad);
    if ((threadIdx.x & (PHK_WAVE - 1)) == 0) {
        if (diff) atomicOr(&meta[0], (unsigned long long)diff);
        if (nb) atomicOr(&meta[1], 1ull);
    }
}

// ---- ranks within a wave -------------------------------------------------------------------------------------------------
// the lanes of the wave that hold digit d (every lane of the wave must call this)
__device__ __forceinline__ uint64_t ev_peers(uint32_t d) {
    uint64_t peers = ~0ull;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// exclusive scan of one uint32 per thread over the workgroup (EV_THREADS threads); *total = the sum.  s_w: EV_WAVES words.
__device__ __forceinline__ uint32_t ev_block_scan_u32(uint32_t v, uint32_t *s_w, uint32_t *total) {
    const int lane = threadIdx.x & (PHK_WAVE - 1), w = threadIdx.x / PHK_WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < PHK_WAVE; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();   // (s_w may still be read from the previous call)
    if (lane == PHK_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < EV_WAVES; ++k) {
        const uint32_t s = s_w[k];
        before += k < w ? s : 0u;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(EV_THREADS) void phk_ev_histogram_kernel(const uint64_t *__restrict__ kin, uint64_t n, uint64_t ntiles,
                                                                     int shift, uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_h[256];
    const int t = threadIdx.x, lane = t & (PHK_WAVE - 1), w = t / PHK_WAVE;
    const uint32_t G = gridDim.x, b = blockIdx.x;
    const uint64_t t0 = ntiles * b / G, t1 = ntiles * (b + 1) / G;
    const uint64_t lt = (1ull << lane) - 1ull;
    s_h[t] = 0;
    __syncthreads();
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t base = tile * EV_TILE + (uint64_t)w * (PHK_WAVE * EV_ITEMS) + lane;
#pragma unroll
        for (int it = 0; it < EV_ITEMS; ++it) {
            const uint64_t i = base + (uint64_t)it * PHK_WAVE;
            const uint32_t d = i < n ? (uint32_t)(kin[i] >> shift) & 255u : 255u;
            const uint64_t peers = ev_peers(d);
            if ((peers & lt) == 0) atomicAdd(&s_h[d], (uint32_t)__popcll(peers));
        }
    }
    __syncthreads();
    uint32_t c = s_h[t];
    if (t == 255 && t1 > t0 && t1 * EV_TILE > n) c -= (uint32_t)(t1 * EV_TILE - n);   // the last tile's tail
    hist[(uint64_t)t * G + b] = c;
}

// exclusive scan of h[count] in place, one workgroup
__global__ __launch_bounds__(EV_SCAN_THREADS) void phk_ev_scan_kernel(uint32_t *__restrict__ h, uint32_t count) {
    __shared__ uint32_t s_w[EV_SCAN_THREADS / PHK_WAVE];
    const int t = threadIdx.x, lane = t & (PHK_WAVE - 1), w = t / PHK_WAVE;
    const uint32_t chunk = (count + EV_SCAN_THREADS - 1) / EV_SCAN_THREADS;
    const uint32_t lo = min((uint32_t)t * chunk, count), hi = min(lo + chunk, count);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += h[i];
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < PHK_WAVE; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == PHK_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int k = 0; k < w; ++k) run += s_w[k];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = h[i];
        h[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(EV_THREADS) void phk_ev_scatter_kernel(const uint64_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                                   uint64_t *__restrict__ kout, uint32_t *__restrict__ vout, uint64_t n,
                                                                   uint64_t ntiles, int shift, const uint32_t *__restrict__ offs) {
    __shared__ uint64_t s_key[EV_TILE];
    __shared__ uint32_t s_val[EV_TILE];
    __shared__ uint32_t s_wh[EV_WAVES][256];   // per wave and digit: keys so far, then the keys of the waves before
    __shared__ uint32_t s_start[256];          // first place of the digit in the reordered tile
    __shared__ uint32_t s_delta[256];          // place in the output - place in the reordered tile (mod 2^32)
    __shared__ uint32_t s_base[256];           // next place of the digit in the output
    __shared__ uint32_t s_w[EV_WAVES];
    const int t = threadIdx.x, lane = t & (PHK_WAVE - 1), w = t / PHK_WAVE;
    const uint32_t G = gridDim.x, b = blockIdx.x;
    const uint64_t t0 = ntiles * b / G, t1 = ntiles * (b + 1) / G;
    const uint64_t lt = (1ull << lane) - 1ull;
    s_base[t] = offs[(uint64_t)t * G + b];
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t tile0 = tile * EV_TILE;
        const uint32_t tile_n = (uint32_t)(n - tile0 < EV_TILE ? n - tile0 : EV_TILE);
#pragma unroll
        for (int k = 0; k < EV_WAVES; ++k) s_wh[k][t] = 0;
        __syncthreads();
        uint64_t key[EV_ITEMS];
        uint32_t val[EV_ITEMS], rank[EV_ITEMS];
        const uint32_t in0 = (uint32_t)w * (PHK_WAVE * EV_ITEMS) + lane;
#pragma unroll
        for (int it = 0; it < EV_ITEMS; ++it) {
            const uint32_t p = in0 + it * PHK_WAVE;
            key[it] = p < tile_n ? kin[tile0 + p] : ~0ull;
            val[it] = p < tile_n ? vin[tile0 + p] : 0u;
        }
#pragma unroll
        for (int it = 0; it < EV_ITEMS; ++it) {
            const uint32_t p = in0 + it * PHK_WAVE;
            const uint32_t d = p < tile_n ? (uint32_t)(key[it] >> shift) & 255u : 255u;
            const uint64_t peers = ev_peers(d);
            const uint32_t prior = s_wh[w][d], r = (uint32_t)__popcll(peers & lt);
            __builtin_amdgcn_wave_barrier();
            if (r == 0) s_wh[w][d] = prior + (uint32_t)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
            rank[it] = prior + r;
        }
        __syncthreads();
        {   // thread t = digit t: the waves' counts -> keys of the waves before; the tile's digit starts; the output's
            uint32_t before = 0;
#pragma unroll
            for (int k = 0; k < EV_WAVES; ++k) {
                const uint32_t c = s_wh[k][t];
                s_wh[k][t] = before;
                before += c;
            }
            uint32_t all;
            const uint32_t start = ev_block_scan_u32(before, s_w, &all);
            s_start[t] = start;
            const uint32_t mine = t == 255 ? before - (EV_TILE - tile_n) : before;
            const uint32_t gb = s_base[t];
            s_delta[t] = gb - start;
            s_base[t] = gb + mine;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < EV_ITEMS; ++it) {
            const uint32_t p = in0 + it * PHK_WAVE;
            const uint32_t d = p < tile_n ? (uint32_t)(key[it] >> shift) & 255u : 255u;
            const uint32_t q = s_start[d] + s_wh[w][d] + rank[it];   // < EV_TILE: a permutation of the tile's places
            s_key[q] = key[it];
            s_val[q] = val[it];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EV_ITEMS; ++j) {
            const uint32_t q = j * EV_THREADS + t;
            if (q < tile_n) {
                const uint64_t k = s_key[q];
                const uint32_t g = s_delta[(uint32_t)(k >> shift) & 255u] + q;   // < n
                kout[g] = k;
                vout[g] = s_val[q];
            }
        }
        __syncthreads();
    }
}

// ---- the sort's driver ---------------------------------------------------------------------------------------------------
struct EvSorted {
    uint64_t *keys = nullptr, *spare_keys = nullptr;   // images in order; the other half of the ping-pong pair
    uint32_t *perm = nullptr, *spare_perm = nullptr;
    char *rest = nullptr;                              // what the caller asked for beside the sort's own buffers
};

static inline uint64_t ev_align(uint64_t b) { return (b + 255) & ~255ull; }

// Sorts d_x[n] (device); `extra` more bytes of the workspace are handed back in out->rest.  PHK_ERR_NAN for a key that is
// not finite.  0 < n < 2^32.
static int ev_sort(phk_ctx *ctx, const char *fname, const double *d_x, uint64_t n, int descending, uint64_t extra, EvSorted *out) {
    const uint64_t ntiles = phk_div_up(n, EV_TILE);
    const uint32_t G = (uint32_t)(ntiles < PHK_SORT_MAX_BLOCKS ? ntiles : PHK_SORT_MAX_BLOCKS);
    const uint64_t kb = ev_align(n * 8), vb = ev_align(n * 4), hb = ev_align(256ull * G * 4);
    void *p;
    PHK_TRY(phk_ws(ctx, WS_SORT, 256 + 2 * kb + 2 * vb + hb + extra, &p));
    char *c = (char *)p;
    unsigned long long *d_meta = (unsigned long long *)c;
    uint64_t *k0 = (uint64_t *)(c + 256), *k1 = (uint64_t *)(c + 256 + kb);
    uint32_t *v0 = (uint32_t *)(c + 256 + 2 * kb), *v1 = (uint32_t *)(c + 256 + 2 * kb + vb);
    uint32_t *d_hist = (uint32_t *)(c + 256 + 2 * kb + 2 * vb);
    out->rest = c + 256 + 2 * kb + 2 * vb + hb;
    PHK_HIP(hipMemsetAsync(d_meta, 0, 16, ctx->stream));
    const unsigned pblocks = (unsigned)std::min<uint64_t>(phk_div_up(n, 256), (uint64_t)ctx->num_cus * 8);
    PHK_LAUNCH(ctx, "phk_ev_prepare_kernel",
               phk_ev_prepare_kernel<<<dim3(pblocks), dim3(256), 0, ctx->stream>>>(d_x, n, descending, k0, v0, d_meta));
    unsigned long long meta[2];
    PHK_HIP(hipMemcpyAsync(meta, d_meta, 16, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (meta[1]) {
        phk_set_error("%s: a key is NaN or infinite", fname);
        return PHK_ERR_NAN;
    }
    for (int pass = 0; pass < 8; ++pass) {
        if (((meta[0] >> (8 * pass)) & 255ull) == 0) continue;   // every key has the same digit here
        const int shift = 8 * pass;
        PHK_LAUNCH(ctx, "phk_ev_histogram_kernel",
                   phk_ev_histogram_kernel<<<dim3(G), dim3(EV_THREADS), 0, ctx->stream>>>(k0, n, ntiles, shift, d_hist));
        PHK_LAUNCH(ctx, "phk_ev_scan_kernel", phk_ev_scan_kernel<<<dim3(1), dim3(EV_SCAN_THREADS), 0, ctx->stream>>>(d_hist, 256u * G));
        PHK_LAUNCH(ctx, "phk_ev_scatter_kernel",
                   phk_ev_scatter_kernel<<<dim3(G), dim3(EV_THREADS), 0, ctx->stream>>>(k0, v0, k1, v1, n, ntiles, shift, d_hist));
        std::swap(k0, k1);
        std::swap(v0, v1);
    }
    out->keys = k0;
    out->spare_keys = k1;
    out->perm = v0;
    out->spare_perm = v1;
    return PHK_OK;
}

static int ev_check_n(const char *fname, uint64_t n) {
    if (n >= (1ull << 32)) {
        phk_set_error("%s: n = %llu; 2^32 keys or more are not supported (uint32 indices)", fname, (unsigned long long)n);
        return PHK_ERR_UNSUPPORTED;
    }
    return PHK_OK;
}

extern "C" int phk_argsort_f64_dev(phk_ctx *ctx, const double *d_keys, uint64_t n, int descending, uint32_t *d_perm) {
    PHK_ENTER(ctx, "phk_argsort_f64_dev");
    PHK_TRY(ev_check_n("phk_argsort_f64_dev", n));
    if (n == 0) return PHK_OK;
    PHK_REQUIRE(d_keys && d_perm, "phk_argsort_f64_dev: NULL pointer");
    EvSorted s;
    PHK_TRY(ev_sort(ctx, "phk_argsort_f64_dev", d_keys, n, descending != 0, 0, &s));
    PHK_HIP(hipMemcpyAsync(d_perm, s.perm, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return PHK_OK;
}

extern "C" int phk_argsort_f64(phk_ctx *ctx, const double *keys, uint64_t n, int descending, uint32_t *perm) {
    PHK_ENTER(ctx, "phk_argsort_f64");
    PHK_TRY(ev_check_n("phk_argsort_f64", n));
    if (n == 0) return PHK_OK;
    PHK_REQUIRE(keys && perm, "phk_argsort_f64: NULL pointer");
    void *d_x;
    PHK_TRY(phk_ws(ctx, WS_WIDE, n * 8, &d_x));
    PHK_TRY(phk_copy_to_device(ctx, d_x, keys, n * 8));
    EvSorted s;
    PHK_TRY(ev_sort(ctx, "phk_argsort_f64", (const double *)d_x, n, descending != 0, 0, &s));
    return phk_copy_to_host(ctx, perm, s.perm, n * 4);
}

// ---- the ROC curve -------------------------------------------------------------------------------------------------------
// Two passes of "sum per workgroup, scan the sums, scan again and write", each workgroup a contiguous range of elements.
// A pair of counts below 2^32 travels as one uint64 (high word, low word), so one scan serves both.
__device__ __forceinline__ uint64_t ev_block_scan_u64(uint64_t v, uint64_t *s_w, uint64_t *total) {
    const int lane = threadIdx.x & (PHK_WAVE - 1), w = threadIdx.x / PHK_WAVE;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < PHK_WAVE; o <<= 1) {
        const uint64_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == PHK_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < EV_WAVES; ++k) {
        const uint64_t s = s_w[k];
        before += k < w ? s : 0ull;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

// exclusive scan of part[count] (count <= EV_ROC_BLOCKS) in place; *total = the sum
__global__ __launch_bounds__(EV_SCAN_THREADS) void phk_ev_scan_parts_kernel(uint64_t *__restrict__ part, uint32_t count,
                                                                           uint64_t *__restrict__ total) {
    __shared__ uint64_t s_w[EV_SCAN_THREADS / PHK_WAVE];
    const int t = threadIdx.x, lane = t & (PHK_WAVE - 1), w = t / PHK_WAVE;
    const uint64_t v = (uint32_t)t < count ? part[t] : 0ull;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < PHK_WAVE; o <<= 1) {
        const uint64_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == PHK_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint64_t before = 0;
    for (int k = 0; k < w; ++k) before += s_w[k];
    if ((uint32_t)t < count) part[t] = before + inc - v;
    if (t == EV_SCAN_THREADS - 1) *total = before + inc;
}

// element i of the sorted order: (its label) << 32 | (1 when it ends a run of equal scores)
__device__ __forceinline__ uint64_t ev_roc_item(const uint64_t *K, const uint32_t *perm, const uint8_t *labels, uint64_t i, uint64_t n) {
    const uint64_t mark = (i + 1 == n || K[i] != K[i + 1]) ? 1ull : 0ull;
    return ((uint64_t)(labels[perm[i]] != 0) << 32) | mark;
}

__global__ __launch_bounds__(EV_THREADS) void phk_ev_roc_sum_kernel(const uint64_t *__restrict__ K, const uint32_t *__restrict__ perm,
                                                                   const uint8_t *__restrict__ labels, uint64_t n,
                                                                   uint64_t *__restrict__ part) {
    __shared__ uint64_t s_w[EV_WAVES];
    const uint64_t lo = n * blockIdx.x / gridDim.x, hi = n * (blockIdx.x + 1) / gridDim.x;
    uint64_t sum = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += EV_THREADS) sum += ev_roc_item(K, perm, labels, i, n);
    uint64_t all;
    ev_block_scan_u64(sum, s_w, &all);
    if (threadIdx.x == 0) part[blockIdx.x] = all;
}

// the distinct-score points: cf / ct / cthr[j] = false positives, true positives, score at the end of the j-th run
__global__ __launch_bounds__(EV_THREADS) void phk_ev_roc_points_kernel(const uint64_t *__restrict__ K, const uint32_t *__restrict__ perm,
                                                                      const uint8_t *__restrict__ labels, const double *__restrict__ scores,
                                                                      uint64_t n, const uint64_t *__restrict__ part,
                                                                      uint32_t *__restrict__ cf, uint32_t *__restrict__ ct,
                                                                      double *__restrict__ cthr) {
    __shared__ uint64_t s_w[EV_WAVES];
    const uint64_t lo = n * blockIdx.x / gridDim.x, hi = n * (blockIdx.x + 1) / gridDim.x;
    uint64_t carry = part[blockIdx.x];
    for (uint64_t c0 = lo; c0 < hi; c0 += EV_THREADS) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t v = i < hi ? ev_roc_item(K, perm, labels, i, n) : 0ull;
        uint64_t all;
        const uint64_t inc = carry + ev_block_scan_u64(v, s_w, &all) + v;
        if (v & 1ull) {
            const uint32_t tps = (uint32_t)(inc >> 32), j = (uint32_t)inc - 1u;   // j < number of runs <= n
            cf[j] = (uint32_t)(1 + i - tps);
            ct[j] = tps;
            cthr[j] = scores[perm[i]];
        }
        carry += all;
    }
}

// point j of m1 stays unless drop_intermediate removes it; its trapezoid (fps_j - fps_j-1)(tps_j + tps_j-1), from (0, 0)
__device__ __forceinline__ bool ev_roc_keep(const uint32_t *cf, const uint32_t *ct, uint64_t j, uint64_t m1, int drop) {
    if (!drop || m1 <= 2 || j == 0 || j + 1 == m1) return true;
    // second differences mod 2^32: both first differences lie in [0, 2^32), so zero mod 2^32 is zero
    return (uint32_t)(cf[j + 1] - 2u * cf[j] + cf[j - 1]) != 0u || (uint32_t)(ct[j + 1] - 2u * ct[j] + ct[j - 1]) != 0u;
}

__global__ __launch_bounds__(EV_THREADS) void phk_ev_roc_keep_sum_kernel(const uint32_t *__restrict__ cf, const uint32_t *__restrict__ ct,
                                                                        uint64_t m1, int drop, uint64_t *__restrict__ part) {
    __shared__ uint64_t s_w[EV_WAVES];
    const uint64_t lo = m1 * blockIdx.x / gridDim.x, hi = m1 * (blockIdx.x + 1) / gridDim.x;
    uint64_t sum = 0;
    for (uint64_t j = lo + threadIdx.x; j < hi; j += EV_THREADS) sum += ev_roc_keep(cf, ct, j, m1, drop) ? 1ull : 0ull;
    uint64_t all;
    ev_block_scan_u64(sum, s_w, &all);
    if (threadIdx.x == 0) part[blockIdx.x] = all;
}

// the curve: point 0 = (0, 0, +inf), then the points kept; *area2 += the trapezoids of this workgroup's points (taken over
// all m1 points: a dropped point lies on the straight line between its neighbours, so the integer sum is the same)
__global__ __launch_bounds__(EV_THREADS) void phk_ev_roc_curve_kernel(const uint32_t *__restrict__ cf, const uint32_t *__restrict__ ct,
                                                                     const double *__restrict__ cthr, uint64_t m1, int drop,
                                                                     const uint64_t *__restrict__ part, uint64_t *__restrict__ fps,
                                                                     uint64_t *__restrict__ tps, double *__restrict__ thr,
                                                                     unsigned long long *__restrict__ area2) {
    __shared__ uint64_t s_w[EV_WAVES];
    const uint64_t lo = m1 * blockIdx.x / gridDim.x, hi = m1 * (blockIdx.x + 1) / gridDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        fps[0] = 0;
        tps[0] = 0;
        thr[0] = __builtin_inf();
    }
    uint64_t carry = part[blockIdx.x], area = 0;
    for (uint64_t c0 = lo; c0 < hi; c0 += EV_THREADS) {
        const uint64_t j = c0 + threadIdx.x;
        const bool in = j < hi;
        const uint64_t v = in && ev_roc_keep(cf, ct, j, m1, drop) ? 1ull : 0ull;
        uint64_t all;
        const uint64_t at = carry + ev_block_scan_u64(v, s_w, &all);
        if (in) {
            const uint64_t f = cf[j], t = ct[j], fp = j ? cf[j - 1] : 0u, tp = j ? ct[j - 1] : 0u;
            area += (f - fp) * (t + tp);
            if (v) {
                fps[1 + at] = f;    // at < m1 <= n: inside the n + 1 places
                tps[1 + at] = t;
                thr[1 + at] = cthr[j];
            }
        }
        carry += all;
    }
    uint64_t all;
    ev_block_scan_u64(area, s_w, &all);
    if (threadIdx.x == 0 && all) atomicAdd(area2, (unsigned long long)all);
}

static int ev_roc(phk_ctx *ctx, const char *fname, const double *d_scores, const uint8_t *d_labels, uint64_t n, int drop,
                  uint64_t *fps, uint64_t *tps, double *thresholds, uint64_t *m, uint64_t *area2) {
    // beside the sort: ct [n] u32 | parts [EV_ROC_BLOCKS + 2] u64 | fps, tps [n + 1] u64 | thr [n + 1] f64
    const uint64_t ctb = ev_align(n * 4), pb = ev_align((EV_ROC_BLOCKS + 2) * 8ull), ob = ev_align((n + 1) * 8);
    EvSorted s;
    PHK_TRY(ev_sort(ctx, fname, d_scores, n, 1, ctb + pb + 3 * ob, &s));
    uint32_t *d_ct = (uint32_t *)s.rest, *d_cf = s.spare_perm;
    double *d_cthr = (double *)s.spare_keys;
    uint64_t *d_part = (uint64_t *)(s.rest + ctb), *d_total = d_part + EV_ROC_BLOCKS;
    unsigned long long *d_area = (unsigned long long *)(d_total + 1);
    uint64_t *d_fps = (uint64_t *)(s.rest + ctb + pb), *d_tps = (uint64_t *)(s.rest + ctb + pb + ob);
    double *d_thr = (double *)(s.rest + ctb + pb + 2 * ob);
    const uint32_t G1 = (uint32_t)std::min<uint64_t>(phk_div_up(n, EV_THREADS), EV_ROC_BLOCKS);
    PHK_HIP(hipMemsetAsync(d_area, 0, 8, ctx->stream));
    PHK_LAUNCH(ctx, "phk_ev_roc_sum_kernel",
               phk_ev_roc_sum_kernel<<<dim3(G1), dim3(EV_THREADS), 0, ctx->stream>>>(s.keys, s.perm, d_labels, n, d_part));
    PHK_LAUNCH(ctx, "phk_ev_scan_parts_kernel",
               phk_ev_scan_parts_kernel<<<dim3(1), dim3(EV_SCAN_THREADS), 0, ctx->stream>>>(d_part, G1, d_total));
    PHK_LAUNCH(ctx, "phk_ev_roc_points_kernel", phk_ev_roc_points_kernel<<<dim3(G1), dim3(EV_THREADS), 0, ctx->stream>>>(
                                                    s.keys, s.perm, d_labels, d_scores, n, d_part, d_cf, d_ct, d_cthr));
    uint64_t total = 0;
    PHK_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t m1 = total & 0xffffffffull;   // runs of equal scores, 1 <= m1 <= n
    const uint32_t G2 = (uint32_t)std::min<uint64_t>(phk_div_up(m1, EV_THREADS), EV_ROC_BLOCKS);
    PHK_LAUNCH(ctx, "phk_ev_roc_keep_sum_kernel",
               phk_ev_roc_keep_sum_kernel<<<dim3(G2), dim3(EV_THREADS), 0, ctx->stream>>>(d_cf, d_ct, m1, drop, d_part));
    PHK_LAUNCH(ctx, "phk_ev_scan_parts_kernel",
               phk_ev_scan_parts_kernel<<<dim3(1), dim3(EV_SCAN_THREADS), 0, ctx->stream>>>(d_part, G2, d_total));
    PHK_LAUNCH(ctx, "phk_ev_roc_curve_kernel", phk_ev_roc_curve_kernel<<<dim3(G2), dim3(EV_THREADS), 0, ctx->stream>>>(
                                                   d_cf, d_ct, d_cthr, m1, drop, d_part, d_fps, d_tps, d_thr, d_area));
    uint64_t tail[2];   // kept points, 2 P N AUC
    PHK_HIP(hipMemcpyAsync(tail, d_total, 16, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t mm = 1 + tail[0];
    PHK_TRY(phk_copy_to_host(ctx, fps, d_fps, mm * 8));
    PHK_TRY(phk_copy_to_host(ctx, tps, d_tps, mm * 8));
    PHK_TRY(phk_copy_to_host(ctx, thresholds, d_thr, mm * 8));
    *m = mm;
    *area2 = tail[1];
    return PHK_OK;
}

static int ev_roc_args(const char *fname, uint64_t n, uint64_t *fps, uint64_t *tps, double *thresholds, uint64_t *m, uint64_t *area2,
                       bool *done) {
    *done = false;
    PHK_TRY(ev_check_n(fname, n));
    PHK_REQUIRE(fps && tps && thresholds && m && area2, "%s: NULL output pointer", fname);
    if (n == 0) {   // the curve's first point alone
        fps[0] = tps[0] = 0;
        thresholds[0] = __builtin_inf();
        *m = 1;
        *area2 = 0;
        *done = true;
    }
    return PHK_OK;
}

extern "C" int phk_roc_curve_dev(phk_ctx *ctx, const double *d_scores, const uint8_t *d_labels, uint64_t n, int drop_intermediate,
                                 uint64_t *fps, uint64_t *tps, double *thresholds, uint64_t *m, uint64_t *area2) {
    PHK_ENTER(ctx, "phk_roc_curve_dev");
    bool done;
    PHK_TRY(ev_roc_args("phk_roc_curve_dev", n, fps, tps, thresholds, m, area2, &done));
    if (done) return PHK_OK;
    PHK_REQUIRE(d_scores && d_labels, "phk_roc_curve_dev: NULL pointer");
    return ev_roc(ctx, "phk_roc_curve_dev", d_scores, d_labels, n, drop_intermediate != 0, fps, tps, thresholds, m, area2);
}

extern "C" int phk_roc_curve(phk_ctx *ctx, const double *scores, const uint8_t *labels, uint64_t n, int drop_intermediate,
                             uint64_t *fps, uint64_t *tps, double *thresholds, uint64_t *m, uint64_t *area2) {
    PHK_ENTER(ctx, "phk_roc_curve");
    bool done;
    PHK_TRY(ev_roc_args("phk_roc_curve", n, fps, tps, thresholds, m, area2, &done));
    if (done) return PHK_OK;
    PHK_REQUIRE(scores && labels, "phk_roc_curve: NULL pointer");
    void *p;
    const uint64_t sb = ev_align(n * 8);
    PHK_TRY(phk_ws(ctx, WS_WIDE, sb + n, &p));
    PHK_TRY(phk_copy_to_device(ctx, p, scores, n * 8));
    PHK_TRY(phk_copy_to_device(ctx, (char *)p + sb, labels, n));
    return ev_roc(ctx, "phk_roc_curve", (const double *)p, (const uint8_t *)p + sb, n, drop_intermediate != 0, fps, tps, thresholds, m,
                  area2);
}

// ---- truth table ---------------------------------------------------------------------------------------------------------
// counts[0..3] += tp, fp, fn, tn: label != 0 and score >= threshold, label == 0 and >=, label != 0 and <, label == 0 and <
// (a NaN score is in none of them, as with NumPy's comparisons)
__global__ __launch_bounds__(256) void phk_ev_truth_kernel(const double *__restrict__ scores, const uint8_t *__restrict__ labels,
                                                          uint64_t n, double threshold, unsigned long long *__restrict__ counts) {
    uint32_t c[4] = {0, 0, 0, 0};   // a thread sees n / (grid x 256) + 1 elements at most
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double s = scores[i];
        const bool pos = labels[i] != 0, ge = s >= threshold, lt = s < threshold;
        c[0] += pos && ge;
        c[1] += !pos && ge;
        c[2] += pos && lt;
        c[3] += !pos && lt;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = c[k];
#pragma unroll
        for (int o = 1; o < PHK_WAVE; o <<= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & (PHK_WAVE - 1)) == 0 && v) atomicAdd(&counts[k], (unsigned long long)v);
    }
}

extern "C" int phk_truth_counts(phk_ctx *ctx, const double *scores, const uint8_t *labels, uint64_t n, double threshold,
                                uint64_t *counts) {
    PHK_ENTER(ctx, "phk_truth_counts");
    PHK_REQUIRE(counts, "phk_truth_counts: NULL pointer");
    PHK_REQUIRE(threshold == threshold, "phk_truth_counts: the threshold is NaN");
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n == 0) return PHK_OK;
    PHK_REQUIRE(scores && labels, "phk_truth_counts: NULL pointer");
    void *p, *d_counts;
    const uint64_t sb = ev_align(n * 8);
    PHK_TRY(phk_ws(ctx, WS_WIDE, sb + n, &p));
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &d_counts));
    PHK_TRY(phk_copy_to_device(ctx, p, scores, n * 8));
    PHK_TRY(phk_copy_to_device(ctx, (char *)p + sb, labels, n));
    PHK_HIP(hipMemsetAsync(d_counts, 0, 32, ctx->stream));
    const unsigned blocks = (unsigned)std::min<uint64_t>(phk_div_up(n, 256), (uint64_t)ctx->num_cus * 8);
    PHK_LAUNCH(ctx, "phk_ev_truth_kernel", phk_ev_truth_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(
                                               (const double *)p, (const uint8_t *)p + sb, n, threshold, (unsigned long long *)d_counts));
    return phk_copy_to_host(ctx, counts, d_counts, 32);
}

// ---- paired comparison of ROC areas ---------------------------------------------------------------------
// scores[C][n]: one row per CELL, columns in vstack(positive, negative) order -- the first P columns are the positives,
// N = n - P.  Scores are finite; -0.0 == +0.0 as in the sort.
//   twice-placements (uint32)  t_pos[c][i] = 2 #{j : y_j < x_i} + #{j : y_j == x_i},  t_neg[c][j] = 2 #{i : x_i > y_j} +
//                              #{i : x_i == y_j}; both sum to area2[c] = 2 P N AUC, the integer phk_roc_curve returns
//   Gram matrices (uint64)     G10[a][b] = sum_i t_pos[a][i] t_pos[b][i],  G01[a][b] = sum_j t_neg[a][j] t_neg[b][j]
//                              (DeLong's covariance is a rational function of these and area2: phamers_amd/compare.py)
//   stratified bootstrap       resample b draws P positives and N negatives with replacement: key(b, s) =
//                              splitmix64(splitmix64(seed) ^ (2 b + s)), s = 0 positives, 1 negatives; draw t of class s is
//                              the class's row mulhi64(splitmix64(key + t), n_s); w[row] = times drawn;
//                              area2_boot[b][c] = sum_ij w_i w_j (2 [x_i > y_j] + [x_i == y_j]) <= 2 P N
// With the run counts of the descending order (fps, tps through the end of run r, before any point is dropped; 0 before the
// first run) a positive of run r has t = 2 N - fps[r] - fps[r - 1], a negative t = tps[r] + tps[r - 1]: the placements are
// a gather on top of the sort and the curve's run points.  The cells are sorted one after the other; each leaves its
// order, its run-end marks and its placements in the handle.  Every sum is an integer sum: order-free, bit-reproducible.
#define CMP_TILE 32            // cells per side of a Gram tile
#define CMP_GRAM_ROWS 256      // rows of one class per workgroup of the Gram kernel
#define CMP_GRAM_STEP 64       // ... staged through LDS this many at a time
#define CMP_BOOT_CELLS 8       // cells a bootstrap workgroup walks with one set of weights
#define CMP_BOOT_PER_LAUNCH 1024u
static_assert(PHK_COMPARE_BOOT_MAX_ROWS <= 65535, "the bootstrap counts a row's draws in 16 bits: a class has fewer rows than 2^16");

struct phk_compare {
    uint64_t C = 0, n = 0, P = 0;
    PhkDevMem perm;   // [C][n] uint32: the descending order of every cell
    PhkDevMem mark;   // [C][n] uint8: 1 where a run of equal scores ends
    PhkDevMem T;      // [C][n] uint32: twice-placements at the ORIGINAL row index
    PhkDevMem sums;   // uint64: area2 [C] | G10 [C][C] | G01 [C][C]
    PhkDevMem boot;   // uint64 [resamples per launch][C]
};

// the gather: element i of the sorted order looks up the counts of its run (cf, ct of phk_ev_roc_points_kernel, same grid
// and `part`) and writes its twice-placement at its row; *area2 += the positives' placements
__global__ __launch_bounds__(EV_THREADS) void phk_cmp_place_kernel(const uint64_t *__restrict__ K, const uint32_t *__restrict__ perm,
                                                                  const uint8_t *__restrict__ labels, uint64_t n, uint32_t n_neg,
                                                                  const uint64_t *__restrict__ part, const uint32_t *__restrict__ cf,
                                                                  const uint32_t *__restrict__ ct, uint32_t *__restrict__ out_perm,
                                                                  uint8_t *__restrict__ out_mark, uint32_t *__restrict__ out_T,
                                                                  unsigned long long *__restrict__ area2) {
    __shared__ uint64_t s_w[EV_WAVES];
    const uint64_t lo = n * blockIdx.x / gridDim.x, hi = n * (blockIdx.x + 1) / gridDim.x;
    uint64_t carry = part[blockIdx.x], sum = 0;
    for (uint64_t c0 = lo; c0 < hi; c0 += EV_THREADS) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t v = i < hi ? ev_roc_item(K, perm, labels, i, n) : 0ull;
        uint64_t all;
        const uint64_t inc = carry + ev_block_scan_u64(v, s_w, &all) + v;
        if (i < hi) {
            const uint32_t j = (uint32_t)inc - (uint32_t)(v & 1ull);   // runs ended before i = the run of i, < number of runs
            const uint32_t f = cf[j], t = ct[j], fp = j ? cf[j - 1] : 0u, tp = j ? ct[j - 1] : 0u;
            const uint32_t row = perm[i];                              // < n
            const bool pos = (v >> 32) != 0;
            const uint32_t T = pos ? 2u * n_neg - f - fp : t + tp;
            out_T[row] = T;
            out_perm[i] = row;
            out_mark[i] = (uint8_t)(v & 1ull);
            if (pos) sum += T;
        }
        carry += all;
    }
    uint64_t all;
    ev_block_scan_u64(sum, s_w, &all);
    if (threadIdx.x == 0 && all) atomicAdd(area2, (unsigned long long)all);
}

// G[cls][a][b] += sum over this workgroup's rows of class cls of T[a][row] T[b][row]: blockIdx.x = a pair of cell tiles
// (ta <= tb; the mirror image is written too), .y = the chunk of CMP_GRAM_ROWS rows, .z = the class.  Thread (ty, tx) of
// 16 x 16 holds the four sums of cells {ty, ty + 16} x {tx, tx + 16} of the tile pair.
__global__ __launch_bounds__(256) void phk_cmp_gram_kernel(const uint32_t *__restrict__ T, uint32_t C, uint64_t n, uint64_t P,
                                                          uint32_t ntiles, unsigned long long *__restrict__ G) {
    __shared__ uint32_t sA[CMP_TILE][CMP_GRAM_STEP + 1], sB[CMP_TILE][CMP_GRAM_STEP + 1];
    uint32_t p = blockIdx.x, ta = 0;
    while (p >= ntiles - ta) {
        p -= ntiles - ta;
        ++ta;
    }
    const uint32_t tb = ta + p, cls = blockIdx.z;
    const uint64_t r1 = cls ? n : P, row0 = (cls ? P : 0ull) + (uint64_t)blockIdx.y * CMP_GRAM_ROWS;
    if (row0 >= r1) return;
    const uint64_t rowE = row0 + CMP_GRAM_ROWS < r1 ? row0 + CMP_GRAM_ROWS : r1;
    const uint32_t ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    uint64_t a00 = 0, a01 = 0, a10 = 0, a11 = 0;
    for (uint64_t s0 = row0; s0 < rowE; s0 += CMP_GRAM_STEP) {
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < CMP_TILE * CMP_GRAM_STEP; e += 256) {
            const uint32_t cell = e / CMP_GRAM_STEP, k = e % CMP_GRAM_STEP;
            const uint64_t row = s0 + k;
            const uint32_t a = ta * CMP_TILE + cell, b = tb * CMP_TILE + cell;
            sA[cell][k] = (a < C && row < rowE) ? T[(uint64_t)a * n + row] : 0u;
            sB[cell][k] = (b < C && row < rowE) ? T[(uint64_t)b * n + row] : 0u;
        }
        __syncthreads();
#pragma unroll 8
        for (uint32_t k = 0; k < CMP_GRAM_STEP; ++k) {
            const uint64_t x0 = sA[ty][k], x1 = sA[ty + 16][k], y0 = sB[tx][k], y1 = sB[tx + 16][k];
            a00 += x0 * y0;
            a01 += x0 * y1;
            a10 += x1 * y0;
            a11 += x1 * y1;
        }
    }
    unsigned long long *g = G + (uint64_t)cls * C * C;
    const uint32_t ca[2] = {ta * CMP_TILE + ty, ta * CMP_TILE + ty + 16}, cb[2] = {tb * CMP_TILE + tx, tb * CMP_TILE + tx + 16};
    const uint64_t acc[2][2] = {{a00, a01}, {a10, a11}};
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (ca[u] >= C || cb[v] >= C || acc[u][v] == 0) continue;
            atomicAdd(&g[(uint64_t)ca[u] * C + cb[v]], (unsigned long long)acc[u][v]);
            if (ta != tb) atomicAdd(&g[(uint64_t)cb[v] * C + ca[u]], (unsigned long long)acc[u][v]);
        }
}

// the generator of the bootstrap draws: splitmix64 as in synth.hip (oracle.py restates it)
__host__ __device__ __forceinline__ uint64_t cmp_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The walk's scan element: bits 0-19 the weighted negatives so far (a plain sum), bits 20-39 / 40-59 the weighted
// positives / negatives of the current run (sums that start over where bit 63, "a run starts here", is set).  Every field
// stays below 2^16 (a class's weights sum to its size), so no field carries into the next.
#define CMP_F_CN 0xFFFFFull
#define CMP_F_SEG (0xFFFFFFFFFFull << 20)
#define CMP_F_START (1ull << 63)
__device__ __forceinline__ uint64_t cmp_combine(uint64_t l, uint64_t r) {   // l before r; associative
    const uint64_t cn = ((l & CMP_F_CN) + (r & CMP_F_CN)) & CMP_F_CN;
    const uint64_t seg = (r & CMP_F_START) ? (r & CMP_F_SEG) : ((l & CMP_F_SEG) + (r & CMP_F_SEG)) & CMP_F_SEG;
    return cn | seg | ((l | r) & CMP_F_START);
}

// inclusive scan under cmp_combine over the workgroup (EV_THREADS threads); *total = all of it
__device__ __forceinline__ uint64_t cmp_block_scan(uint64_t v, uint64_t *s_w, uint64_t *total) {
    const int lane = threadIdx.x & (PHK_WAVE - 1), w = threadIdx.x / PHK_WAVE;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < PHK_WAVE; o <<= 1) {
        const uint64_t u = __shfl_up(inc, o);
        if (lane >= o) inc = cmp_combine(u, inc);
    }
    __syncthreads();
    if (lane == PHK_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < EV_WAVES; ++k) {
        const uint64_t s = s_w[k];
        if (k < w) before = cmp_combine(before, s);
        all = cmp_combine(all, s);
    }
    *total = all;
    return cmp_combine(before, inc);
}

// Workgroup (x, y): resample first + x, cells y, y + gridDim.y, ...  The weights of the resample -- n 16-bit counters, two
// to a word of dynamic LDS -- are drawn once; each cell's sorted order is then walked in chunks of EV_THREADS elements, one
// scan per chunk and a carry between chunks, and a run of weighted totals Wp, Wn ending with cn weighted negatives so far
// adds Wp ((N - cn) + (N - (cn - Wn))).  out[x][c] = the cell's sum.
__global__ __launch_bounds__(EV_THREADS) void phk_cmp_boot_kernel(const uint32_t *__restrict__ perm, const uint8_t *__restrict__ mark,
                                                                 uint32_t C, uint32_t n, uint32_t P, uint64_t seed_mix, uint64_t first,
                                                                 unsigned long long *__restrict__ out) {
    extern __shared__ uint32_t cmp_w[];   // (n + 1) / 2 words
    __shared__ uint64_t s_w[EV_WAVES];
    const uint32_t t = threadIdx.x, words = (n + 1) / 2, N = n - P;
    const uint64_t b = first + blockIdx.x;
    for (uint32_t i = t; i < words; i += EV_THREADS) cmp_w[i] = 0;
    __syncthreads();
    for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t ns = s ? N : P, base = s ? P : 0u;
        const uint64_t key = cmp_splitmix64(seed_mix ^ (2 * b + s));
        for (uint32_t d = t; d < ns; d += EV_THREADS) {
            const uint32_t row = base + (uint32_t)__umul64hi(cmp_splitmix64(key + d), (uint64_t)ns);   // < base + ns <= n
            atomicAdd(&cmp_w[row >> 1], 1u << (16 * (row & 1u)));
        }
    }
    __syncthreads();
    for (uint32_t c = blockIdx.y; c < C; c += gridDim.y) {
        const uint32_t *cperm = perm + (uint64_t)c * n;
        const uint8_t *cmark = mark + (uint64_t)c * n;
        uint64_t carry = 0, sum = 0;
        for (uint32_t c0 = 0; c0 < n; c0 += EV_THREADS) {
            const uint32_t i = c0 + t;
            uint64_t v = 0;
            bool end = false;
            if (i < n) {
                const uint32_t row = cperm[i];   // < n
                const uint64_t w = (cmp_w[row >> 1] >> (16 * (row & 1u))) & 0xFFFFu;
                v = row < P ? w << 20 : (w | (w << 40));
                if (i == 0 || cmark[i - 1]) v |= CMP_F_START;
                end = cmark[i] != 0;
            }
            uint64_t all;
            const uint64_t r = cmp_combine(carry, cmp_block_scan(v, s_w, &all));
            if (end) {
                const uint64_t cn = r & CMP_F_CN, wp = (r >> 20) & CMP_F_CN, wn = (r >> 40) & CMP_F_CN;
                sum += wp * (2ull * N - 2ull * cn + wn);
            }
            carry = cmp_combine(carry, all);
        }
        uint64_t all;
        ev_block_scan_u64(sum, s_w, &all);
        if (t == 0) out[(uint64_t)blockIdx.x * C + c] = all;
    }
}

extern "C" int phk_compare_create(phk_ctx *ctx, const double *scores, uint64_t C, uint64_t n, uint64_t n_pos, phk_compare **out) {
    static const char *fname = "phk_compare_create";
    PHK_ENTER(ctx, "phk_compare_create");
    PHK_REQUIRE(out && scores, "%s: NULL pointer", fname);
    PHK_REQUIRE(C >= 1 && C <= PHK_COMPARE_MAX_CELLS, "%s: need 1 <= cells <= %d (got %llu)", fname, PHK_COMPARE_MAX_CELLS,
                (unsigned long long)C);
    PHK_REQUIRE(n_pos >= 1 && n_pos < n, "%s: both classes need a row (%llu rows, %llu positive)", fname, (unsigned long long)n,
                (unsigned long long)n_pos);
    const uint64_t P = n_pos, N = n - n_pos;
    const unsigned __int128 lim = (unsigned __int128)1 << 64;
    if (n >= (1ull << 31) || (unsigned __int128)4 * N * N * P >= lim || (unsigned __int128)4 * P * P * N >= lim) {
        phk_set_error("%s: %llu positive and %llu negative rows; the Gram sums are exact below 4 N^2 P = 2^64 and 4 P^2 N = 2^64 only",
                      fname, (unsigned long long)P, (unsigned long long)N);
        return PHK_ERR_UNSUPPORTED;
    }
    if (!phk_rows_finite(scores, C * n)) {
        phk_set_error("%s: a score is NaN or infinite", fname);
        return PHK_ERR_NAN;
    }
    phk_compare *h = new phk_compare;
    h->C = C;
    h->n = n;
    h->P = P;
    PhkDevMem d_scores, d_labels;
    auto run = [&]() -> int {
        PHK_TRY(d_scores.alloc(fname, "scores", C * n * 8));
        PHK_TRY(d_labels.alloc(fname, "labels", n));
        PHK_TRY(h->perm.alloc(fname, "sorted orders", C * n * 4));
        PHK_TRY(h->mark.alloc(fname, "run marks", C * n));
        PHK_TRY(h->T.alloc(fname, "placements", C * n * 4));
        PHK_TRY(h->sums.alloc(fname, "Gram matrices", (C + 2 * C * C) * 8));
        PHK_TRY(phk_copy_to_device(ctx, d_scores.ptr, scores, C * n * 8));
        PHK_HIP(hipMemsetAsync(d_labels.ptr, 1, P, ctx->stream));
        PHK_HIP(hipMemsetAsync(d_labels.as<uint8_t>() + P, 0, N, ctx->stream));
        PHK_HIP(hipMemsetAsync(h->sums.ptr, 0, (C + 2 * C * C) * 8, ctx->stream));
        unsigned long long *d_area = h->sums.as<unsigned long long>(), *d_G = d_area + C;
        const uint64_t ctb = ev_align(n * 4), pb = ev_align((EV_ROC_BLOCKS + 2) * 8ull);
        const uint32_t G1 = (uint32_t)std::min<uint64_t>(phk_div_up(n, EV_THREADS), EV_ROC_BLOCKS);
        for (uint64_t c = 0; c < C; ++c) {
            const double *d_x = d_scores.as<double>() + c * n;
            EvSorted s;
            PHK_TRY(ev_sort(ctx, fname, d_x, n, 1, ctb + pb, &s));
            uint32_t *d_ct = (uint32_t *)s.rest, *d_cf = s.spare_perm;
            uint64_t *d_part = (uint64_t *)(s.rest + ctb), *d_total = d_part + EV_ROC_BLOCKS;
            PHK_LAUNCH(ctx, "phk_ev_roc_sum_kernel", phk_ev_roc_sum_kernel<<<dim3(G1), dim3(EV_THREADS), 0, ctx->stream>>>(
                                                         s.keys, s.perm, d_labels.as<uint8_t>(), n, d_part));
            PHK_LAUNCH(ctx, "phk_ev_scan_parts_kernel",
                       phk_ev_scan_parts_kernel<<<dim3(1), dim3(EV_SCAN_THREADS), 0, ctx->stream>>>(d_part, G1, d_total));
            PHK_LAUNCH(ctx, "phk_ev_roc_points_kernel", phk_ev_roc_points_kernel<<<dim3(G1), dim3(EV_THREADS), 0, ctx->stream>>>(
                                                            s.keys, s.perm, d_labels.as<uint8_t>(), d_x, n, d_part, d_cf, d_ct,
                                                            (double *)s.spare_keys));
            PHK_LAUNCH(ctx, "phk_cmp_place_kernel", phk_cmp_place_kernel<<<dim3(G1), dim3(EV_THREADS), 0, ctx->stream>>>(
                                                        s.keys, s.perm, d_labels.as<uint8_t>(), n, (uint32_t)N, d_part, d_cf, d_ct,
                                                        h->perm.as<uint32_t>() + c * n, h->mark.as<uint8_t>() + c * n,
                                                        h->T.as<uint32_t>() + c * n, d_area + c));
        }
        const uint32_t ntiles = (uint32_t)phk_div_up(C, CMP_TILE);
        const uint32_t chunks = (uint32_t)phk_div_up(std::max(P, N), CMP_GRAM_ROWS);   // < 2^16: P, N < 2^22 by the limit above
        PHK_LAUNCH(ctx, "phk_cmp_gram_kernel",
                   phk_cmp_gram_kernel<<<dim3(ntiles * (ntiles + 1) / 2, chunks, 2), dim3(256), 0, ctx->stream>>>(
                       h->T.as<uint32_t>(), (uint32_t)C, n, P, ntiles, d_G));
        PHK_HIP(hipStreamSynchronize(ctx->stream));   // (the call's own buffers go with it)
        return PHK_OK;
    };
    const int rc = run();
    if (rc != PHK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        delete h;
        return rc;
    }
    *out = h;
    return PHK_OK;
}

extern "C" int phk_compare_destroy(phk_ctx *ctx, phk_compare *cmp) {
    PHK_ENTER(ctx, "phk_compare_destroy");
    if (!cmp) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    delete cmp;
    return PHK_OK;
}

extern "C" int phk_compare_placements(phk_ctx *ctx, phk_compare *cmp, uint32_t *t_pos, uint32_t *t_neg) {
    PHK_ENTER(ctx, "phk_compare_placements");
    PHK_REQUIRE(cmp && t_pos && t_neg, "phk_compare_placements: NULL pointer");
    const uint64_t C = cmp->C, n = cmp->n, P = cmp->P, N = n - P;
    std::vector<uint32_t> T(C * n);
    PHK_TRY(phk_copy_to_host(ctx, T.data(), cmp->T.ptr, C * n * 4));
    for (uint64_t c = 0; c < C; ++c) {
        std::copy(T.begin() + c * n, T.begin() + c * n + P, t_pos + c * P);
        std::copy(T.begin() + c * n + P, T.begin() + (c + 1) * n, t_neg + c * N);
    }
    return PHK_OK;
}

extern "C" int phk_compare_grams(phk_ctx *ctx, phk_compare *cmp, uint64_t *area2, uint64_t *g10, uint64_t *g01) {
    PHK_ENTER(ctx, "phk_compare_grams");
    PHK_REQUIRE(cmp && area2 && g10 && g01, "phk_compare_grams: NULL pointer");
    const uint64_t C = cmp->C;
    const uint64_t *d = cmp->sums.as<uint64_t>();
    PHK_TRY(phk_copy_to_host(ctx, area2, d, C * 8));
    PHK_TRY(phk_copy_to_host(ctx, g10, d + C, C * C * 8));
    return phk_copy_to_host(ctx, g01, d + C + C * C, C * C * 8);
}

extern "C" int phk_compare_bootstrap(phk_ctx *ctx, phk_compare *cmp, uint64_t seed, uint64_t first_resample, uint64_t count,
                                     uint64_t per_launch, uint64_t *area2_boot) {
    PHK_ENTER(ctx, "phk_compare_bootstrap");
    PHK_REQUIRE(cmp, "phk_compare_bootstrap: NULL handle");
    const uint64_t C = cmp->C, n = cmp->n;
    if (n > PHK_COMPARE_BOOT_MAX_ROWS) {
        phk_set_error("phk_compare_bootstrap: %llu rows; the bootstrap keeps a resample's weights in LDS, at most %d rows",
                      (unsigned long long)n, PHK_COMPARE_BOOT_MAX_ROWS);
        return PHK_ERR_UNSUPPORTED;
    }
    if (count == 0) return PHK_OK;
    PHK_REQUIRE(area2_boot, "phk_compare_bootstrap: NULL pointer");
    const uint64_t per = std::min<uint64_t>(count, per_launch ? std::min<uint64_t>(per_launch, 65536) : CMP_BOOT_PER_LAUNCH);
    PHK_TRY(cmp->boot.grow(ctx, "phk_compare_bootstrap", per * C * 8, per));
    const uint32_t lds = (uint32_t)((n + 1) / 2 * 4);
    PHK_HIP(hipFuncSetAttribute((const void *)phk_cmp_boot_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (PHK_COMPARE_BOOT_MAX_ROWS + 1) / 2 * 4));
    const uint64_t seed_mix = cmp_splitmix64(seed);
    const uint32_t groups = (uint32_t)phk_div_up(C, CMP_BOOT_CELLS);
    for (uint64_t done = 0; done < count; done += per) {
        const uint64_t now = std::min(per, count - done);
        PHK_LAUNCH(ctx, "phk_cmp_boot_kernel", phk_cmp_boot_kernel<<<dim3((unsigned)now, groups), dim3(EV_THREADS), lds, ctx->stream>>>(
                                                   cmp->perm.as<uint32_t>(), cmp->mark.as<uint8_t>(), (uint32_t)C, (uint32_t)n,
                                                   (uint32_t)cmp->P, seed_mix, first_resample + done,
                                                   cmp->boot.as<unsigned long long>()));
        PHK_TRY(phk_copy_to_host(ctx, area2_boot + done * C, cmp->boot.ptr, now * C * 8));
    }
    return PHK_OK;
}
