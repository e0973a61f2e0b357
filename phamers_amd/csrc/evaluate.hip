// evaluate.hip -- evaluation of score vectors on the device (gfx950): what PhaMers' scripts/learning.py:185-243 computes
// with scikit-learn's roc_curve / auc and NumPy comparisons, and the sort under it.
//   phk_argsort_f64 / _dev : the stable permutation that orders n float64 keys (least-significant-digit radix sort)
//   phk_roc_curve / _dev   : scikit-learn's roc_curve(..., drop_intermediate) in integers: fps, tps, thresholds, 2 P N AUC
//   phk_truth_counts       : tp, fp, fn, tn at a threshold (>= / <), one reduction
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
