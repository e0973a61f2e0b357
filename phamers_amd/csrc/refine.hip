// refine.hip -- the boundaries of composition segments refined to the base (phamers_amd/refine.py).
//
// A boundary sits between a run of windows in state a and a run in state b.  Within an interval [lo, hi] around the window
// boundary x the best change point is the prefix maximum of the per-base log ratio of the two states' profiles:
//     d(i) = q[a][code(i)] - q[b][code(i)]     for a valid k-mer starting at base i, 0 otherwise
//     P(p) = sum_{lo <= i < p} d(i)            p = lo .. hi
//     p*   = arg max P, ties to the smallest |p - x|, then to the smallest p
// q are int64 (segment.quantise: units of 2^-16 nat), so every sum is exact and the result does not depend on the order of
// the reduction.  One wave per boundary: a pass covers 64 packed words = 1024 k-mer starts, a lane walks the 16 starts of its
// word in order, the lanes' totals go through a wave scan, the wave's best through a butterfly over the three-key order.
#include <string.h>

#include <vector>

#include "phk_common.h"

#define PHK_REFINE_WAVES 4              // boundaries (waves) per workgroup
#define PHK_REFINE_BLOCKS_MAX 2048      // workgroups per launch, grid-stride beyond
#define PHK_REFINE_LDS_D 1024           // the difference row lives in LDS up to this many columns (k <= 5)
#define PHK_REFINE_MAX_SPAN (1ull << 30)
#define PHK_REFINE_MAX_Q (1ll << 31)

struct PhkRefineJob {
    uint64_t lo, x, hi;   // in bases of the packed stream
    uint64_t vend;        // k-mer starts from here on run past the sequence's end
    uint64_t base;        // the sequence's first base in the stream
    uint32_t left, right; // table rows
};

// LDS operations of one wave are executed in order; this only keeps the compiler from moving them across the point where
// the lanes of a wave hand data to each other through LDS (as windows.hip's)
__device__ __forceinline__ void refine_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bit j = base g0 + j lies in [a, b)
__device__ __forceinline__ uint32_t refine_rangebits(uint64_t g0, uint64_t a, uint64_t b) {
    const uint32_t lj = a > g0 ? (a - g0 < 16 ? (uint32_t)(a - g0) : 16u) : 0u;
    const uint32_t hj = b > g0 ? (b - g0 < 16 ? (uint32_t)(b - g0) : 16u) : 0u;
    return hj > lj ? ((1u << hj) - 1u) & ~((1u << lj) - 1u) : 0u;
}

// bit j = the k-mer starting at base 16 w + j is free of invalid bases (windows.hip's win_okbits layout: mask bit 31 - i of
// word m = base 32 m + i valid; the bases past the stream's end are invalid)
__device__ __forceinline__ uint32_t refine_validbits(const uint32_t *__restrict__ mask, uint64_t w, int K) {
    const uint64_t mi = w >> 1;
    const uint64_t V = ((uint64_t)mask[mi] << 32) | mask[mi + 1];
    const uint32_t vb = (uint32_t)(V >> (32 - 16 * (int)(w & 1)));
    uint32_t wv = vb;
    for (int j = 1; j < K; ++j) wv &= vb << j;
    return __brev(wv);
}

// candidate (v, p) comes before (bv, bp): the larger sum, then the smaller distance from x, then the smaller position
__device__ __forceinline__ bool refine_better(long long v, uint64_t p, long long bv, uint64_t bp, uint64_t x) {
    if (v != bv) return v > bv;
    const uint64_t d = p > x ? p - x : x - p, bd = bp > x ? bp - x : x - bp;
    if (d != bd) return d < bd;
    return p < bp;
}

// TABLE: the difference row of the boundary is built in the wave's LDS (D <= PHK_REFINE_LDS_D); otherwise both rows are read
// from global memory per k-mer.
template <bool TABLE>
__global__ __launch_bounds__(64 * PHK_REFINE_WAVES) void phk_refine_boundaries_kernel(
    const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask, const long long *__restrict__ q, uint32_t D, int K,
    const PhkRefineJob *__restrict__ jobs, uint64_t B, long long *__restrict__ position, long long *__restrict__ evidence,
    uint32_t *__restrict__ support) {
    __shared__ __attribute__((aligned(16))) long long rows_s[TABLE ? PHK_REFINE_WAVES * PHK_REFINE_LDS_D : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long *drow = rows_s + (TABLE ? wave * PHK_REFINE_LDS_D : 0);
    const uint32_t dmask = D - 1u;
    const long long NONE = (long long)0x8000000000000000ull;
    for (uint64_t bi = (uint64_t)blockIdx.x * PHK_REFINE_WAVES + wave; bi < B; bi += (uint64_t)gridDim.x * PHK_REFINE_WAVES) {
        const PhkRefineJob job = jobs[bi];
        const uint64_t lo = job.lo, x = job.x, hi = job.hi;
        const uint64_t ve = job.vend < hi ? job.vend : hi;   // valid k-mer starts lie in [lo, ve)
        const long long *ql = q + (uint64_t)job.left * D, *qr = q + (uint64_t)job.right * D;
        long long best_v = 0, carry = 0, px = 0;             // the candidate p = lo: P = 0
        uint64_t best_p = lo;
        uint32_t sup = 0;
        if (hi > lo) {                                       // (wave-uniform; an empty interval stays at lo = x with zeros)
            if (TABLE) {
                refine_wave_sync();                          // the previous boundary's gathers are done
                for (uint32_t c = lane; c < D; c += 64) drow[c] = ql[c] - qr[c];
                refine_wave_sync();
            }
            const uint64_t wlo = lo >> 4, whi = (hi - 1) >> 4;
            for (uint64_t wb = wlo; wb <= whi; wb += 64) {
                const uint64_t w = wb + lane;
                const bool act = w <= whi;
                const uint64_t wc = act ? w : whi;
                const uint64_t g0 = wc << 4;
                const uint32_t a = packed[wc], b = packed[wc + 1];
                const uint32_t inr = act ? refine_rangebits(g0, lo, hi) : 0u;
                const uint32_t ok = act ? refine_rangebits(g0, lo, ve) & refine_validbits(mask, wc, K) : 0u;
                const uint64_t X = ((uint64_t)a << 32) | b;
                long long s = 0, lv = NONE, lpx = 0;
                uint64_t lp = 0;
                bool hasx = false;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t idx = (uint32_t)(X >> (64 - 2 * K - 2 * j)) & dmask;
                    long long d = 0;
                    if (TABLE) {
                        d = (ok >> j) & 1u ? drow[idx] : 0ll;
                    } else if ((ok >> j) & 1u) {
                        d = ql[idx] - qr[idx];
                    }
                    s += d;
                    if ((inr >> j) & 1u) {                   // the candidate p = g0 + j + 1 with P = (what comes before) + s
                        const uint64_t p = g0 + j + 1;
                        if (lv == NONE || refine_better(s, p, lv, lp, x)) { lv = s; lp = p; }
                        if (p == x) { lpx = s; hasx = true; }
                    }
                }
                sup += __popc(ok);
                // exclusive scan of the lanes' totals
                long long inc = s;
#pragma unroll
                for (int sh = 1; sh < 64; sh <<= 1) {
                    const long long t = __shfl_up(inc, sh);
                    if (lane >= sh) inc += t;
                }
                const long long before = carry + (inc - s);
                if (hasx) px += before + lpx;
                long long v = lv == NONE ? NONE : before + lv;
                uint64_t p = lp;
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) {
                    const long long ov = __shfl_xor(v, sh);
                    const uint64_t op = __shfl_xor(p, sh);
                    const bool take = ov != NONE && (v == NONE || refine_better(ov, op, v, p, x));
                    v = take ? ov : v;
                    p = take ? op : p;
                }
                if (refine_better(v, p, best_v, best_p, x)) { best_v = v; best_p = p; }   // (every lane holds the pass's best)
                carry += __shfl(inc, 63);
            }
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) px += __shfl_xor(px, sh);
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) sup += __shfl_xor(sup, sh);
        if (lane == 0) {
            position[bi] = (long long)(best_p - job.base);
            evidence[3 * bi + 0] = best_v - px;
            evidence[3 * bi + 1] = best_v;
            evidence[3 * bi + 2] = best_v - carry;
            support[bi] = sup;
        }
    }
}

// ------------------------------------------------------------------------------------
// boundary confidence: the second pass over the prefix sums
// ------------------------------------------------------------------------------------
// With P* = P(p*) and p* as the kernel above left them on the device, per boundary
//     lower / upper / n_within = the smallest / the largest / the number of p in [lo, hi] with P(p) >= P* - drop_q   (exact)
//     w(p) = exp(-(P* - P(p)) 2^-16), 0 where P* - P(p) > 700 * 2^16 (an integer comparison)                         (float64)
//     Z = sum w, M = sum of w over lower <= p <= upper, S1_left = sum_{p < p*} (p* - p) w, S1_right = sum_{p > p*} (p - p*) w,
//     S2 = sum (p - p*)^2 w
// One wave per boundary, 1024 k-mer starts per pass.  The walk is laid on the boundary itself, not on the packed words: lane l
// of pass t holds the starts lo + 1024 t + 16 l + j, j = 0 .. 15 (its bits shifted out of three packed words), so which lane
// and pass a candidate falls to -- and with it the order of every float64 sum -- depends on lo and hi alone, not on where the
// sequence lies in the stream.  Two walks: the first reduces the three integers (min, max, sum: any order), the second, which
// needs lower and upper for M, the five sums in this order: the candidate lo, then per pass the lane's candidates in order of
// p from 0.0, the lanes by the xor butterfly 32, 16, .. 1, the pass's total onto the running sum.
#define PHK_CONF_CUT (700ll << 16)

// the 16 valid bits / the 64 bits of packed bases from base s on (s in word w at offset o); wlast: the interval's last word --
// no k-mer that starts inside the interval reaches past word wlast + 1, and the kernel above reads as far
__device__ __forceinline__ uint32_t conf_validbits(const uint32_t *__restrict__ mask, uint64_t w, uint32_t o, uint64_t wlast, int K) {
    const uint32_t v0 = refine_validbits(mask, w, K) & 0xffffu;
    const uint32_t v1 = refine_validbits(mask, w < wlast ? w + 1 : wlast, K) & 0xffffu;   // (clamped: starts past hi, masked)
    return ((v0 | (v1 << 16)) >> o) & 0xffffu;
}

__device__ __forceinline__ uint64_t conf_bases(const uint32_t *__restrict__ packed, uint64_t w, uint32_t o, uint64_t wlast) {
    const uint32_t a = packed[w], b = packed[w + 1], c = packed[w + 2 <= wlast + 1 ? w + 2 : wlast + 1];
    const uint64_t X = ((uint64_t)a << 32) | b;
    return o ? (X << (2 * o)) | (uint64_t)(c >> (32 - 2 * o)) : X;
}

// d of the j-th start of a lane whose 64 bits of bases are X (0 for a k-mer that is not valid)
template <bool TABLE>
__device__ __forceinline__ long long conf_diff(uint64_t X, int j, int K, uint32_t dmask, uint32_t ok, const long long *drow,
                                               const long long *__restrict__ ql, const long long *__restrict__ qr) {
    const uint32_t idx = (uint32_t)(X >> (64 - 2 * K - 2 * j)) & dmask;
    if (TABLE) return (ok >> j) & 1u ? drow[idx] : 0ll;
    return (ok >> j) & 1u ? ql[idx] - qr[idx] : 0ll;
}

// the candidate p with prefix sum P joins the five sums
__device__ __forceinline__ void conf_add(long long P, uint64_t p, long long best_v, uint64_t best_p, uint64_t lower, uint64_t upper,
                                         double &z, double &m, double &s1l, double &s1r, double &s2) {
    const long long delta = best_v - P;                      // >= 0
    if (delta > PHK_CONF_CUT) return;
    const double w = exp(-(double)delta * 0x1p-16);          // (the argument is exact)
    z += w;
    if (p >= lower && p <= upper) m += w;
    const long long dp = (long long)(p - best_p);
    if (dp < 0) s1l += (double)(-dp) * w;
    if (dp > 0) s1r += (double)dp * w;
    s2 += (double)(dp * dp) * w;
}

__device__ __forceinline__ double conf_wave_sum(double v) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh);
    return v;
}

template <bool TABLE>
__global__ __launch_bounds__(64 * PHK_REFINE_WAVES) void phk_boundary_confidence_kernel(
    const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask, const long long *__restrict__ q, uint32_t D, int K,
    const PhkRefineJob *__restrict__ jobs, uint64_t B, const long long *__restrict__ position, const long long *__restrict__ evidence,
    long long drop_q, long long *__restrict__ interval, double *__restrict__ sums) {
    __shared__ __attribute__((aligned(16))) long long rows_s[TABLE ? PHK_REFINE_WAVES * PHK_REFINE_LDS_D : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long *drow = rows_s + (TABLE ? wave * PHK_REFINE_LDS_D : 0);
    const uint32_t dmask = D - 1u;
    for (uint64_t bi = (uint64_t)blockIdx.x * PHK_REFINE_WAVES + wave; bi < B; bi += (uint64_t)gridDim.x * PHK_REFINE_WAVES) {
        const PhkRefineJob job = jobs[bi];
        const uint64_t lo = job.lo, hi = job.hi;
        const uint64_t ve = job.vend < hi ? job.vend : hi;   // valid k-mer starts lie in [lo, ve)
        const long long *ql = q + (uint64_t)job.left * D, *qr = q + (uint64_t)job.right * D;
        const long long best_v = evidence[3 * bi + 1];       // P* (= P* - P(lo))
        const uint64_t best_p = job.base + (uint64_t)position[bi];
        const long long thr = best_v - drop_q;               // (P* <= 2^62, drop_q >= 0: inside int64)
        uint64_t lower = ~0ull, upper = 0;
        uint32_t cnt = 0;
        if (0 >= thr) {                                      // the candidate p = lo: P = 0
            lower = upper = lo;
            cnt = lane == 0;
        }
        double Z = 0.0, M = 0.0, S1L = 0.0, S1R = 0.0, S2 = 0.0;
        const uint64_t wlast = hi > lo ? (hi - 1) >> 4 : lo >> 4;
        if (TABLE && hi > lo) {
            refine_wave_sync();                              // the previous boundary's gathers are done
            for (uint32_t c = lane; c < D; c += 64) drow[c] = ql[c] - qr[c];
            refine_wave_sync();
        }
        for (int phase = 0; phase < 2; ++phase) {
            if (phase == 1) {
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) {
                    const uint64_t ol = __shfl_xor(lower, sh), ou = __shfl_xor(upper, sh);
                    lower = ol < lower ? ol : lower;
                    upper = ou > upper ? ou : upper;
                    cnt += __shfl_xor(cnt, sh);
                }
                conf_add(0, lo, best_v, best_p, lower, upper, Z, M, S1L, S1R, S2);
            }
            long long carry = 0;
            for (uint64_t sb = lo; sb < hi; sb += 1024) {
                const uint64_t s0 = sb + 16 * (uint64_t)lane;
                const bool act = s0 < hi;
                const uint64_t sc = act ? s0 : hi - 1;       // (an idle lane loads what the last busy one may)
                const uint64_t w = sc >> 4;
                const uint32_t o = (uint32_t)(sc & 15);
                const uint32_t inr = act ? refine_rangebits(sc, lo, hi) : 0u;
                const uint32_t ok = act ? refine_rangebits(sc, lo, ve) & conf_validbits(mask, w, o, wlast, K) : 0u;
                const uint64_t X = conf_bases(packed, w, o, wlast);
                long long s = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) s += conf_diff<TABLE>(X, j, K, dmask, ok, drow, ql, qr);
                long long inc = s;                           // exclusive scan of the lanes' totals
#pragma unroll
                for (int sh = 1; sh < 64; sh <<= 1) {
                    const long long t = __shfl_up(inc, sh);
                    if (lane >= sh) inc += t;
                }
                // the lane's candidates p = sc + j + 1 in order, their differences gathered again (a rolled loop: one body of
                // the exp, not sixteen, and no array of differences to keep)
                long long P = carry + (inc - s);
                double z = 0.0, m = 0.0, s1l = 0.0, s1r = 0.0, s2 = 0.0;
#pragma unroll 2
                for (int j = 0; j < 16; ++j) {
                    P += conf_diff<TABLE>(X, j, K, dmask, ok, drow, ql, qr);
                    if (!((inr >> j) & 1u)) continue;
                    const uint64_t p = sc + j + 1;
                    if (phase == 1) {
                        conf_add(P, p, best_v, best_p, lower, upper, z, m, s1l, s1r, s2);
                    } else if (P >= thr) {
                        lower = p < lower ? p : lower;
                        upper = p > upper ? p : upper;
                        ++cnt;
                    }
                }
                if (phase == 1) {
                    Z += conf_wave_sum(z);
                    M += conf_wave_sum(m);
                    S1L += conf_wave_sum(s1l);
                    S1R += conf_wave_sum(s1r);
                    S2 += conf_wave_sum(s2);
                }
                carry += __shfl(inc, 63);
            }
        }
        if (lane == 0) {
            interval[3 * bi + 0] = (long long)(lower - job.base);
            interval[3 * bi + 1] = (long long)(upper - job.base);
            interval[3 * bi + 2] = (long long)cnt;
            sums[5 * bi + 0] = Z;
            sums[5 * bi + 1] = M;
            sums[5 * bi + 2] = S1L;
            sums[5 * bi + 3] = S1R;
            sums[5 * bi + 4] = S2;
        }
    }
}

extern "C" uint64_t phk_refine_grid_pass(void) { return (uint64_t)PHK_REFINE_BLOCKS_MAX * PHK_REFINE_WAVES; }

// ------------------------------------------------------------------------------------
// checks (before any launch) and launch
// ------------------------------------------------------------------------------------
static int refine_check(const char *fname, const uint64_t *offsets, uint64_t n_seq, int k, const char *sym, const int64_t *qtable,
                        uint64_t n_rows, uint64_t D, const uint64_t *seq, const uint64_t *lo, const uint64_t *x,
                        const uint64_t *hi, const uint32_t *left_row, const uint32_t *right_row, uint64_t B,
                        const int64_t *position, const int64_t *evidence, const uint32_t *support) {
    PHK_REQUIRE(k >= 1, "%s: k must be >= 1 (got %d)", fname, k);
    if (k > PHK_MAX_K) {
        phk_set_error("%s: k=%d is above PHK_MAX_K=%d", fname, k, PHK_MAX_K);
        return PHK_ERR_UNSUPPORTED;
    }
    PHK_REQUIRE(D == phk_pow4(k), "%s: the table has %llu columns, 4^k = %llu", fname, (unsigned long long)D,
                (unsigned long long)phk_pow4(k));
    PHK_REQUIRE(strlen(sym) == 4, "%s: symbols must be exactly 4 characters", fname);
    PHK_REQUIRE(n_seq == 0 || offsets, "%s: NULL offsets", fname);
    if (n_seq) {
        PHK_REQUIRE(offsets[0] == 0, "%s: offsets[0] must be 0", fname);
        for (uint64_t c = 0; c < n_seq; ++c) PHK_REQUIRE(offsets[c + 1] >= offsets[c], "%s: offsets must be non-decreasing", fname);
    }
    PHK_REQUIRE(n_rows == 0 || qtable, "%s: NULL table", fname);
    for (uint64_t i = 0; i < n_rows * D; ++i)
        PHK_REQUIRE(qtable[i] >= -PHK_REFINE_MAX_Q && qtable[i] <= PHK_REFINE_MAX_Q, "%s: table entry %llu is outside [-2^31, 2^31]", fname,
                    (unsigned long long)i);
    if (B == 0) return PHK_OK;
    PHK_REQUIRE(seq && lo && x && hi && left_row && right_row && position && evidence && support, "%s: NULL argument", fname);
    for (uint64_t b = 0; b < B; ++b) {
        PHK_REQUIRE(seq[b] < n_seq, "%s: boundary %llu names sequence %llu of %llu", fname, (unsigned long long)b,
                    (unsigned long long)seq[b], (unsigned long long)n_seq);
        PHK_REQUIRE(left_row[b] < n_rows && right_row[b] < n_rows, "%s: boundary %llu names a table row outside the %llu rows", fname,
                    (unsigned long long)b, (unsigned long long)n_rows);
        const uint64_t L = offsets[seq[b] + 1] - offsets[seq[b]];
        PHK_REQUIRE(lo[b] <= x[b] && x[b] <= hi[b], "%s: boundary %llu needs lo <= x <= hi", fname, (unsigned long long)b);
        PHK_REQUIRE(hi[b] - lo[b] <= PHK_REFINE_MAX_SPAN, "%s: boundary %llu spans more than 2^30 bases", fname, (unsigned long long)b);
        PHK_REQUIRE(hi[b] <= L, "%s: boundary %llu ends at base %llu of a sequence of %llu", fname, (unsigned long long)b,
                    (unsigned long long)hi[b], (unsigned long long)L);
    }
    return PHK_OK;
}

// d_packed / d_mask: the packed stream of the sequences `offsets` (host) describes.  Everything past the pack.  With
// `interval` (and `sums`) the confidence kernel follows the refinement kernel on the stream and reads its device outputs.
static int refine_run(phk_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *offsets, int k,
                      const int64_t *qtable, uint64_t n_rows, uint64_t D, const uint64_t *seq, const uint64_t *lo, const uint64_t *x,
                      const uint64_t *hi, const uint32_t *left_row, const uint32_t *right_row, uint64_t B, int64_t *position,
                      int64_t *evidence, uint32_t *support, int64_t drop_q = 0, int64_t *interval = nullptr, double *sums = nullptr) {
    std::vector<PhkRefineJob> jobs(B);
    for (uint64_t b = 0; b < B; ++b) {
        const uint64_t base = offsets[seq[b]], L = offsets[seq[b] + 1] - base;
        PhkRefineJob &j = jobs[b];
        j.base = base;
        j.lo = base + lo[b];
        j.x = base + x[b];
        j.hi = base + hi[b];
        j.vend = base + (L >= (uint64_t)k ? L - k + 1 : 0);
        j.left = left_row[b];
        j.right = right_row[b];
    }
    void *d_q, *d_jobs, *d_out;
    PHK_TRY(phk_ws(ctx, WS_WIDE, n_rows * D * 8, &d_q));
    PHK_TRY(phk_ws(ctx, WS_LONG, B * sizeof(PhkRefineJob), &d_jobs));
    PHK_TRY(phk_ws(ctx, WS_OUT, B * (interval ? 100 : 36), &d_out));
    PHK_TRY(phk_copy_to_device(ctx, d_q, qtable, n_rows * D * 8));
    PHK_TRY(phk_copy_to_device(ctx, d_jobs, jobs.data(), B * sizeof(PhkRefineJob)));
    long long *d_pos = (long long *)d_out, *d_ev = d_pos + B, *d_int = d_ev + 3 * B;   // (the 8-byte outputs first)
    double *d_sums = (double *)(d_int + 3 * B);
    uint32_t *d_sup = interval ? (uint32_t *)(d_sums + 5 * B) : (uint32_t *)(d_ev + 3 * B);
    uint64_t blocks = phk_div_up(B, PHK_REFINE_WAVES);
    if (blocks > PHK_REFINE_BLOCKS_MAX) blocks = PHK_REFINE_BLOCKS_MAX;
    if (D <= PHK_REFINE_LDS_D)
        PHK_LAUNCH(ctx, "phk_refine_boundaries_kernel",
                   phk_refine_boundaries_kernel<true><<<dim3((unsigned)blocks), dim3(64 * PHK_REFINE_WAVES), 0, ctx->stream>>>(
                       d_packed, d_mask, (const long long *)d_q, (uint32_t)D, k, (const PhkRefineJob *)d_jobs, B, d_pos, d_ev, d_sup));
    else
        PHK_LAUNCH(ctx, "phk_refine_boundaries_kernel",
                   phk_refine_boundaries_kernel<false><<<dim3((unsigned)blocks), dim3(64 * PHK_REFINE_WAVES), 0, ctx->stream>>>(
                       d_packed, d_mask, (const long long *)d_q, (uint32_t)D, k, (const PhkRefineJob *)d_jobs, B, d_pos, d_ev, d_sup));
    if (interval && D <= PHK_REFINE_LDS_D)
        PHK_LAUNCH(ctx, "phk_boundary_confidence_kernel",
                   phk_boundary_confidence_kernel<true><<<dim3((unsigned)blocks), dim3(64 * PHK_REFINE_WAVES), 0, ctx->stream>>>(
                       d_packed, d_mask, (const long long *)d_q, (uint32_t)D, k, (const PhkRefineJob *)d_jobs, B, d_pos, d_ev,
                       (long long)drop_q, d_int, d_sums));
    else if (interval)
        PHK_LAUNCH(ctx, "phk_boundary_confidence_kernel",
                   phk_boundary_confidence_kernel<false><<<dim3((unsigned)blocks), dim3(64 * PHK_REFINE_WAVES), 0, ctx->stream>>>(
                       d_packed, d_mask, (const long long *)d_q, (uint32_t)D, k, (const PhkRefineJob *)d_jobs, B, d_pos, d_ev,
                       (long long)drop_q, d_int, d_sums));
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // (the job table is a host vector)
    PHK_TRY(phk_copy_to_host(ctx, position, d_pos, B * 8));
    PHK_TRY(phk_copy_to_host(ctx, evidence, d_ev, B * 24));
    if (interval) {
        PHK_TRY(phk_copy_to_host(ctx, interval, d_int, B * 24));
        PHK_TRY(phk_copy_to_host(ctx, sums, d_sums, B * 40));
    }
    return phk_copy_to_host(ctx, support, d_sup, B * 4);
}

// ------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------
// both entries: the checks, the bases up and packed, the kernels; `confidence`: drop_q, interval and sums are part of the call
static int refine_ascii(phk_ctx *ctx, const char *fname, const char *bases, const uint64_t *seq_offsets, uint64_t n_seq, int k,
                        const char *symbols4, const int64_t *qtable, uint64_t n_rows, uint64_t D, const uint64_t *seq,
                        const uint64_t *lo, const uint64_t *x, const uint64_t *hi, const uint32_t *left_row, const uint32_t *right_row,
                        uint64_t B, int64_t *position, int64_t *evidence, uint32_t *support, bool confidence, int64_t drop_q,
                        int64_t *interval, double *sums) {
    const char *sym = symbols4 ? symbols4 : "ATGC";
    PHK_TRY(refine_check(fname, seq_offsets, n_seq, k, sym, qtable, n_rows, D, seq, lo, x, hi, left_row, right_row, B, position,
                         evidence, support));
    if (confidence) PHK_REQUIRE(drop_q >= 0, "%s: drop_q must be >= 0 (got %lld)", fname, (long long)drop_q);
    if (B == 0) return PHK_OK;
    if (confidence) PHK_REQUIRE(interval && sums, "%s: NULL argument", fname);
    const uint64_t T = seq_offsets[n_seq];
    PHK_REQUIRE(T == 0 || bases, "%s: NULL bases", fname);
    void *d_ascii, *d_packed, *d_mask;
    PHK_TRY(phk_ws(ctx, WS_ASCII, T, &d_ascii));
    PHK_TRY(phk_ws(ctx, WS_PACKED, (phk_div_up(T, 16) + 1) * 4, &d_packed));
    PHK_TRY(phk_ws(ctx, WS_MASK, (phk_div_up(T, 32) + 1) * 4, &d_mask));
    if (T) PHK_TRY(phk_copy_to_device(ctx, d_ascii, bases, T));
    PHK_TRY(phk_launch_pack(ctx, (const char *)d_ascii, T, sym, (uint32_t *)d_packed, (uint32_t *)d_mask, nullptr));
    return refine_run(ctx, (const uint32_t *)d_packed, (const uint32_t *)d_mask, seq_offsets, k, qtable, n_rows, D, seq, lo, x, hi,
                      left_row, right_row, B, position, evidence, support, drop_q, confidence ? interval : nullptr, sums);
}

extern "C" int phk_refine_boundaries_ascii(phk_ctx *ctx, const char *bases, const uint64_t *seq_offsets, uint64_t n_seq, int k,
                                           const char *symbols4, const int64_t *qtable, uint64_t n_rows, uint64_t D,
                                           const uint64_t *seq, const uint64_t *lo, const uint64_t *x, const uint64_t *hi,
                                           const uint32_t *left_row, const uint32_t *right_row, uint64_t B, int64_t *position,
                                           int64_t *evidence, uint32_t *support) {
    PHK_ENTER(ctx, "phk_refine_boundaries_ascii");
    return refine_ascii(ctx, "phk_refine_boundaries_ascii", bases, seq_offsets, n_seq, k, symbols4, qtable, n_rows, D, seq, lo, x, hi,
                        left_row, right_row, B, position, evidence, support, false, 0, nullptr, nullptr);
}

extern "C" int phk_refine_confidence_ascii(phk_ctx *ctx, const char *bases, const uint64_t *seq_offsets, uint64_t n_seq, int k,
                                           const char *symbols4, const int64_t *qtable, uint64_t n_rows, uint64_t D,
                                           const uint64_t *seq, const uint64_t *lo, const uint64_t *x, const uint64_t *hi,
                                           const uint32_t *left_row, const uint32_t *right_row, uint64_t B, int64_t drop_q,
                                           int64_t *position, int64_t *evidence, uint32_t *support, int64_t *interval, double *sums) {
    PHK_ENTER(ctx, "phk_refine_confidence_ascii");
    return refine_ascii(ctx, "phk_refine_confidence_ascii", bases, seq_offsets, n_seq, k, symbols4, qtable, n_rows, D, seq, lo, x, hi,
                        left_row, right_row, B, position, evidence, support, true, drop_q, interval, sums);
}
