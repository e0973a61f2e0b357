// sweep.hip -- the silhouette-against-k sweep of scripts/cluster.py:31-47 (KMeans(k, random_state) for a grid of k on one
// feature matrix, the mean silhouette of each fit) as batched k-means: the SAME rows, a different k -- and, if the caller
// wants, a different seed -- per problem.  gfx950.  (placement.hip batches along the other axis: one k, one more row each.)
//
// The rows X[n][D] are resident (phk_sweep_create), raw and centred by their column mean (NumPy's X - X.mean(axis=0), bit
// for bit: what KMeans.fit and learning.kmeans_reference_on_device run on).  phk_sweep_run solves S problems in chunks of
// problems, every stage one launch for the whole chunk, the grid's second dimension the problem:
//   seeding  : scikit-learn's k-means++ with the caller's draws (learning.kmeans_plusplus_seeds is the specification), the two
//              launches per centre of placement.hip: direct-difference distances of the step's trial rows to all rows, then
//              one workgroup per problem for the potentials (256 contiguous slices in index order, then the slice sums in
//              order), the greedy choice, the prefix sum and its search.  A problem whose k_s centres are chosen returns at
//              once: a chunk costs 2 max k_s launches, not 2 sum k_s.  The closest call is reported as seed_margin
//              (DESIGN.md 4.9);
//   Lloyd    : kmeans.hip's phk_kmeans_lloyd iteration on the centred rows, operation order included (labels, sweep counts
//              and min_gap equal the single-problem path's bit for bit), each problem with its own centres, labels, stopping
//              flags and sweep count; the host reads one word per sweep for the chunk, finished problems return at once;
//   silhouettes of all rows : the pair distances d[n][n] (raw rows, float64 direct differences by fma in column order,
//              pair_tile.h) do not depend on the problem: they are computed ONCE per call; per problem a thread per row
//              then adds, cluster by cluster, the stored distances in exactly the order phk_cl_silhouette_sums_kernel
//              takes them and applies phk_cl_silhouette_finish_kernel's rules: equal to phk_silhouettes bit for bit.
//              Budget: d takes n^2 * 8 bytes; when that exceeds the caller's budget (default: a quarter of the free device
//              memory at the call) the problems go one after the other through phk_silhouettes' own pass on the resident
//              rows instead: same bits, the pair pass paid per problem.
// Everything is float64 and order-deterministic (the only atomics are integer counts and minima); every sum's order is
// fixed by n, the labels and the problem alone, so a problem's result does not depend on S, on its place or on `chunk`.
#include "pair_tile.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#define SW_MAX_TRIALS 10      // 2 + int(ln k): k < 2981
#define SW_ROWS_SEED 4        // rows per wave of the seeding's distance kernel
#define SW_ROWS_ASSIGN 8      // rows per wave of the E-step
#define SW_DEFAULT_CHUNK 64

struct SwState {              // per problem, device
    uint32_t k, T;            // centres; seeding trials per centre
    uint32_t koff;            // centres of the chunk's problems before this one
    uint32_t changed;         // labels changed in the running E-step (zeroed by the stopping kernel)
    uint32_t active;          // still sweeping
    uint32_t strict;          // stopped because no label changed (no extra E-step)
    uint32_t n_iter;
    uint32_t n_empty;         // empty clusters met, summed over the sweeps
    uint32_t cur;             // which of the two centre buffers holds the current centres
    uint32_t pad;
    uint64_t doff;            // first draw of the problem in the chunk's draws
    double pot;               // seeding: current potential
    double seed_margin;
    double tol;
    unsigned long long gapbits;
};

struct phk_sweep {
    uint64_t n = 0, D = 0;
    double *d_x = nullptr;    // raw rows
    double *d_xc = nullptr;   // centred rows
    double var_mean = 0.0;    // np.mean(np.var(centred rows, axis=0))
    void *ws = nullptr;
    uint64_t ws_bytes = 0;
    double *d_pair = nullptr; // d[n][n], kept between calls
};

struct SwView {
    const double *Xc;       // [n][D] centred
    double *cen;            // per problem [2][k][D] at 2 * koff * D
    uint32_t *labels;       // [Sc][n]
    double *closest;        // [Sc][n]
    double *td;             // [Sc][SW_MAX_TRIALS][n]
    uint32_t *cand;         // [Sc][SW_MAX_TRIALS]
    uint32_t *seeds;        // per problem [k] at koff
    uint32_t *sizes;        // per problem [k] at koff
    SwState *st;            // [Sc]
    const double *draws;    // the chunk's draws
    uint64_t n, D;
};

__device__ __forceinline__ uint64_t sw_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- seeding --------------------------------------------------------------------------------------------------------
// Squared distances of the step's trial rows to every row, min-ed with the running closest distances (not at the first
// centre).  One wave per SW_ROWS_SEED rows; float64 direct differences of the centred rows, fma in column order.
__global__ __launch_bounds__(256) void sw_seed_dist_kernel(SwView v, uint32_t step) {
    const uint32_t b = blockIdx.y;
    const SwState *st = v.st + b;
    if (step >= st->k) return;
    const uint32_t ntr = step == 0 ? 1u : st->T;
    const int lane = threadIdx.x & 63;
    const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t i0 = w * SW_ROWS_SEED;
    if (i0 >= v.n) return;
    const double *rows[SW_ROWS_SEED], *cr[SW_MAX_TRIALS];
#pragma unroll
    for (int r = 0; r < SW_ROWS_SEED; ++r) rows[r] = v.Xc + sw_min(i0 + r, v.n - 1) * v.D;
#pragma unroll
    for (int t = 0; t < SW_MAX_TRIALS; ++t)
        cr[t] = v.Xc + sw_min(v.cand[(uint64_t)b * SW_MAX_TRIALS + (t < (int)ntr ? t : 0)], v.n - 1) * v.D;
    double acc[SW_ROWS_SEED][SW_MAX_TRIALS];
#pragma unroll
    for (int r = 0; r < SW_ROWS_SEED; ++r)
#pragma unroll
        for (int t = 0; t < SW_MAX_TRIALS; ++t) acc[r][t] = 0.0;
    for (uint64_t d = lane; d < v.D; d += 64) {
        double x[SW_ROWS_SEED];
#pragma unroll
        for (int r = 0; r < SW_ROWS_SEED; ++r) x[r] = rows[r][d];
#pragma unroll
        for (int t = 0; t < SW_MAX_TRIALS; ++t)
            if (t < (int)ntr) {
                const double c = cr[t][d];
#pragma unroll
                for (int r = 0; r < SW_ROWS_SEED; ++r) {
                    const double e = x[r] - c;
                    acc[r][t] = fma(e, e, acc[r][t]);
                }
            }
    }
#pragma unroll
    for (int t = 0; t < SW_MAX_TRIALS; ++t)
        if (t < (int)ntr) {
#pragma unroll
            for (int r = 0; r < SW_ROWS_SEED; ++r) {
                double a = acc[r][t];
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s);
                const uint64_t i = i0 + r;
                if (lane == 0 && i < v.n) {
                    const double old = v.closest[(uint64_t)b * v.n + i];
                    v.td[((uint64_t)b * SW_MAX_TRIALS + t) * v.n + i] = step == 0 ? a : fmin(old, a);
                }
            }
        }
}

// One workgroup per problem.  Centre `step`: the potentials of its trials (slice sums of 256 contiguous slices in index
// order, then the 256 partials in order), the greedy choice (first smallest), the gap to the best trial on ANOTHER row; the
// chosen row becomes centre `step`.  Then, for centre step + 1: the prefix sum of the closest distances in the same order
// and, per draw u, the first row whose prefix reaches u * potential (np.searchsorted(np.cumsum(closest), u * pot)), with
// the draw's distance to the two prefix values around it.
__global__ __launch_bounds__(256) void sw_seed_choose_kernel(SwView v, uint32_t step) {
    __shared__ double part[SW_MAX_TRIALS][256];
    __shared__ double pots[SW_MAX_TRIALS];
    __shared__ double pre[257];
    __shared__ uint32_t s_best, s_cand[SW_MAX_TRIALS], s_claim[SW_MAX_TRIALS];
    __shared__ unsigned long long s_mbits[SW_MAX_TRIALS];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    SwState *st = v.st + b;
    const uint32_t k = st->k, T = st->T;
    if (step >= k) return;
    const uint32_t ntr = step == 0 ? 1u : T;
    const double *draws = step + 1 < k ? v.draws + st->doff + (uint64_t)step * T : nullptr;
    const uint64_t n = v.n;
    const uint64_t per = (n + 255) / 256, lo = sw_min(per * t, n), hi = sw_min(lo + per, n);
    const double *td = v.td + (uint64_t)b * SW_MAX_TRIALS * n;
    uint32_t *cand = v.cand + (uint64_t)b * SW_MAX_TRIALS;
    for (uint32_t tr = 0; tr < ntr; ++tr) {
        double s = 0.0;
        for (uint64_t i = lo; i < hi; ++i) s += td[tr * n + i];
        part[tr][t] = s;
    }
    __syncthreads();
    if (t < (int)ntr) {
        double total = 0.0;
        for (int j = 0; j < 256; ++j) total += part[t][j];
        pots[t] = total;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t best = 0;
        for (uint32_t tr = 1; tr < ntr; ++tr)
            if (pots[tr] < pots[best]) best = tr;
        double margin = st->seed_margin;
        for (uint32_t tr = 0; tr < ntr; ++tr)
            if (cand[tr] != cand[best]) {
                const double g = (pots[tr] - pots[best]) / pots[best];
                margin = g == g ? fmin(margin, g) : 0.0;
            }
        if (!(pots[best] > 0.0) && step + 1 < k) margin = 0.0;   // nothing left to draw from: every row is a centre already
        st->seed_margin = margin;
        st->pot = pots[best];
        v.seeds[st->koff + step] = cand[best];
        s_best = best;
    }
    __syncthreads();
    const uint32_t best = s_best;
    {   // centre `step` = the chosen centred row; the running closest distances = the chosen trial's
        const double *src = v.Xc + (uint64_t)cand[best] * v.D;
        double *cen = v.cen + ((uint64_t)2 * st->koff + step) * v.D;
        for (uint64_t d = t; d < v.D; d += 256) cen[d] = src[d];
        double *closest = v.closest + (uint64_t)b * n;
        for (uint64_t i = lo; i < hi; ++i) closest[i] = td[best * n + i];
    }
    if (draws == nullptr) return;
    if (t == 0) {
        double run = 0.0;
        for (int j = 0; j < 256; ++j) { pre[j] = run; run += part[best][j]; }
        pre[256] = run;
    }
    if (t < SW_MAX_TRIALS) {
        s_cand[t] = 0xFFFFFFFFu;
        s_claim[t] = 0;
        s_mbits[t] = (unsigned long long)__double_as_longlong((double)INFINITY);
    }
    __syncthreads();
    const double pot = pots[best];
    for (uint32_t tr = 0; tr < T; ++tr) {
        const double val = draws[tr] * pot;
        double run = pre[t];
        if (run < val) {
            for (uint64_t i = lo; i < hi; ++i) {
                const double prev = run;
                run += td[best * n + i];
                if (run >= val) {
                    atomicMin(&s_cand[tr], (uint32_t)i);
                    atomicAdd(&s_claim[tr], 1u);
                    const double m = fmin(run - val, val - prev) / pot;
                    atomicMin(&s_mbits[tr], (unsigned long long)__double_as_longlong(m >= 0.0 ? m : 0.0));
                    break;
                }
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        double margin = st->seed_margin;
        for (uint32_t tr = 0; tr < T; ++tr) {
            // exactly one slice holds the first row that reaches the draw; none or two (the slices' own roundings) is a draw
            // within rounding of a prefix value, and so is a draw past the total: margin 0
            const double m = s_claim[tr] == 1 ? __longlong_as_double((long long)s_mbits[tr]) : 0.0;
            margin = m == m ? fmin(margin, m) : 0.0;
            cand[tr] = s_cand[tr] < n ? s_cand[tr] : (uint32_t)(n - 1);
        }
        st->seed_margin = margin;
    }
}

// ---- Lloyd ----------------------------------------------------------------------------------------------------------
// km_assign_kernel (kmeans.hip) for a chunk of problems: the same per-point arithmetic -- lane l sums columns l, l + 64, ...
// of x - centre by fma, the butterfly, the strict comparison that keeps the lower centre index -- with SW_ROWS_ASSIGN rows
// per wave sharing each centre value they load.  final = 1: the extra E-step of the problems that stopped on the shift.
__global__ __launch_bounds__(256) void sw_assign_kernel(SwView v, int final) {
    const uint32_t b = blockIdx.y;
    SwState *st = v.st + b;
    if (final ? (st->strict != 0) : (st->active == 0)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t i0 = w * SW_ROWS_ASSIGN;
    if (i0 >= v.n) return;
    const uint32_t k = st->k;
    const double *cen = v.cen + ((uint64_t)2 * st->koff + (uint64_t)st->cur * k) * v.D;
    const double *rows[SW_ROWS_ASSIGN];
#pragma unroll
    for (int r = 0; r < SW_ROWS_ASSIGN; ++r) rows[r] = v.Xc + sw_min(i0 + r, v.n - 1) * v.D;
    double best[SW_ROWS_ASSIGN], second[SW_ROWS_ASSIGN];
    uint32_t bi[SW_ROWS_ASSIGN];
#pragma unroll
    for (int r = 0; r < SW_ROWS_ASSIGN; ++r) { best[r] = INFINITY; second[r] = INFINITY; bi[r] = 0; }
    for (uint32_t c = 0; c < k; ++c) {
        double acc[SW_ROWS_ASSIGN];
#pragma unroll
        for (int r = 0; r < SW_ROWS_ASSIGN; ++r) acc[r] = 0.0;
        const double *cc = cen + (uint64_t)c * v.D;
        for (uint64_t d = lane; d < v.D; d += 64) {
            const double cv = cc[d];
#pragma unroll
            for (int r = 0; r < SW_ROWS_ASSIGN; ++r) {
                const double e = rows[r][d] - cv;
                acc[r] = fma(e, e, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < SW_ROWS_ASSIGN; ++r) {
            double a = acc[r];
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s);
            if (a < best[r]) { second[r] = best[r]; best[r] = a; bi[r] = c; }
            else if (a < second[r]) second[r] = a;
        }
    }
    if (lane == 0) {
        uint32_t *labels = v.labels + (uint64_t)b * v.n;
#pragma unroll
        for (int r = 0; r < SW_ROWS_ASSIGN; ++r) {
            const uint64_t i = i0 + r;
            if (i >= v.n) continue;
            if (labels[i] != bi[r]) atomicAdd(&st->changed, 1u);
            labels[i] = bi[r];
            if (k > 1 && second[r] > 0.0 && second[r] < INFINITY)
                atomicMin(&st->gapbits, (unsigned long long)__double_as_longlong((second[r] - best[r]) / second[r]));
        }
    }
}

// km_update_kernel for a chunk: new centre = mean of the members' rows in index order, written to the other centre buffer
// (an empty cluster keeps its centre); one workgroup per (centre, problem)
__global__ __launch_bounds__(256) void sw_update_kernel(SwView v) {
    const uint32_t c = blockIdx.x, b = blockIdx.y;
    SwState *st = v.st + b;
    const uint32_t k = st->k;
    if (st->active == 0 || c >= k) return;
    const double *old = v.cen + ((uint64_t)2 * st->koff + (uint64_t)st->cur * k + c) * v.D;
    double *cen = v.cen + ((uint64_t)2 * st->koff + (uint64_t)(st->cur ^ 1u) * k + c) * v.D;
    const uint32_t *labels = v.labels + (uint64_t)b * v.n;
    uint32_t cnt = 0;
    for (uint64_t d = threadIdx.x; d < v.D; d += 256) {
        double s = 0.0;
        uint32_t m = 0;
        for (uint64_t i = 0; i < v.n; ++i)
            if (labels[i] == c) { s += v.Xc[i * v.D + d]; ++m; }
        cen[d] = m ? s / (double)m : old[d];
        cnt = m;
    }
    if (threadIdx.x == 0) v.sizes[st->koff + c] = cnt;
}

// km_shift_kernel + the host's stopping rule, per problem: total squared centre shift (same summation order), empty
// clusters, then "no label changed" (strict) or "shift <= tol" (one more E-step).  The new centres become current.
__global__ __launch_bounds__(256) void sw_stop_kernel(SwView v, uint32_t *__restrict__ n_active) {
    __shared__ double part[256];
    const uint32_t b = blockIdx.x;
    SwState *st = v.st + b;
    if (st->active == 0) return;
    const uint32_t k = st->k;
    const uint64_t count = (uint64_t)k * v.D;
    const double *base = v.cen + (uint64_t)2 * st->koff * v.D;
    const double *old = base + (uint64_t)st->cur * count, *cen = base + (uint64_t)(st->cur ^ 1u) * count;
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < count; i += 256) {
        const double d = cen[i] - old[i];
        s = fma(d, d, s);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double shift = 0.0;
        for (int i = 0; i < 256; ++i) shift += part[i];
        uint32_t e = 0;
        for (uint32_t c = 0; c < k; ++c) e += v.sizes[st->koff + c] == 0 ? 1u : 0u;
        st->n_empty += e;
        st->n_iter += 1;
        st->cur ^= 1u;
        if (st->changed == 0) { st->strict = 1; st->active = 0; }
        else if (shift <= st->tol) st->active = 0;
        st->changed = 0;
        if (st->active) atomicAdd(n_active, 1u);
    }
}

// ---- silhouettes ----------------------------------------------------------------------------------------------------
// d[q][j] = sqrt(sum_k (x_qk - x_jk)^2) for all pairs of the raw rows: pair_tile.h's tile, one workgroup per 64 x 64 tile
// (tile row = blockIdx.y + y0).  The same bits for (q, j) and (j, q).
__global__ __launch_bounds__(CL_THREADS) void sw_pair_kernel(const double *__restrict__ X, uint64_t n, uint64_t D, uint64_t y0,
                                                            double *__restrict__ dist) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t qbase = (y0 + blockIdx.y) * CL_T, cbase = (uint64_t)blockIdx.x * CL_T;
    double s[4][4];
    cl_tile(X, D, nullptr, n, qbase, nullptr, n, cbase, Qs, Cs, s);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t q = qbase + ty + 16 * r;
        if (q >= n) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t j = cbase + tx + 16 * c;
            if (j < n) dist[q * n + j] = sqrt(s[r][c]);
        }
    }
}

// One thread per (row q, problem).  perm = the problem's rows sorted by label (stable); cluster c = perm[first[c] ..
// first[c + 1]).  phk_cl_silhouette_sums_kernel gives the 16 threads of a query the columns tx, tx + 16, tx + 32, tx + 48
// of each chunk of 64 of the cluster, chunk after chunk -- thread tx adds the members at positions tx, tx + 16, tx + 32,
// ... of the cluster in that order -- and folds the 16 sums by the butterfly xor 1, 2, 4, 8: here one thread keeps the 16
// sums and folds them as that butterfly does.  Then phk_cl_silhouette_finish_kernel's rules.  d is read as d[member][q]
// (= d[q][member] bit for bit): the 64 rows of a wave read 64 neighbouring values.
__global__ __launch_bounds__(256) void sw_silhouette_kernel(const double *__restrict__ dist, uint64_t n, const SwState *__restrict__ st,
                                                           const uint32_t *__restrict__ labels, const uint32_t *__restrict__ perm,
                                                           const uint32_t *__restrict__ first, const uint8_t *__restrict__ want,
                                                           double *__restrict__ out) {
    const uint32_t b = blockIdx.y;
    if (!want[b]) return;
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t qq = q < n ? q : n - 1;
    const uint32_t k = st[b].k;
    const uint32_t *pm = perm + (uint64_t)b * n, *fs = first + st[b].koff + b;   // (k + 1 entries per problem)
    const uint32_t own = labels[(uint64_t)b * n + qq];
    double a_own = 0.0, bb = __builtin_inf();
    uint32_t n_own = 0;
    for (uint32_t c = 0; c < k; ++c) {
        const uint32_t f0 = fs[c], size = fs[c + 1] - f0;
        if (size == 0) continue;
        double a[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = 0.0;
        for (uint32_t p = 0; p < size; p += 16) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (p + j < size) a[j] += dist[(uint64_t)pm[f0 + p + j] * n + qq];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)
#pragma unroll
            for (int j = 0; j < 16; j += 2 * o) a[j] += a[j + o];
        if (c == own) { a_own = a[0]; n_own = size; }
        else bb = fmin(bb, a[0] / (double)size);
    }
    const double aa = a_own / (double)(n_own - 1u);
    const double s = (bb - aa) / fmax(aa, bb);
    if (q < n) out[(uint64_t)b * n + q] = s == s ? s : 0.0;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// np.add.reduce of a contiguous float64 vector: pairwise, in pieces of 8192 (count.hip's phk_np_pairwise_sum on the host)
static double sw_np_pairwise(const double *a, uint64_t n) {
    if (n < 8) {
        double r = 0.0;
        for (uint64_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        uint64_t i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    uint64_t n2 = n / 2;
    n2 -= n2 % 8;
    return sw_np_pairwise(a, n2) + sw_np_pairwise(a + n2, n - n2);
}

static double sw_np_sum(const double *a, uint64_t n) {
    double s = sw_np_pairwise(a, std::min<uint64_t>(n, 8192));
    for (uint64_t o = 8192; o < n; o += 8192) s += sw_np_pairwise(a + o, std::min<uint64_t>(n - o, 8192));
    return s;
}

static void sw_free(phk_sweep *sw) {
    if (sw->d_x) (void)hipFree(sw->d_x);
    if (sw->d_xc) (void)hipFree(sw->d_xc);
    if (sw->ws) (void)hipFree(sw->ws);
    if (sw->d_pair) (void)hipFree(sw->d_pair);
    delete sw;
}

extern "C" int phk_sweep_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_sweep **out) {
    PHK_ENTER(ctx, "phk_sweep_create");
    PHK_REQUIRE(X && out, "phk_sweep_create: NULL pointer");
    PHK_REQUIRE(n >= 1 && D >= 1 && n < (1ull << 31) - 1, "phk_sweep_create: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)D);
    for (uint64_t i = 0; i < n * D; ++i)
        if (!(X[i] - X[i] == 0.0)) {
            phk_set_error("phk_sweep_create: the rows contain NaN or infinity");
            return PHK_ERR_NAN;
        }
    // NumPy's X - X.mean(axis=0) and np.mean(np.var(that, axis=0)): column sums in row order, one division each -- except
    // that a matrix of ONE column is a contiguous vector to NumPy's reduction, which it sums pairwise
    std::vector<double> mean(D, 0.0), xc(n * D), m2(D, 0.0), var(D, 0.0), sq;
    auto column_sums = [&](const double *A, std::vector<double> &out) {
        if (D == 1) {
            out[0] = sw_np_sum(A, n);
            return;
        }
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t d = 0; d < D; ++d) out[d] += A[i * D + d];
    };
    column_sums(X, mean);
    for (uint64_t d = 0; d < D; ++d) mean[d] /= (double)n;
    for (uint64_t i = 0; i < n * D; ++i) xc[i] = X[i] - mean[i % D];
    column_sums(xc.data(), m2);
    for (uint64_t d = 0; d < D; ++d) m2[d] /= (double)n;
    sq.resize(n * D);
    for (uint64_t i = 0; i < n * D; ++i) {
        const double e = xc[i] - m2[i % D];
        sq[i] = e * e;
    }
    column_sums(sq.data(), var);
    for (uint64_t d = 0; d < D; ++d) var[d] /= (double)n;
    phk_sweep *sw = new phk_sweep;
    sw->n = n;
    sw->D = D;
    sw->var_mean = sw_np_sum(var.data(), D) / (double)D;
    const uint64_t bytes = n * D * sizeof(double);
    if (hipMalloc((void **)&sw->d_x, bytes) != hipSuccess || hipMalloc((void **)&sw->d_xc, bytes) != hipSuccess) {
        sw_free(sw);
        phk_set_error("phk_sweep_create: out of device memory (2 x %llu bytes)", (unsigned long long)bytes);
        return PHK_ERR_NOMEM;
    }
    int rc = phk_copy_to_device(ctx, sw->d_x, X, bytes);
    if (rc == PHK_OK) rc = phk_copy_to_device(ctx, sw->d_xc, xc.data(), bytes);
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PHK_ERR_HIP;
    if (rc != PHK_OK) {
        sw_free(sw);
        return rc;
    }
    *out = sw;
    return PHK_OK;
}

extern "C" int phk_sweep_destroy(phk_ctx *ctx, phk_sweep *sw) {
    PHK_ENTER(ctx, "phk_sweep_destroy");
    if (!sw) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    sw_free(sw);
    return PHK_OK;
}

static uint64_t sw_align(uint64_t b) { return (b + 255) & ~255ull; }

extern "C" int phk_sweep_run(phk_ctx *ctx, phk_sweep *sw, uint64_t S, const uint32_t *ks, const uint32_t *first_seed,
                             const double *draws, const uint64_t *draw_off, double tol_rel, int max_iter, uint32_t chunk,
                             int64_t pair_budget, uint32_t *labels, uint32_t *seeds, double *sil, uint32_t *status, int32_t *n_iter,
                             double *min_gap, double *seed_margin) {
    PHK_ENTER(ctx, "phk_sweep_run");
    PHK_REQUIRE(sw, "phk_sweep_run: NULL sweep");
    const uint64_t n = sw->n, D = sw->D;
    PHK_REQUIRE(max_iter >= 1 && tol_rel >= 0.0 && chunk <= 65535, "phk_sweep_run: bad max_iter / tol / chunk");
    if (S == 0) return PHK_OK;
    PHK_REQUIRE(ks && first_seed && draw_off && labels && status && n_iter && min_gap && seed_margin, "phk_sweep_run: NULL pointer");
    for (uint64_t s = 0; s < S; ++s) {
        const uint32_t k = ks[s];
        PHK_REQUIRE(k >= 1 && k <= n, "phk_sweep_run: need 1 <= k <= n (problem %llu: k=%u, n=%llu)", (unsigned long long)s, k,
                    (unsigned long long)n);
        PHK_REQUIRE(!sil || (k >= 2 && (uint64_t)k <= n - 1 && n >= 3),
                    "phk_sweep_run: Number of labels is %u. Valid values are 2 to n_samples - 1 (inclusive)", k);
        PHK_REQUIRE(first_seed[s] < n, "phk_sweep_run: first seed %u of problem %llu is not a row", first_seed[s], (unsigned long long)s);
        const uint32_t T = 2 + (uint32_t)std::log((double)k);
        PHK_REQUIRE(T <= SW_MAX_TRIALS, "phk_sweep_run: k = %u needs %u seeding trials per centre, at most %d are built", k, T,
                    SW_MAX_TRIALS);
        PHK_REQUIRE(draws || k == 1, "phk_sweep_run: NULL draws");
    }
    const uint64_t Sc = std::min<uint64_t>(S, chunk ? chunk : SW_DEFAULT_CHUNK);
    // the largest chunk's centres and draws
    uint64_t ksum_max = 0, dsum_max = 0;
    for (uint64_t s0 = 0; s0 < S; s0 += Sc) {
        uint64_t ksum = 0, dsum = 0;
        for (uint64_t s = s0; s < std::min(S, s0 + Sc); ++s) {
            ksum += ks[s];
            dsum += (uint64_t)(ks[s] - 1) * (2 + (uint32_t)std::log((double)ks[s]));
        }
        ksum_max = std::max(ksum_max, ksum);
        dsum_max = std::max(dsum_max, dsum);
    }
    // the pair distances, once per call, when they fit the budget
    bool stored = false;
    if (sil) {
        uint64_t budget;
        if (pair_budget < 0) {
            size_t free_b = 0, total_b = 0;
            PHK_HIP(hipMemGetInfo(&free_b, &total_b));
            budget = (uint64_t)free_b / 4 + (sw->d_pair ? n * n * 8 : 0);   // (the kept matrix is not "used" memory here)
        } else {
            budget = (uint64_t)pair_budget;
        }
        stored = n * n * 8 <= budget;
        if (stored && !sw->d_pair) {
            if (hipMalloc((void **)&sw->d_pair, n * n * 8) != hipSuccess) {
                sw->d_pair = nullptr;
                (void)hipGetLastError();
                stored = false;   // no room after all: the per-problem pass
            } else {
                const uint64_t tiles = phk_div_up(n, CL_T);
                const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(65535, CL_MAX_BLOCKS / tiles));
                for (uint64_t y0 = 0; y0 < tiles; y0 += step)
                    PHK_LAUNCH(ctx, "sw_pair_kernel",
                               sw_pair_kernel<<<dim3((unsigned)tiles, (unsigned)std::min(step, tiles - y0)), dim3(CL_THREADS), 0,
                                                ctx->stream>>>(sw->d_x, n, D, y0, sw->d_pair));
            }
        }
    }
    // the chunk's workspace
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) { const uint64_t o = off; off += sw_align(bytes); return o; };
    const uint64_t o_cen = take(2 * ksum_max * D * 8), o_lab = take(Sc * n * 4), o_clo = take(Sc * n * 8),
                   o_td = take(Sc * SW_MAX_TRIALS * n * 8), o_cand = take(Sc * SW_MAX_TRIALS * 4), o_seed = take(ksum_max * 4),
                   o_size = take(ksum_max * 4), o_st = take(Sc * sizeof(SwState)), o_draw = take(dsum_max * 8 + 8),
                   o_act = take(256), o_perm = take(sil ? Sc * n * 4 : 0), o_first = take(sil ? (ksum_max + Sc) * 4 : 0),
                   o_want = take(Sc), o_sil = take(sil ? Sc * n * 8 : 0);
    if (sw->ws_bytes < off) {
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        if (sw->ws) (void)hipFree(sw->ws);
        sw->ws = nullptr;
        sw->ws_bytes = 0;
        if (hipMalloc(&sw->ws, off) != hipSuccess) {
            sw->ws = nullptr;
            phk_set_error("phk_sweep_run: out of device memory (%llu bytes for %llu problems at once)", (unsigned long long)off,
                          (unsigned long long)Sc);
            return PHK_ERR_NOMEM;
        }
        sw->ws_bytes = off;
    }
    char *w = (char *)sw->ws;
    SwView v;
    v.Xc = sw->d_xc;
    v.cen = (double *)(w + o_cen);
    v.labels = (uint32_t *)(w + o_lab);
    v.closest = (double *)(w + o_clo);
    v.td = (double *)(w + o_td);
    v.cand = (uint32_t *)(w + o_cand);
    v.seeds = (uint32_t *)(w + o_seed);
    v.sizes = (uint32_t *)(w + o_size);
    v.st = (SwState *)(w + o_st);
    v.draws = (const double *)(w + o_draw);
    v.n = n;
    v.D = D;
    uint32_t *d_act = (uint32_t *)(w + o_act);
    uint32_t *d_perm = (uint32_t *)(w + o_perm), *d_first = (uint32_t *)(w + o_first);
    uint8_t *d_want = (uint8_t *)(w + o_want);
    double *d_sil = (double *)(w + o_sil);

    std::vector<SwState> st(Sc);
    std::vector<uint32_t> cand(Sc * SW_MAX_TRIALS), perm, first;
    std::vector<uint8_t> want(Sc);
    const double tol = sw->var_mean * tol_rel;
    const unsigned seed_blocks = (unsigned)phk_div_up(phk_div_up(n, SW_ROWS_SEED), 4);
    const unsigned assign_blocks = (unsigned)phk_div_up(phk_div_up(n, SW_ROWS_ASSIGN), 4);
    uint64_t seed_out = 0;   // centres of the problems before the chunk
    for (uint64_t s0 = 0; s0 < S; s0 += Sc) {
        const uint64_t nb = std::min(Sc, S - s0);
        const unsigned gb = (unsigned)nb;
        uint32_t kmax = 0, ksum = 0;
        uint64_t dsum = 0;
        std::fill(cand.begin(), cand.end(), 0u);
        for (uint64_t b = 0; b < nb; ++b) {
            SwState &s = st[b];
            memset(&s, 0, sizeof(s));
            s.k = ks[s0 + b];
            s.T = 2 + (uint32_t)std::log((double)s.k);
            s.koff = ksum;
            s.doff = dsum;
            s.active = 1;
            s.seed_margin = INFINITY;
            s.tol = tol;
            const double inf = INFINITY;
            memcpy(&s.gapbits, &inf, 8);
            cand[b * SW_MAX_TRIALS] = first_seed[s0 + b];
            const uint64_t nd = (uint64_t)(s.k - 1) * s.T;
            if (nd)
                PHK_HIP(hipMemcpyAsync(w + o_draw + dsum * 8, draws + draw_off[s0 + b], nd * 8, hipMemcpyHostToDevice, ctx->stream));
            ksum += s.k;
            dsum += nd;
            kmax = std::max(kmax, s.k);
        }
        PHK_HIP(hipMemcpyAsync(v.st, st.data(), nb * sizeof(SwState), hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(v.cand, cand.data(), nb * SW_MAX_TRIALS * 4, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemsetAsync(v.labels, 0xFF, nb * n * 4, ctx->stream));
        // seeding: centre 0 is the caller's row, then up to kmax - 1 greedy steps; a problem with k_s <= step returns at once
        for (uint32_t c = 0; c < kmax; ++c) {
            PHK_LAUNCH(ctx, "sw_seed_dist_kernel", sw_seed_dist_kernel<<<dim3(seed_blocks, gb), dim3(256), 0, ctx->stream>>>(v, c));
            PHK_LAUNCH(ctx, "sw_seed_choose_kernel", sw_seed_choose_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(v, c));
        }
        // Lloyd: one host synchronisation per sweep for the whole chunk (the number of problems still sweeping)
        for (int it = 0; it < max_iter; ++it) {
            PHK_HIP(hipMemsetAsync(d_act, 0, 4, ctx->stream));
            PHK_LAUNCH(ctx, "sw_assign_kernel", sw_assign_kernel<<<dim3(assign_blocks, gb), dim3(256), 0, ctx->stream>>>(v, 0));
            PHK_LAUNCH(ctx, "sw_update_kernel", sw_update_kernel<<<dim3(kmax, gb), dim3(256), 0, ctx->stream>>>(v));
            PHK_LAUNCH(ctx, "sw_stop_kernel", sw_stop_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(v, d_act));
            uint32_t active = 0;
            PHK_HIP(hipMemcpyAsync(&active, d_act, 4, hipMemcpyDeviceToHost, ctx->stream));
            PHK_HIP(hipStreamSynchronize(ctx->stream));
            if (active == 0) break;
        }
        PHK_LAUNCH(ctx, "sw_assign_kernel", sw_assign_kernel<<<dim3(assign_blocks, gb), dim3(256), 0, ctx->stream>>>(v, 1));
        PHK_HIP(hipMemcpyAsync(labels + s0 * n, v.labels, nb * n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (seeds) PHK_HIP(hipMemcpyAsync(seeds + seed_out, v.seeds, (uint64_t)ksum * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipMemcpyAsync(st.data(), v.st, nb * sizeof(SwState), hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        for (uint64_t b = 0; b < nb; ++b) {
            const SwState &s = st[b];
            status[s0 + b] = s.n_empty ? PHK_SWEEP_EMPTY : 0u;
            n_iter[s0 + b] = (int32_t)s.n_iter;
            seed_margin[s0 + b] = s.seed_margin;
            double gap;
            static_assert(sizeof(gap) == sizeof(s.gapbits), "");
            memcpy(&gap, &s.gapbits, 8);
            min_gap[s0 + b] = gap;
        }
        if (sil && stored) {
            // rows sorted by label (stable) and the clusters' first positions, per problem
            perm.assign(nb * n, 0);
            first.assign((uint64_t)ksum + nb, 0);
            for (uint64_t b = 0; b < nb; ++b) {
                const uint32_t k = st[b].k;
                const uint32_t *lab = labels + (s0 + b) * n;
                uint32_t *f = first.data() + st[b].koff + b;
                bool ok = true;
                for (uint64_t i = 0; i < n; ++i) {
                    if (lab[i] >= k) { ok = false; break; }
                    ++f[lab[i] + 1];
                }
                want[b] = ok;
                if (!ok) continue;
                for (uint32_t c = 0; c < k; ++c) f[c + 1] += f[c];
                std::vector<uint32_t> at(f, f + k);
                for (uint64_t i = 0; i < n; ++i) perm[b * n + at[lab[i]]++] = (uint32_t)i;
            }
            PHK_HIP(hipMemcpyAsync(d_perm, perm.data(), nb * n * 4, hipMemcpyHostToDevice, ctx->stream));
            PHK_HIP(hipMemcpyAsync(d_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            PHK_HIP(hipMemcpyAsync(d_want, want.data(), nb, hipMemcpyHostToDevice, ctx->stream));
            PHK_LAUNCH(ctx, "sw_silhouette_kernel",
                       sw_silhouette_kernel<<<dim3((unsigned)phk_div_up(n, 256), gb), dim3(256), 0, ctx->stream>>>(
                           sw->d_pair, n, v.st, v.labels, d_perm, d_first, d_want, d_sil));
            PHK_TRY(phk_copy_to_host(ctx, sil + s0 * n, d_sil, nb * n * 8));
        } else if (sil) {
            for (uint64_t b = 0; b < nb; ++b)
                PHK_TRY(phk_silhouettes_resident(ctx, sw->d_x, n, D, labels + (s0 + b) * n, st[b].k, sil + (s0 + b) * n));
        }
        seed_out += ksum;
    }
    return PHK_OK;
}
