// placement.hip -- batched per-contig k-means placement (scripts/analysis.py:754-792: for every candidate contig, k-means
// on the reference phage rows plus the contig's row, then the silhouettes of the contig's cluster).  gfx950.
//
// The reference rows X[n][D] are resident (phk_placement_create); phk_placement_run solves, for B contig rows Z[B][D], the B
// independent problems "rows 0..n-1 = X, row n = Z[b]" in chunks of problems, every stage one launch for the whole chunk:
//   centring : mean_b = (S + Z[b]) / (n + 1) with S the row-order column sum of X (NumPy's column mean of the appended
//              matrix, bit for bit); the kernels subtract it on the fly, x - mean_b: the very subtraction the host path does;
//   seeding  : scikit-learn's k-means++ with the host's draws (learning.kmeans_plusplus_seeds is the specification): per
//              centre a distance launch (trial candidates to all rows, float64 direct differences) and a choose/search launch
//              (potentials, greedy choice, prefix sum and its search for the next centre's draws).  Only decisions have to
//              equal scikit-learn's; the closest call of either kind is reported as seed_margin;
//   Lloyd    : kmeans.hip's phk_kmeans_lloyd iteration, operation order included, each problem with its own centres, labels,
//              stopping flags and sweep count; a finished problem's workgroups return at once;
//   cluster silhouettes : for the members of the contig's cluster only, sums in an order fixed by the labels alone.
// Everything is float64 and order-deterministic (the only atomics are integer counts and minima), so a problem's result
// does not depend on its place in the batch, on the chunking or on the run.
#include "phk_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#define PL_MAX_TRIALS 10      // 2 + int(ln k): k < 2981
#define PL_ROWS_SEED 4        // rows per wave of the seeding's distance kernel
#define PL_ROWS_ASSIGN 8      // rows per wave of the E-step
#define PL_SIL_GROUPS 16      // workgroups per problem of the silhouette kernel (members are dealt round robin)
#define PL_DEFAULT_CHUNK 256

struct PlState {              // per problem, device
    uint32_t changed;         // labels changed in the running E-step (zeroed by the stopping kernel)
    uint32_t active;          // still sweeping
    uint32_t strict;          // stopped because no label changed (no extra E-step)
    uint32_t n_iter;
    uint32_t n_empty;         // empty clusters met, summed over the sweeps
    uint32_t dup;             // the contig's row equals a reference row
    uint32_t cur;             // which of the two centre buffers holds the current centres
    uint32_t n_members;
    double pot;               // seeding: current potential
    double seed_margin;
    double tol;
    unsigned long long gapbits;
};

struct phk_placement {
    uint64_t n = 0, D = 0;
    double *d_x = nullptr;
    std::vector<double> S, SS;   // column sums of x and x^2 in row order
    void *ws = nullptr;
    uint64_t ws_bytes = 0;
};

__device__ __forceinline__ uint64_t pl_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

__device__ __forceinline__ const double *pl_row(const double *__restrict__ X, const double *__restrict__ z, uint64_t n, uint64_t D,
                                                uint64_t i) {
    return i < n ? X + i * D : z;
}

// per-problem views of the chunk's workspace
struct PlView {
    const double *X;        // [n][D]
    const double *Z;        // [Bc][D]
    double *mean;           // [Bc][D]
    double *cen;            // [Bc][2][k][D]
    uint32_t *labels;       // [Bc][n1]
    double *closest;        // [Bc][n1]
    double *td;             // [Bc][T][n1]
    uint32_t *cand;         // [Bc][PL_MAX_TRIALS]
    uint32_t *seeds;        // [Bc][k]
    uint32_t *sizes;        // [Bc][k]
    PlState *st;            // [Bc]
    uint32_t *members;      // [Bc][n1]
    double *sdist;          // [Bc][PL_SIL_GROUPS][n1]
    double *ssum;           // [Bc][PL_SIL_GROUPS][k]
    uint32_t *ssize;        // [Bc][PL_SIL_GROUPS][k]
    double *sil;            // [Bc][n1]
    uint64_t n, n1, D;
    uint32_t k, T;
};

// ---- set-up: per-problem state, and whether the contig's row equals a reference row ------------------------------------
__global__ __launch_bounds__(256) void pl_init_kernel(PlView v, const double *__restrict__ tol, uint32_t first_seed) {
    const uint32_t b = blockIdx.x;
    PlState *s = v.st + b;
    if (threadIdx.x == 0) {
        s->changed = 0; s->active = 1; s->strict = 0; s->n_iter = 0; s->n_empty = 0; s->dup = 0; s->cur = 0; s->n_members = 0;
        s->pot = 0.0;
        s->seed_margin = INFINITY;
        s->tol = tol[b];
        s->gapbits = (unsigned long long)__double_as_longlong((double)INFINITY);
        v.cand[(uint64_t)b * PL_MAX_TRIALS] = first_seed;
    }
    for (uint64_t i = threadIdx.x; i < v.n1; i += 256) v.labels[(uint64_t)b * v.n1 + i] = 0xFFFFFFFFu;
}

// one wave per (reference row, problem): an exact duplicate of the contig's row
__global__ __launch_bounds__(256) void pl_dup_kernel(PlView v) {
    const int lane = threadIdx.x & 63;
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t b = blockIdx.y;
    if (i >= v.n) return;
    const double *x = v.X + i * v.D, *z = v.Z + (uint64_t)b * v.D;
    bool same = true;
    for (uint64_t d = lane; d < v.D; d += 64) same &= x[d] == z[d];
    if (__all(same) && lane == 0) atomicOr(&v.st[b].dup, 1u);
}

// ---- seeding --------------------------------------------------------------------------------------------------------
// Squared distances of the step's trial candidates to every row, min-ed with the running closest distances (not at the
// first centre).  One wave per PL_ROWS_SEED rows; float64 direct differences of the centred rows, fma in column order.
__global__ __launch_bounds__(256) void pl_seed_dist_kernel(PlView v, uint32_t ntr, int first) {
    const int lane = threadIdx.x & 63;
    const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t b = blockIdx.y;
    const uint64_t i0 = w * PL_ROWS_SEED;
    if (i0 >= v.n1) return;
    const double *z = v.Z + (uint64_t)b * v.D, *mean = v.mean + (uint64_t)b * v.D;
    const double *rows[PL_ROWS_SEED], *cr[PL_MAX_TRIALS];
#pragma unroll
    for (int r = 0; r < PL_ROWS_SEED; ++r) rows[r] = pl_row(v.X, z, v.n, v.D, i0 + r < v.n1 ? i0 + r : v.n1 - 1);
#pragma unroll
    for (int t = 0; t < PL_MAX_TRIALS; ++t) cr[t] = pl_row(v.X, z, v.n, v.D, v.cand[(uint64_t)b * PL_MAX_TRIALS + (t < (int)ntr ? t : 0)]);
    double acc[PL_ROWS_SEED][PL_MAX_TRIALS];
#pragma unroll
    for (int r = 0; r < PL_ROWS_SEED; ++r)
#pragma unroll
        for (int t = 0; t < PL_MAX_TRIALS; ++t) acc[r][t] = 0.0;
    for (uint64_t d = lane; d < v.D; d += 64) {
        const double m = mean[d];
        double x[PL_ROWS_SEED];
#pragma unroll
        for (int r = 0; r < PL_ROWS_SEED; ++r) x[r] = rows[r][d] - m;
#pragma unroll
        for (int t = 0; t < PL_MAX_TRIALS; ++t)
            if (t < (int)ntr) {
                const double c = cr[t][d] - m;
#pragma unroll
                for (int r = 0; r < PL_ROWS_SEED; ++r) {
                    const double e = x[r] - c;
                    acc[r][t] = fma(e, e, acc[r][t]);
                }
            }
    }
#pragma unroll
    for (int t = 0; t < PL_MAX_TRIALS; ++t)
        if (t < (int)ntr) {
#pragma unroll
            for (int r = 0; r < PL_ROWS_SEED; ++r) {
                double a = acc[r][t];
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s);
                const uint64_t i = i0 + r;
                if (lane == 0 && i < v.n1) {
                    const double old = v.closest[(uint64_t)b * v.n1 + i];
                    v.td[((uint64_t)b * v.T + t) * v.n1 + i] = first ? a : fmin(old, a);
                }
            }
        }
}

// One workgroup per problem.  Centre `step`: the potentials of its trials (slice sums of 256 contiguous slices in index
// order, then the 256 partials in order), the greedy choice (first smallest), the gap to the best trial on ANOTHER row; the
// chosen row becomes centre `step`.  Then, for centre step + 1: the prefix sum of the closest distances in the same order
// and, per draw u, the first row whose prefix reaches u * potential (np.searchsorted(np.cumsum(closest), u * pot)), with
// the draw's distance to the two prefix values around it.  draws = the T uniforms of centre step + 1 (NULL at the end).
__global__ __launch_bounds__(256) void pl_seed_choose_kernel(PlView v, uint32_t step, uint32_t ntr, const double *__restrict__ draws) {
    __shared__ double part[PL_MAX_TRIALS][256];
    __shared__ double pots[PL_MAX_TRIALS];
    __shared__ double pre[257];
    __shared__ uint32_t s_best, s_cand[PL_MAX_TRIALS], s_claim[PL_MAX_TRIALS];
    __shared__ unsigned long long s_mbits[PL_MAX_TRIALS];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    PlState *st = v.st + b;
    const uint64_t n1 = v.n1;
    const uint64_t per = (n1 + 255) / 256, lo = pl_min(per * t, n1), hi = pl_min(lo + per, n1);
    const double *td = v.td + (uint64_t)b * v.T * n1;
    uint32_t *cand = v.cand + (uint64_t)b * PL_MAX_TRIALS;
    for (uint32_t tr = 0; tr < ntr; ++tr) {
        double s = 0.0;
        for (uint64_t i = lo; i < hi; ++i) s += td[tr * n1 + i];
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
        if (!(pots[best] > 0.0) && step + 1 < v.k) margin = 0.0;   // nothing left to draw from: every row is a centre already
        st->seed_margin = margin;
        st->pot = pots[best];
        v.seeds[(uint64_t)b * v.k + step] = cand[best];
        s_best = best;
    }
    __syncthreads();
    const uint32_t best = s_best;
    {   // centre `step` = the centred chosen row; the running closest distances = the chosen trial's
        const double *src = pl_row(v.X, v.Z + (uint64_t)b * v.D, v.n, v.D, cand[best]);
        const double *mean = v.mean + (uint64_t)b * v.D;
        double *cen = v.cen + ((uint64_t)b * 2 * v.k + step) * v.D;
        for (uint64_t d = t; d < v.D; d += 256) cen[d] = src[d] - mean[d];
        double *closest = v.closest + (uint64_t)b * n1;
        for (uint64_t i = lo; i < hi; ++i) closest[i] = td[best * n1 + i];
    }
    if (draws == nullptr) return;
    if (t == 0) {
        double run = 0.0;
        for (int j = 0; j < 256; ++j) { pre[j] = run; run += part[best][j]; }
        pre[256] = run;
    }
    if (t < PL_MAX_TRIALS) {
        s_cand[t] = 0xFFFFFFFFu;
        s_claim[t] = 0;
        s_mbits[t] = (unsigned long long)__double_as_longlong((double)INFINITY);
    }
    __syncthreads();
    const double pot = pots[best];
    for (uint32_t tr = 0; tr < v.T; ++tr) {
        const double val = draws[tr] * pot;
        double run = pre[t];
        if (run < val) {
            for (uint64_t i = lo; i < hi; ++i) {
                const double prev = run;
                run += td[best * n1 + i];
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
        for (uint32_t tr = 0; tr < v.T; ++tr) {
            // exactly one slice holds the first row that reaches the draw; none or two (the slices' own roundings) is a draw
            // within rounding of a prefix value, and so is a draw past the total: margin 0
            const double m = s_claim[tr] == 1 ? __longlong_as_double((long long)s_mbits[tr]) : 0.0;
            margin = m == m ? fmin(margin, m) : 0.0;
            cand[tr] = s_cand[tr] < n1 ? s_cand[tr] : (uint32_t)(n1 - 1);
        }
        st->seed_margin = margin;
    }
}

// ---- Lloyd ----------------------------------------------------------------------------------------------------------
// km_assign_kernel (kmeans.hip) for a chunk of problems: the same per-point arithmetic -- lane l sums columns l, l + 64, ...
// of (x - mean) - centre by fma, the butterfly, the strict comparison that keeps the lower centre index -- with
// PL_ROWS_ASSIGN rows per wave sharing each centre value they load.  final = 1: the extra E-step of the problems that
// stopped on the centre shift.
__global__ __launch_bounds__(256) void pl_assign_kernel(PlView v, int final) {
    const uint32_t b = blockIdx.y;
    PlState *st = v.st + b;
    if (final ? (st->strict != 0) : (st->active == 0)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t i0 = w * PL_ROWS_ASSIGN;
    if (i0 >= v.n1) return;
    const double *z = v.Z + (uint64_t)b * v.D, *mean = v.mean + (uint64_t)b * v.D;
    const double *cen = v.cen + ((uint64_t)b * 2 + st->cur) * v.k * v.D;
    const double *rows[PL_ROWS_ASSIGN];
#pragma unroll
    for (int r = 0; r < PL_ROWS_ASSIGN; ++r) rows[r] = pl_row(v.X, z, v.n, v.D, i0 + r < v.n1 ? i0 + r : v.n1 - 1);
    double best[PL_ROWS_ASSIGN], second[PL_ROWS_ASSIGN];
    uint32_t bi[PL_ROWS_ASSIGN];
#pragma unroll
    for (int r = 0; r < PL_ROWS_ASSIGN; ++r) { best[r] = INFINITY; second[r] = INFINITY; bi[r] = 0; }
    for (uint32_t c = 0; c < v.k; ++c) {
        double acc[PL_ROWS_ASSIGN];
#pragma unroll
        for (int r = 0; r < PL_ROWS_ASSIGN; ++r) acc[r] = 0.0;
        const double *cc = cen + (uint64_t)c * v.D;
        for (uint64_t d = lane; d < v.D; d += 64) {
            const double m = mean[d], cv = cc[d];
#pragma unroll
            for (int r = 0; r < PL_ROWS_ASSIGN; ++r) {
                const double e = (rows[r][d] - m) - cv;
                acc[r] = fma(e, e, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < PL_ROWS_ASSIGN; ++r) {
            double a = acc[r];
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s);
            if (a < best[r]) { second[r] = best[r]; best[r] = a; bi[r] = c; }
            else if (a < second[r]) second[r] = a;
        }
    }
    if (lane == 0) {
        uint32_t *labels = v.labels + (uint64_t)b * v.n1;
#pragma unroll
        for (int r = 0; r < PL_ROWS_ASSIGN; ++r) {
            const uint64_t i = i0 + r;
            if (i >= v.n1) continue;
            if (labels[i] != bi[r]) atomicAdd(&st->changed, 1u);
            labels[i] = bi[r];
            if (v.k > 1 && second[r] > 0.0 && second[r] < INFINITY)
                atomicMin(&st->gapbits, (unsigned long long)__double_as_longlong((second[r] - best[r]) / second[r]));
        }
    }
}

// km_update_kernel for a chunk: new centre = mean of the members' centred rows in index order, written to the other
// centre buffer (an empty cluster keeps its centre); one workgroup per (centre, problem)
__global__ __launch_bounds__(256) void pl_update_kernel(PlView v) {
    const uint32_t c = blockIdx.x, b = blockIdx.y;
    PlState *st = v.st + b;
    if (st->active == 0) return;
    const double *z = v.Z + (uint64_t)b * v.D, *mean = v.mean + (uint64_t)b * v.D;
    const double *old = v.cen + (((uint64_t)b * 2 + st->cur) * v.k + c) * v.D;
    double *cen = v.cen + (((uint64_t)b * 2 + (st->cur ^ 1u)) * v.k + c) * v.D;
    const uint32_t *labels = v.labels + (uint64_t)b * v.n1;
    uint32_t cnt = 0;
    for (uint64_t d = threadIdx.x; d < v.D; d += 256) {
        const double mu = mean[d];
        double s = 0.0;
        uint32_t m = 0;
        for (uint64_t i = 0; i < v.n1; ++i)
            if (labels[i] == c) { s += pl_row(v.X, z, v.n, v.D, i)[d] - mu; ++m; }
        cen[d] = m ? s / (double)m : old[d];
        cnt = m;
    }
    if (threadIdx.x == 0) v.sizes[(uint64_t)b * v.k + c] = cnt;
}

// km_shift_kernel + the host's stopping rule, per problem: total squared centre shift (same summation order), empty
// clusters, then "no label changed" (strict) or "shift <= tol" (one more E-step).  The new centres become current.
__global__ __launch_bounds__(256) void pl_stop_kernel(PlView v, uint32_t *__restrict__ n_active) {
    __shared__ double part[256];
    const uint32_t b = blockIdx.x;
    PlState *st = v.st + b;
    if (st->active == 0) return;
    const uint64_t count = (uint64_t)v.k * v.D;
    const double *old = v.cen + ((uint64_t)b * 2 + st->cur) * count, *cen = v.cen + ((uint64_t)b * 2 + (st->cur ^ 1u)) * count;
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
        for (uint32_t c = 0; c < v.k; ++c) e += v.sizes[(uint64_t)b * v.k + c] == 0 ? 1u : 0u;
        st->n_empty += e;
        st->n_iter += 1;
        st->cur ^= 1u;
        if (st->changed == 0) { st->strict = 1; st->active = 0; }
        else if (shift <= st->tol) st->active = 0;
        st->changed = 0;
        if (st->active) atomicAdd(n_active, 1u);
    }
}

// ---- cluster silhouettes --------------------------------------------------------------------------------------------
// the members of the contig's cluster in row order (the contig, row n, comes last): one workgroup per problem
__global__ __launch_bounds__(256) void pl_members_kernel(PlView v) {
    __shared__ uint32_t cnt[256];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t *labels = v.labels + (uint64_t)b * v.n1;
    const uint32_t own = labels[v.n];
    const uint64_t per = (v.n1 + 255) / 256, lo = pl_min(per * t, v.n1), hi = pl_min(lo + per, v.n1);
    uint32_t m = 0;
    for (uint64_t i = lo; i < hi; ++i) m += labels[i] == own ? 1u : 0u;
    cnt[t] = m;
    __syncthreads();
    uint32_t at = 0;
    for (int j = 0; j < t; ++j) at += cnt[j];
    uint32_t *members = v.members + (uint64_t)b * v.n1;
    for (uint64_t i = lo; i < hi; ++i)
        if (labels[i] == own) members[at++] = (uint32_t)i;
    if (t == 255) v.st[b].n_members = at;
}

// Workgroup (g, problem) takes members g, g + PL_SIL_GROUPS, ...: distances of the member to all rows (one wave per row,
// direct differences of the rows as given), then per cluster the sum over its rows in row order (one thread per cluster),
// then scikit-learn's silhouette_samples: a = sum_own / (n_own - 1), b = min over the other non-empty clusters of
// sum_c / n_c, (b - a) / max(a, b), NaN (a singleton) -> 0.
__global__ __launch_bounds__(256) void pl_silhouette_kernel(PlView v) {
    const uint32_t g = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nm = v.st[b].n_members;
    const uint32_t *labels = v.labels + (uint64_t)b * v.n1;
    const uint32_t *members = v.members + (uint64_t)b * v.n1;
    const uint32_t own = labels[v.n];
    const double *z = v.Z + (uint64_t)b * v.D;
    double *dist = v.sdist + ((uint64_t)b * PL_SIL_GROUPS + g) * v.n1;
    double *csum = v.ssum + ((uint64_t)b * PL_SIL_GROUPS + g) * v.k;
    uint32_t *csize = v.ssize + ((uint64_t)b * PL_SIL_GROUPS + g) * v.k;
    for (uint32_t q = g; q < nm; q += PL_SIL_GROUPS) {
        const double *xq = pl_row(v.X, z, v.n, v.D, members[q]);
        for (uint64_t j = wave; j < v.n1; j += 4) {
            const double *xj = pl_row(v.X, z, v.n, v.D, j);
            double acc = 0.0;
            for (uint64_t d = lane; d < v.D; d += 64) {
                const double e = xq[d] - xj[d];
                acc = fma(e, e, acc);
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
            if (lane == 0) dist[j] = sqrt(acc);
        }
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < v.k; c += 256) {
            double s = 0.0;
            uint32_t m = 0;
            for (uint64_t j = 0; j < v.n1; ++j)
                if (labels[j] == c) { s += dist[j]; ++m; }
            csum[c] = s;
            csize[c] = m;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double a = csum[own] / (double)(csize[own] - 1u);
            double bb = __builtin_inf();
            for (uint32_t c = 0; c < v.k; ++c)
                if (c != own && csize[c]) bb = fmin(bb, csum[c] / (double)csize[c]);
            const double s = (bb - a) / fmax(a, bb);
            v.sil[(uint64_t)b * v.n1 + q] = s == s ? s : 0.0;
        }
        __syncthreads();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
extern "C" int phk_placement_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_placement **out) {
    PHK_ENTER(ctx, "phk_placement_create");
    PHK_REQUIRE(X && out, "phk_placement_create: NULL pointer");
    PHK_REQUIRE(n >= 1 && D >= 1 && n < (1ull << 31) - 1, "phk_placement_create: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)D);
    for (uint64_t i = 0; i < n * D; ++i)
        if (!(X[i] - X[i] == 0.0)) {
            phk_set_error("phk_placement_create: the reference rows contain NaN or infinity");
            return PHK_ERR_NAN;
        }
    phk_placement *pl = new phk_placement;
    pl->n = n;
    pl->D = D;
    pl->S.assign(D, 0.0);
    pl->SS.assign(D, 0.0);
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t d = 0; d < D; ++d) {
            const double x = X[i * D + d];
            pl->S[d] += x;             // row order: NumPy's add.reduce over axis 0 of a C-contiguous matrix
            pl->SS[d] += x * x;
        }
    if (hipMalloc((void **)&pl->d_x, n * D * sizeof(double)) != hipSuccess) {
        delete pl;
        phk_set_error("phk_placement_create: out of device memory (%llu bytes)", (unsigned long long)(n * D * sizeof(double)));
        return PHK_ERR_NOMEM;
    }
    int rc = phk_copy_to_device(ctx, pl->d_x, X, n * D * sizeof(double));
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PHK_ERR_HIP;
    if (rc != PHK_OK) {
        (void)hipFree(pl->d_x);
        delete pl;
        return rc;
    }
    *out = pl;
    return PHK_OK;
}

extern "C" int phk_placement_destroy(phk_ctx *ctx, phk_placement *pl) {
    PHK_ENTER(ctx, "phk_placement_destroy");
    if (!pl) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (pl->d_x) (void)hipFree(pl->d_x);
    if (pl->ws) (void)hipFree(pl->ws);
    delete pl;
    return PHK_OK;
}

static uint64_t pl_align(uint64_t b) { return (b + 255) & ~255ull; }

extern "C" int phk_placement_run(phk_ctx *ctx, phk_placement *pl, const double *Z, uint64_t B, uint32_t k, uint32_t first_seed,
                                 const double *draws, double tol_rel, int max_iter, uint32_t chunk, uint32_t *labels,
                                 uint32_t *seeds, double *sil, uint32_t *n_members, uint32_t *status, int32_t *n_iter,
                                 double *min_gap, double *seed_margin) {
    PHK_ENTER(ctx, "phk_placement_run");
    PHK_REQUIRE(pl, "phk_placement_run: NULL placement");
    const uint64_t n = pl->n, D = pl->D, n1 = n + 1;
    PHK_REQUIRE(k >= 1 && k <= n1, "phk_placement_run: need 1 <= k <= n + 1 (k=%u, n=%llu)", k, (unsigned long long)n);
    const uint32_t T = 2 + (uint32_t)std::log((double)k);
    PHK_REQUIRE(T <= PL_MAX_TRIALS, "phk_placement_run: k = %u needs %u seeding trials per centre, at most %d are built", k, T,
                PL_MAX_TRIALS);
    PHK_REQUIRE(max_iter >= 1 && tol_rel >= 0.0 && first_seed < n1 && chunk <= 65535, "phk_placement_run: bad max_iter / tol / first seed / chunk");
    if (B == 0) return PHK_OK;
    PHK_REQUIRE(Z && labels && sil && n_members && status && n_iter && min_gap && seed_margin && (draws || k == 1),
                "phk_placement_run: NULL pointer");
    for (uint64_t i = 0; i < B * D; ++i)
        if (!(Z[i] - Z[i] == 0.0)) {
            phk_set_error("phk_placement_run: the contig rows contain NaN or infinity");
            return PHK_ERR_NAN;
        }
    const uint64_t Bc = std::min<uint64_t>(B, chunk ? chunk : PL_DEFAULT_CHUNK);
    // the chunk's workspace
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) { const uint64_t o = off; off += pl_align(bytes); return o; };
    const uint64_t o_z = take(Bc * D * 8), o_mean = take(Bc * D * 8), o_tol = take(Bc * 8), o_cen = take(Bc * 2 * k * D * 8),
                   o_lab = take(Bc * n1 * 4), o_clo = take(Bc * n1 * 8), o_td = take(Bc * T * n1 * 8),
                   o_cand = take(Bc * PL_MAX_TRIALS * 4), o_seed = take(Bc * k * 4), o_size = take(Bc * k * 4),
                   o_st = take(Bc * sizeof(PlState)), o_mem = take(Bc * n1 * 4), o_sd = take(Bc * PL_SIL_GROUPS * n1 * 8),
                   o_ss = take(Bc * PL_SIL_GROUPS * (uint64_t)k * 8), o_sc = take(Bc * PL_SIL_GROUPS * (uint64_t)k * 4), o_sil = take(Bc * n1 * 8), o_draw = take((uint64_t)k * T * 8),
                   o_act = take(256);
    if (pl->ws_bytes < off) {
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        if (pl->ws) (void)hipFree(pl->ws);
        pl->ws = nullptr;
        pl->ws_bytes = 0;
        if (hipMalloc(&pl->ws, off) != hipSuccess) {
            pl->ws = nullptr;
            phk_set_error("phk_placement_run: out of device memory (%llu bytes for %llu problems at once)", (unsigned long long)off,
                          (unsigned long long)Bc);
            return PHK_ERR_NOMEM;
        }
        pl->ws_bytes = off;
    }
    char *w = (char *)pl->ws;
    PlView v;
    v.X = pl->d_x;
    v.Z = (const double *)(w + o_z);
    v.mean = (double *)(w + o_mean);
    v.cen = (double *)(w + o_cen);
    v.labels = (uint32_t *)(w + o_lab);
    v.closest = (double *)(w + o_clo);
    v.td = (double *)(w + o_td);
    v.cand = (uint32_t *)(w + o_cand);
    v.seeds = (uint32_t *)(w + o_seed);
    v.sizes = (uint32_t *)(w + o_size);
    v.st = (PlState *)(w + o_st);
    v.members = (uint32_t *)(w + o_mem);
    v.sdist = (double *)(w + o_sd);
    v.ssum = (double *)(w + o_ss);
    v.ssize = (uint32_t *)(w + o_sc);
    v.sil = (double *)(w + o_sil);
    v.n = n; v.n1 = n1; v.D = D; v.k = k; v.T = T;
    double *d_tol = (double *)(w + o_tol), *d_draws = (double *)(w + o_draw);
    uint32_t *d_act = (uint32_t *)(w + o_act);
    if (k > 1) PHK_HIP(hipMemcpyAsync(d_draws, draws, (uint64_t)(k - 1) * T * 8, hipMemcpyHostToDevice, ctx->stream));

    std::vector<double> mean(Bc * D), tol(Bc);
    std::vector<PlState> st(Bc);
    const unsigned seed_blocks = (unsigned)phk_div_up(phk_div_up(n1, PL_ROWS_SEED), 4);
    const unsigned assign_blocks = (unsigned)phk_div_up(phk_div_up(n1, PL_ROWS_ASSIGN), 4);
    for (uint64_t b0 = 0; b0 < B; b0 += Bc) {
        const uint64_t nb = std::min(Bc, B - b0);
        const unsigned gb = (unsigned)nb;
        // centring and the stopping tolerance: mean = (S + z) / (n + 1); tol = tol_rel * mean over the columns of the
        // column variances of the appended matrix (np.mean(np.var(X, axis=0)) * tol in the single-problem path)
        for (uint64_t b = 0; b < nb; ++b) {
            const double *z = Z + (b0 + b) * D;
            double vs = 0.0;
            for (uint64_t d = 0; d < D; ++d) {
                const double m = (pl->S[d] + z[d]) / (double)n1;
                mean[b * D + d] = m;
                const double var = (pl->SS[d] + z[d] * z[d]) / (double)n1 - m * m;
                vs += var > 0.0 ? var : 0.0;
            }
            tol[b] = vs / (double)D * tol_rel;
        }
        PHK_HIP(hipMemcpyAsync(w + o_z, Z + b0 * D, nb * D * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(w + o_mean, mean.data(), nb * D * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(d_tol, tol.data(), nb * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_LAUNCH(ctx, "pl_init_kernel", pl_init_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(v, d_tol, first_seed));
        PHK_LAUNCH(ctx, "pl_dup_kernel",
                   pl_dup_kernel<<<dim3((unsigned)phk_div_up(n, 4), gb), dim3(256), 0, ctx->stream>>>(v));
        // seeding: centre 0 is the host's draw (the same row for every problem), then k - 1 greedy steps
        for (uint32_t c = 0; c < k; ++c) {
            const uint32_t ntr = c == 0 ? 1 : T;
            PHK_LAUNCH(ctx, "pl_seed_dist_kernel",
                       pl_seed_dist_kernel<<<dim3(seed_blocks, gb), dim3(256), 0, ctx->stream>>>(v, ntr, c == 0 ? 1 : 0));
            PHK_LAUNCH(ctx, "pl_seed_choose_kernel",
                       pl_seed_choose_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(
                           v, c, ntr, c + 1 < k ? (const double *)(d_draws + (uint64_t)c * T) : (const double *)nullptr));
        }
        // Lloyd: one host synchronisation per sweep for the whole chunk (the number of problems still sweeping)
        for (int it = 0; it < max_iter; ++it) {
            PHK_HIP(hipMemsetAsync(d_act, 0, 4, ctx->stream));
            PHK_LAUNCH(ctx, "pl_assign_kernel", pl_assign_kernel<<<dim3(assign_blocks, gb), dim3(256), 0, ctx->stream>>>(v, 0));
            PHK_LAUNCH(ctx, "pl_update_kernel", pl_update_kernel<<<dim3(k, gb), dim3(256), 0, ctx->stream>>>(v));
            PHK_LAUNCH(ctx, "pl_stop_kernel", pl_stop_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(v, d_act));
            uint32_t active = 0;
            PHK_HIP(hipMemcpyAsync(&active, d_act, 4, hipMemcpyDeviceToHost, ctx->stream));
            PHK_HIP(hipStreamSynchronize(ctx->stream));
            if (active == 0) break;
        }
        PHK_LAUNCH(ctx, "pl_assign_kernel", pl_assign_kernel<<<dim3(assign_blocks, gb), dim3(256), 0, ctx->stream>>>(v, 1));
        PHK_LAUNCH(ctx, "pl_members_kernel", pl_members_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(v));
        PHK_LAUNCH(ctx, "pl_silhouette_kernel",
                   pl_silhouette_kernel<<<dim3(PL_SIL_GROUPS, gb), dim3(256), 0, ctx->stream>>>(v));
        PHK_HIP(hipMemcpyAsync(labels + b0 * n1, v.labels, nb * n1 * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipMemcpyAsync(sil + b0 * n1, v.sil, nb * n1 * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (seeds) PHK_HIP(hipMemcpyAsync(seeds + b0 * k, v.seeds, nb * k * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipMemcpyAsync(st.data(), v.st, nb * sizeof(PlState), hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        for (uint64_t b = 0; b < nb; ++b) {
            const PlState &s = st[b];
            status[b0 + b] = (s.dup ? PHK_PLACEMENT_DUPLICATE : 0u) | (s.n_empty ? PHK_PLACEMENT_EMPTY : 0u);
            n_iter[b0 + b] = (int32_t)s.n_iter;
            n_members[b0 + b] = s.n_members;
            seed_margin[b0 + b] = s.seed_margin;
            double gap;
            static_assert(sizeof(gap) == sizeof(s.gapbits), "");
            memcpy(&gap, &s.gapbits, 8);
            min_gap[b0 + b] = gap;
        }
    }
    return PHK_OK;
}
