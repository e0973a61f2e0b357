// kmeans_batch.h -- the batched k-means core of placement.hip, sweep.hip (4.11) and combo_grid.hip (4.18): a chunk of independent
// k-means problems, every stage one launch for the whole chunk, the grid's second dimension (or its only one) the problem.
//   seeding : scikit-learn's k-means++ with the caller's draws (learning.kmeans_plusplus_seeds is the specification): per
//             centre a distance launch (trial candidates to all rows, float64 direct differences) and a choose/search launch
//             (potentials, greedy choice, prefix sum and its search for the next centre's draws).  Only decisions have to
//             equal scikit-learn's; the closest call of either kind is reported as seed_margin.  A problem
//             whose k centres are chosen returns at once: a chunk costs 2 max k launches, not 2 sum k;
//   Lloyd   : kmeans.hip's phk_kmeans_lloyd iteration, operation order included (labels, sweep counts and min_gap equal the
//             single-problem path's bit for bit), each problem with its own centres, labels, stopping flags and sweep count;
//             the host reads one word per sweep for the chunk, a finished problem's workgroups return at once.
// Where a problem's rows come from is a compile-time parameter of the kernels (KbCentredRows, KbAppendedRows, KbFoldRows below); each
// client instantiates them for its own source.
// The host half, below the kernels, is shared as well: the trial and draw counts (kb_trials, kb_draws), the refusals of a call
// and of a problem (kb_check_call, kb_check_problem), the largest chunk of a call (kb_extent), the one statement of the chunk's
// workspace (KbSpace: the core's ten regions out of the client's PhkLayout, bound to a KbView after the allocation), the
// chunk's way in and out (KbChunk: add a problem with its draws, upload, download, the per-problem results) and
// kb_solve_chunk.  A client is its own checks, its own regions and a loop over chunks around those calls.
// Everything is float64 and order-deterministic (the only atomics are integer
// counts and minima); every sum's order is fixed by the rows, the labels and the problem alone, so a problem's result does
// not depend on its place in the chunk, on the chunking or on the run.
#pragma once
#include "phk_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#define KB_MAX_TRIALS 10      // 2 + int(ln k): k < 2981
#define KB_ROWS_SEED 4        // rows per wave of the seeding's distance kernel
#define KB_ROWS_ASSIGN 8      // rows per wave of the E-step

struct KbState {              // per problem, device
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

struct KbView {               // the chunk's workspace; Bc = problems of a chunk
    double *cen;              // per problem [2][k][D] at 2 * koff * D
    uint32_t *labels;         // [Bc][n]
    double *closest;          // [Bc][n]
    double *td;               // [Bc][trials][n]
    uint32_t *cand;           // [Bc][KB_MAX_TRIALS]
    uint32_t *seeds;          // per problem [k] at koff
    uint32_t *sizes;          // per problem [k] at koff
    KbState *st;              // [Bc]
    const double *draws;      // the chunk's draws; problem b's T uniforms of centre step + 1 at doff + step * T
    uint64_t n, D;            // rows per problem, columns
    uint32_t trials;          // trial stride of td: >= every problem's T
};

// ---- row sources: row(b, i, D) = row i of problem b as stored, shift(b, d, D) = what the problem subtracts from column d
// (loaded once per column), value(x, shift) = the value the k-means runs on ------------------------------------------------
struct KbCentredRows {        // resident rows, centred beforehand, the same for every problem
    const double *X;          // [n][D]
    __device__ __forceinline__ const double *row(uint32_t, uint64_t i, uint64_t D) const { return X + i * D; }
    __device__ __forceinline__ double shift(uint32_t, uint64_t, uint64_t) const { return 0.0; }
    __device__ static __forceinline__ double value(double x, double) { return x; }
};

struct KbAppendedRows {       // nX resident reference rows plus problem b's own row Z[b], centred on the fly by mean[b]
    const double *X;          // [nX][D]
    const double *Z;          // [Bc][D]
    const double *mean;       // [Bc][D]
    uint64_t nX;
    __device__ __forceinline__ const double *row(uint32_t b, uint64_t i, uint64_t D) const { return i < nX ? X + i * D : Z + (uint64_t)b * D; }
    __device__ __forceinline__ double shift(uint32_t b, uint64_t d, uint64_t D) const { return mean[(uint64_t)b * D + d]; }
    __device__ static __forceinline__ double value(double x, double m) { return x - m; }
};

struct KbFoldRows {           // problem b's row i is the resident row X[idx[ioff[b] + i]] (a fold's train rows), centred on the fly
    const double *X;          // [M][D]
    const int32_t *idx;       // the row lists of the train sets, one after the other
    const uint64_t *ioff;     // [Bc] where problem b's list starts in idx
    const double *mean;       // the train sets' column means, one after the other
    const uint64_t *moff;     // [Bc] where problem b's mean starts
    __device__ __forceinline__ const double *row(uint32_t b, uint64_t i, uint64_t D) const { return X + (uint64_t)idx[ioff[b] + i] * D; }
    __device__ __forceinline__ double shift(uint32_t b, uint64_t d, uint64_t) const { return mean[moff[b] + d]; }
    __device__ static __forceinline__ double value(double x, double m) { return x - m; }
};

__device__ __forceinline__ uint64_t kb_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- seeding --------------------------------------------------------------------------------------------------------
// Squared distances of the step's trial rows to every row, min-ed with the running closest distances (not at the first
// centre).  One wave per KB_ROWS_SEED rows; float64 direct differences of the centred rows, fma in column order.
template <class Rows>
__global__ __launch_bounds__(256) void kb_seed_dist_kernel(KbView v, Rows src, uint32_t step) {
    const uint32_t b = blockIdx.y;
    const KbState *st = v.st + b;
    // the step's trials: none once the problem's k centres are chosen, one for the caller's first centre.  (k and T are
    // read together, ahead of the branch: one scalar load in the chain kernel arguments -> state -> candidates -> rows.)
    const uint32_t k = st->k, T = st->T;
    const uint32_t ntr = step >= k ? 0u : step == 0 ? 1u : T;
    if (ntr == 0) return;
    const int lane = threadIdx.x & 63;
    const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t i0 = w * KB_ROWS_SEED;
    if (i0 >= v.n) return;
    const double *rows[KB_ROWS_SEED], *cr[KB_MAX_TRIALS];
#pragma unroll
    for (int r = 0; r < KB_ROWS_SEED; ++r) rows[r] = src.row(b, kb_min(i0 + r, v.n - 1), v.D);
#pragma unroll
    for (int t = 0; t < KB_MAX_TRIALS; ++t)   // (every candidate is a row: the host checks the first, the choose kernel clamps the rest)
        cr[t] = src.row(b, v.cand[(uint64_t)b * KB_MAX_TRIALS + (t < (int)ntr ? t : 0)], v.D);
    double acc[KB_ROWS_SEED][KB_MAX_TRIALS];
#pragma unroll
    for (int r = 0; r < KB_ROWS_SEED; ++r)
#pragma unroll
        for (int t = 0; t < KB_MAX_TRIALS; ++t) acc[r][t] = 0.0;
    for (uint64_t d = lane; d < v.D; d += 64) {
        const double m = src.shift(b, d, v.D);
        double x[KB_ROWS_SEED];
#pragma unroll
        for (int r = 0; r < KB_ROWS_SEED; ++r) x[r] = Rows::value(rows[r][d], m);
#pragma unroll
        for (int t = 0; t < KB_MAX_TRIALS; ++t)
            if (t < (int)ntr) {
                const double c = Rows::value(cr[t][d], m);
#pragma unroll
                for (int r = 0; r < KB_ROWS_SEED; ++r) {
                    const double e = x[r] - c;
                    acc[r][t] = fma(e, e, acc[r][t]);
                }
            }
    }
#pragma unroll
    for (int t = 0; t < KB_MAX_TRIALS; ++t)
        if (t < (int)ntr) {
#pragma unroll
            for (int r = 0; r < KB_ROWS_SEED; ++r) {
                double a = acc[r][t];
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s);
                const uint64_t i = i0 + r;
                if (lane == 0 && i < v.n) {
                    const double old = v.closest[(uint64_t)b * v.n + i];
                    v.td[((uint64_t)b * v.trials + t) * v.n + i] = step == 0 ? a : fmin(old, a);
                }
            }
        }
}

// One workgroup per problem.  Centre `step`: the potentials of its trials (slice sums of 256 contiguous slices in index
// order, then the 256 partials in order), the greedy choice (first smallest), the gap to the best trial on ANOTHER row; the
// chosen row becomes centre `step`.  Then, for centre step + 1: the prefix sum of the closest distances in the same order
// and, per draw u, the first row whose prefix reaches u * potential (np.searchsorted(np.cumsum(closest), u * pot)), with
// the draw's distance to the two prefix values around it.
template <class Rows>
__global__ __launch_bounds__(256) void kb_seed_choose_kernel(KbView v, Rows src, uint32_t step) {
    __shared__ double part[KB_MAX_TRIALS][256];
    __shared__ double pots[KB_MAX_TRIALS];
    __shared__ double pre[257];
    __shared__ uint32_t s_best, s_cand[KB_MAX_TRIALS], s_claim[KB_MAX_TRIALS];
    __shared__ unsigned long long s_mbits[KB_MAX_TRIALS];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    KbState *st = v.st + b;
    const uint32_t k = st->k, T = st->T;
    if (step >= k) return;
    const uint32_t ntr = step == 0 ? 1u : T;
    const double *draws = step + 1 < k ? v.draws + st->doff + (uint64_t)step * T : nullptr;
    const uint64_t n = v.n;
    const uint64_t per = (n + 255) / 256, lo = kb_min(per * t, n), hi = kb_min(lo + per, n);
    const double *td = v.td + (uint64_t)b * v.trials * n;
    uint32_t *cand = v.cand + (uint64_t)b * KB_MAX_TRIALS;
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
    {   // centre `step` = the chosen row's values; the running closest distances = the chosen trial's
        const double *row = src.row(b, cand[best], v.D);
        double *cen = v.cen + ((uint64_t)2 * st->koff + step) * v.D;
        for (uint64_t d = t; d < v.D; d += 256) cen[d] = Rows::value(row[d], src.shift(b, d, v.D));
        double *closest = v.closest + (uint64_t)b * n;
        for (uint64_t i = lo; i < hi; ++i) closest[i] = td[best * n + i];
    }
    if (draws == nullptr) return;
    if (t == 0) {
        double run = 0.0;
        for (int j = 0; j < 256; ++j) { pre[j] = run; run += part[best][j]; }
        pre[256] = run;
    }
    if (t < KB_MAX_TRIALS) {
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
// of value - centre by fma, the butterfly, the strict comparison that keeps the lower centre index -- with KB_ROWS_ASSIGN
// rows per wave sharing each centre value they load.  final = 1: the extra E-step of the problems that stopped on the
// centre shift.
template <class Rows>
__global__ __launch_bounds__(256) void kb_assign_kernel(KbView v, Rows src, int final) {
    const uint32_t b = blockIdx.y;
    KbState *st = v.st + b;
    if (final ? (st->strict != 0) : (st->active == 0)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t i0 = w * KB_ROWS_ASSIGN;
    if (i0 >= v.n) return;
    const uint32_t k = st->k;
    const double *cen = v.cen + ((uint64_t)2 * st->koff + (uint64_t)st->cur * k) * v.D;
    const double *rows[KB_ROWS_ASSIGN];
#pragma unroll
    for (int r = 0; r < KB_ROWS_ASSIGN; ++r) rows[r] = src.row(b, kb_min(i0 + r, v.n - 1), v.D);
    double best[KB_ROWS_ASSIGN], second[KB_ROWS_ASSIGN];
    uint32_t bi[KB_ROWS_ASSIGN];
#pragma unroll
    for (int r = 0; r < KB_ROWS_ASSIGN; ++r) { best[r] = INFINITY; second[r] = INFINITY; bi[r] = 0; }
    for (uint32_t c = 0; c < k; ++c) {
        double acc[KB_ROWS_ASSIGN];
#pragma unroll
        for (int r = 0; r < KB_ROWS_ASSIGN; ++r) acc[r] = 0.0;
        const double *cc = cen + (uint64_t)c * v.D;
        for (uint64_t d = lane; d < v.D; d += 64) {
            const double m = src.shift(b, d, v.D), cv = cc[d];
#pragma unroll
            for (int r = 0; r < KB_ROWS_ASSIGN; ++r) {
                const double e = Rows::value(rows[r][d], m) - cv;
                acc[r] = fma(e, e, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < KB_ROWS_ASSIGN; ++r) {
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
        for (int r = 0; r < KB_ROWS_ASSIGN; ++r) {
            const uint64_t i = i0 + r;
            if (i >= v.n) continue;
            if (labels[i] != bi[r]) atomicAdd(&st->changed, 1u);
            labels[i] = bi[r];
            if (k > 1 && second[r] > 0.0 && second[r] < INFINITY)
                atomicMin(&st->gapbits, (unsigned long long)__double_as_longlong((second[r] - best[r]) / second[r]));
        }
    }
}

// km_update_kernel for a chunk: new centre = mean of the members' values in row order, written to the other centre buffer
// (an empty cluster keeps its centre); one workgroup per (centre, problem)
template <class Rows>
__global__ __launch_bounds__(256) void kb_update_kernel(KbView v, Rows src) {
    const uint32_t c = blockIdx.x, b = blockIdx.y;
    KbState *st = v.st + b;
    const uint32_t k = st->k;
    if (st->active == 0 || c >= k) return;
    const double *old = v.cen + ((uint64_t)2 * st->koff + (uint64_t)st->cur * k + c) * v.D;
    double *cen = v.cen + ((uint64_t)2 * st->koff + (uint64_t)(st->cur ^ 1u) * k + c) * v.D;
    const uint32_t *labels = v.labels + (uint64_t)b * v.n;
    uint32_t cnt = 0;
    for (uint64_t d = threadIdx.x; d < v.D; d += 256) {
        const double mu = src.shift(b, d, v.D);
        double s = 0.0;
        uint32_t m = 0;
        for (uint64_t i = 0; i < v.n; ++i)
            if (labels[i] == c) { s += Rows::value(src.row(b, i, v.D)[d], mu); ++m; }
        cen[d] = m ? s / (double)m : old[d];
        cnt = m;
    }
    if (threadIdx.x == 0) v.sizes[st->koff + c] = cnt;
}

// km_shift_kernel + the host's stopping rule, per problem: total squared centre shift (same summation order), empty
// clusters, then "no label changed" (strict) or "shift <= tol" (one more E-step).  The new centres become current.
// (No rows are read: one instance per file that includes this header.)
static __global__ __launch_bounds__(256) void kb_stop_kernel(KbView v, uint32_t *__restrict__ n_active) {
    __shared__ double part[256];
    const uint32_t b = blockIdx.x;
    KbState *st = v.st + b;
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

// ---- host side ------------------------------------------------------------------------------------------------------
// scikit-learn's seeding trials per centre, and the uniforms a problem's seeding takes (none for its first centre)
static inline uint32_t kb_trials(uint32_t k) { return 2 + (uint32_t)std::log((double)k); }
static inline uint64_t kb_draws(uint32_t k) { return (uint64_t)(k - 1) * kb_trials(k); }

// what every client refuses: of a call, and of its problem s (k centres among n rows); fname = the client's entry point
static inline int kb_check_call(const char *fname, int max_iter, uint32_t chunk) {
    PHK_REQUIRE(max_iter >= 1 && chunk <= 65535, "%s: bad max_iter / chunk", fname);
    return PHK_OK;
}
static inline int kb_check_problem(const char *fname, uint64_t s, uint32_t k, uint64_t n, uint32_t first_seed, const double *draws) {
    PHK_REQUIRE(k >= 1 && k <= n, "%s: need 1 <= k <= n (problem %llu: k=%u, n=%llu)", fname, (unsigned long long)s, k,
                (unsigned long long)n);
    PHK_REQUIRE(first_seed < n, "%s: first seed %u of problem %llu is not a row", fname, first_seed, (unsigned long long)s);
    PHK_REQUIRE(kb_trials(k) <= KB_MAX_TRIALS, "%s: k = %u needs %u seeding trials per centre, at most %d are built", fname, k,
                kb_trials(k), KB_MAX_TRIALS);
    PHK_REQUIRE(draws || k == 1, "%s: NULL draws", fname);
    return PHK_OK;
}

// What the workspace has to hold: the most of each over the call's chunks.
struct KbExtent {
    uint64_t problems, rows, D;   // problems of a chunk; rows of a problem; columns
    uint64_t ksum;                // centres of a chunk's problems
    uint32_t trials;              // trial stride of td
    uint64_t draws;               // uniforms of a chunk
};

// The extent of the chunks [cut[c], cut[c + 1]) of the problems ks[order[p]] (order = nullptr: as given), n rows each at most.
static inline KbExtent kb_extent(const uint32_t *ks, const uint64_t *order, const std::vector<uint64_t> &cut, uint64_t n, uint64_t D) {
    KbExtent e = {0, n, D, 0, KB_MAX_TRIALS, 0};
    for (uint64_t c = 0; c + 1 < cut.size(); ++c) {
        uint64_t ksum = 0, dsum = 0;
        for (uint64_t p = cut[c]; p < cut[c + 1]; ++p) {
            const uint32_t k = ks[order ? order[p] : p];
            ksum += k;
            dsum += kb_draws(k);
        }
        e.problems = std::max(e.problems, cut[c + 1] - cut[c]);
        e.ksum = std::max(e.ksum, ksum);
        e.draws = std::max(e.draws, dsum);
    }
    return e;
}

// The core's regions of a client's workspace: taken from the client's layout (its own regions go before or behind, in the
// same allocation), bound to the allocation's address afterwards.
struct KbSpace {
    KbExtent e;
    uint64_t o_cen, o_lab, o_clo, o_td, o_cand, o_seed, o_size, o_st, o_draw, o_act;
    KbSpace(PhkLayout &ws, const KbExtent &x) : e(x) {
        o_cen = ws.take(2 * e.ksum * e.D * 8);
        o_lab = ws.take(e.problems * e.rows * 4);
        o_clo = ws.take(e.problems * e.rows * 8);
        o_td = ws.take(e.problems * e.trials * e.rows * 8);
        o_cand = ws.take(e.problems * KB_MAX_TRIALS * 4);
        o_seed = ws.take(e.ksum * 4);
        o_size = ws.take(e.ksum * 4);
        o_st = ws.take(e.problems * sizeof(KbState));
        o_draw = ws.take(e.draws * 8 + 8);
        o_act = ws.take(256);
    }
    // the view of chunks of e.rows rows (a chunk of fewer sets v.n) and the device word of kb_solve_chunk's read-back
    KbView bind(void *base, uint32_t **d_active) const {
        char *w = (char *)base;
        KbView v;
        v.cen = (double *)(w + o_cen);
        v.labels = (uint32_t *)(w + o_lab);
        v.closest = (double *)(w + o_clo);
        v.td = (double *)(w + o_td);
        v.cand = (uint32_t *)(w + o_cand);
        v.seeds = (uint32_t *)(w + o_seed);
        v.sizes = (uint32_t *)(w + o_size);
        v.st = (KbState *)(w + o_st);
        v.draws = (const double *)(w + o_draw);
        v.n = e.rows;
        v.D = e.D;
        v.trials = e.trials;
        *d_active = (uint32_t *)(w + o_act);
        return v;
    }
};

// the host's side of a chunk: the problems' states and first centres, filled by add(), sent by upload(), back by download()
struct KbChunk {
    std::vector<KbState> st;
    std::vector<uint32_t> cand;   // [problems][KB_MAX_TRIALS], the first centre's row in front
    uint32_t ksum = 0, kmax = 0;  // centres of the chunk's problems, and the most of one problem
    uint64_t dsum = 0;            // draws of the chunk's problems so far

    void clear() {
        st.clear();
        cand.clear();
        ksum = kmax = 0;
        dsum = 0;
    }
    // a problem whose draws are in the workspace already, at doff (the placement: one set for every problem)
    void add(uint32_t k, uint32_t first_seed, uint64_t doff, double tol) {
        KbState s;
        memset(&s, 0, sizeof(s));
        s.k = k;
        s.T = kb_trials(k);
        s.koff = ksum;
        s.doff = doff;
        s.active = 1;
        s.seed_margin = INFINITY;
        s.tol = tol;
        const double inf = INFINITY;
        memcpy(&s.gapbits, &inf, 8);
        st.push_back(s);
        cand.resize(cand.size() + KB_MAX_TRIALS, 0u);
        cand[cand.size() - KB_MAX_TRIALS] = first_seed;
        ksum += k;
        kmax = std::max(kmax, k);
    }
    // a problem and its own kb_draws(k) uniforms, which go up behind those of the chunk's earlier problems
    int add(phk_ctx *ctx, const KbView &v, uint32_t k, uint32_t first_seed, const double *draws, double tol) {
        add(k, first_seed, dsum, tol);
        const uint64_t nd = kb_draws(k);
        if (nd) PHK_HIP(hipMemcpyAsync((double *)v.draws + dsum, draws, nd * 8, hipMemcpyHostToDevice, ctx->stream));
        dsum += nd;
        return PHK_OK;
    }
    int upload(phk_ctx *ctx, const KbView &v) const {
        PHK_HIP(hipMemcpyAsync(v.st, st.data(), st.size() * sizeof(KbState), hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(v.cand, cand.data(), cand.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemsetAsync(v.labels, 0xFF, st.size() * v.n * 4, ctx->stream));
        return PHK_OK;
    }
    // after kb_solve_chunk and whatever the client queued behind it: the states back, the stream drained; then per problem
    int download(phk_ctx *ctx, const KbView &v) {
        PHK_HIP(hipMemcpyAsync(st.data(), v.st, st.size() * sizeof(KbState), hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        return PHK_OK;
    }
    int32_t n_iter(uint64_t b) const { return (int32_t)st[b].n_iter; }
    double seed_margin(uint64_t b) const { return st[b].seed_margin; }
    bool met_empty(uint64_t b) const { return st[b].n_empty != 0; }
    double min_gap(uint64_t b) const {
        double gap;
        static_assert(sizeof(gap) == sizeof(st[b].gapbits), "");
        memcpy(&gap, &st[b].gapbits, 8);
        return gap;
    }
};

struct KbNames {              // the launches' names in the profile
    const char *seed_dist, *seed_choose, *assign, *update, *stop;
};

// Seeding, Lloyd sweeps and the final E-step of an uploaded chunk; d_active = one device word for the sweeps' read-back.
template <class Rows>
static int kb_solve_chunk(phk_ctx *ctx, const KbView &v, const Rows &src, const KbChunk &ch, int max_iter, uint32_t *d_active,
                          const KbNames &names) {
    const unsigned gb = (unsigned)ch.st.size();
    const unsigned seed_blocks = (unsigned)phk_div_up(phk_div_up(v.n, KB_ROWS_SEED), 4);
    const unsigned assign_blocks = (unsigned)phk_div_up(phk_div_up(v.n, KB_ROWS_ASSIGN), 4);
    // seeding: centre 0 is the caller's row, then up to kmax - 1 greedy steps; a problem with k <= step returns at once
    for (uint32_t c = 0; c < ch.kmax; ++c) {
        PHK_LAUNCH(ctx, names.seed_dist, kb_seed_dist_kernel<Rows><<<dim3(seed_blocks, gb), dim3(256), 0, ctx->stream>>>(v, src, c));
        PHK_LAUNCH(ctx, names.seed_choose, kb_seed_choose_kernel<Rows><<<dim3(gb), dim3(256), 0, ctx->stream>>>(v, src, c));
    }
    // Lloyd: one host synchronisation per sweep for the whole chunk (the number of problems still sweeping)
    for (int it = 0; it < max_iter; ++it) {
        PHK_HIP(hipMemsetAsync(d_active, 0, 4, ctx->stream));
        PHK_LAUNCH(ctx, names.assign, kb_assign_kernel<Rows><<<dim3(assign_blocks, gb), dim3(256), 0, ctx->stream>>>(v, src, 0));
        PHK_LAUNCH(ctx, names.update, kb_update_kernel<Rows><<<dim3(ch.kmax, gb), dim3(256), 0, ctx->stream>>>(v, src));
        PHK_LAUNCH(ctx, names.stop, kb_stop_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(v, d_active));
        uint32_t active = 0;
        PHK_HIP(hipMemcpyAsync(&active, d_active, 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        if (active == 0) break;
    }
    PHK_LAUNCH(ctx, names.assign, kb_assign_kernel<Rows><<<dim3(assign_blocks, gb), dim3(256), 0, ctx->stream>>>(v, src, 1));
    return PHK_OK;
}
