// cluster.hip -- the clustering analysis of PhaMers' scripts/learning.py on the device (gfx950):
//   phk_silhouettes : learning.silhouettes (:84-92, scikit-learn silhouette_samples)
//   phk_dbscan      : learning.dbscan (:149-163, scikit-learn DBSCAN(eps, min_samples).fit(X).labels_)
// (phk_dbscan_sweep, the same for a whole eps x min_samples grid in one pass over the pairs: dbscan_sweep.hip)
//
// Both are all-pairs passes over X[n][D] float64.  Every pass is built on one pair tile: 64 query rows x 64 column rows,
// 256 threads, each thread a 4 x 4 block of pairs (queries ty + 16 r, columns tx + 16 c); KC columns of both row sets are
// staged in LDS per step.  Distances are float64 DIRECT DIFFERENCES, s_ij = sum_k (x_ik - x_jk)^2 accumulated by fma in
// column order, d_ij = sqrt(s_ij): the same value for (i, j) and (j, i), for any tiling, and no rounding bound to certify
// ("Clustering").
//
// DBSCAN's neighbour test d_ij <= eps is decided as s_ij <= t, t = the largest double whose correctly rounded square root
// is <= eps (computed on the host): exactly the float64 decision sqrt(s_ij) <= eps.
#include "cluster_shared.h"
#include "pair_tile.h"

#include <algorithm>
#include <cmath>

// ---- silhouettes -------------------------------------------------------------------------------------------------------
// Columns are visited through perm (rows sorted by label, stable), cut into chunks of at most CL_T rows that never straddle
// two clusters: chunk k = rows perm[cstart[k] .. cstart[k] + clen[k]) of cluster ccl[k]; cflag[k] = 1 on a cluster's last
// chunk.  Workgroup (query block, group g) walks chunks [gbeg[g], gbeg[g + 1]) -- groups are cut at cluster boundaries --
// and writes sums[q - q0][c] = sum_{j in c} d(q, j) for each cluster it finishes.  The order of every such sum is fixed
// by the labels alone: a thread adds its columns tx, tx + 16, ... chunk by chunk, then the 16 threads of a query fold by a
// fixed butterfly.
__global__ __launch_bounds__(CL_THREADS) void phk_cl_silhouette_sums_kernel(
    const double *__restrict__ X, uint64_t n, uint64_t D, const int32_t *__restrict__ perm, const uint32_t *__restrict__ cstart,
    const uint32_t *__restrict__ clen, const uint32_t *__restrict__ ccl, const uint8_t *__restrict__ cflag,
    const uint32_t *__restrict__ gbeg, uint64_t qb0, uint64_t q0, uint64_t nq, uint32_t K, double *__restrict__ sums) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t qbase = (qb0 + blockIdx.x) * CL_T;   // first query row of the block (original order)
    const uint32_t g = blockIdx.y;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = gbeg[g]; k < gbeg[g + 1]; ++k) {
        const uint32_t cs = cstart[k], cl = clen[k];
        double s[4][4];
        cl_tile({X, nullptr, q0 + nq, qbase}, {X, perm, (uint64_t)cs + cl, cs}, D, Qs, Cs, s);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if ((uint32_t)(tx + 16 * c) < cl) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] += sqrt(s[r][c]);
            }
        if (cflag[k]) {
            const uint32_t cid = ccl[k];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double v = acc[r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
                const uint64_t q = qbase + ty + 16 * r;
                if (tx == 0 && q < q0 + nq) sums[(q - q0) * K + cid] = v;
                acc[r] = 0.0;
            }
        }
    }
}

// One thread per query of the batch: scikit-learn's silhouette_samples from the cluster sums (sklearn/metrics/cluster/
// _unsupervised.py): a = sum_own / (n_own - 1), b = min over the other clusters of sum_c / n_c, s = (b - a) / max(a, b),
// NaN (a singleton's 0 / 0, or a = b = 0) -> 0.  Clusters without members take no part in b.
__global__ __launch_bounds__(256) void phk_cl_silhouette_finish_kernel(const double *__restrict__ sums, const uint32_t *__restrict__ labels,
                                                                      const uint32_t *__restrict__ sizes, uint64_t q0, uint64_t nq,
                                                                      uint32_t K, double *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t own = labels[q0 + i];
    const double *row = sums + i * K;
    const double a = row[own] / (double)(sizes[own] - 1u);
    double b = __builtin_inf();
    for (uint32_t c = 0; c < K; ++c)
        if (c != own && sizes[c]) b = fmin(b, row[c] / (double)sizes[c]);
    const double s = (b - a) / fmax(a, b);
    out[q0 + i] = s == s ? s : 0.0;
}

// ---- DBSCAN ------------------------------------------------------------------------------------------------------------
// Pass 1: neighbour counts, self included.  Workgroup (query block, column group g) counts the column tiles
// [g T / G, (g + 1) T / G) and adds its per-query totals to cnt[] (integer atomics: the result is order-free).
__global__ __launch_bounds__(CL_THREADS) void phk_cl_count_kernel(const double *__restrict__ X, uint64_t n, uint64_t D, double t,
                                                                  uint64_t qb0, uint32_t groups, uint32_t *__restrict__ cnt) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t qbase = (qb0 + blockIdx.x) * CL_T;
    const uint64_t T = (n + CL_T - 1) / CL_T;
    const uint64_t j0 = T * blockIdx.y / groups, j1 = T * (blockIdx.y + 1) / groups;
    uint32_t c4[4] = {0, 0, 0, 0};
    for (uint64_t J = j0; J < j1; ++J) {
        double s[4][4];
        cl_tile({X, nullptr, n, qbase}, {X, nullptr, n, J * CL_T}, D, Qs, Cs, s);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (J * CL_T + tx + 16 * c < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) c4[r] += s[r][c] <= t ? 1u : 0u;
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint32_t v = c4[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
        const uint64_t q = qbase + ty + 16 * r;
        if (tx == 0 && q < n && v) atomicAdd(&cnt[q], v);
    }
}

// (The union-find on the parent array and on the LDS slots -- uf_union, lf_union -- is in cluster_shared.h.)
// Pass 2: joins every core-core neighbour pair.  Tile (I, J) of the core points with I <= J (symmetry: d_ij = d_ji bit for
// bit); its edges are first joined on 128 slots in LDS (slot r: core point 64 I + r, slot 64 + c: core point 64 J + c; the
// diagonal tile uses slots 0..63 for both), then each slot is joined to its LDS root in the global parent array: at most
// 127 global unions per tile, however many of its 4096 pairs are edges.
__global__ __launch_bounds__(CL_THREADS) void phk_cl_union_kernel(const double *__restrict__ X, uint64_t D, double t,
                                                                  const int32_t *__restrict__ core, uint64_t nc, uint64_t ib0,
                                                                  int32_t *parent) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    __shared__ int lp[2 * CL_T];
    const uint64_t I = ib0 + blockIdx.y, J = blockIdx.x;
    if (I > J) return;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const bool diag = I == J;
    if (threadIdx.x < 2 * CL_T) lp[threadIdx.x] = threadIdx.x;
    double s[4][4];
    cl_tile({X, core, nc, I * CL_T}, {X, core, nc, J * CL_T}, D, Qs, Cs, s);   // (its barriers order the lp init)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int qi = ty + 16 * r, cj = tx + 16 * c;
            if (s[r][c] <= t && I * CL_T + qi < nc && J * CL_T + cj < nc) lf_union(lp, qi, diag ? cj : CL_T + cj);
        }
    __syncthreads();
    const int x = threadIdx.x;
    if (x < 2 * CL_T && !(diag && x >= CL_T)) {
        const int r = lf_find(lp, x);
        if (r != x) {
            const uint64_t gx = x < CL_T ? I * CL_T + x : J * CL_T + (x - CL_T);
            const uint64_t gr = r < CL_T ? I * CL_T + r : J * CL_T + (r - CL_T);
            uf_union(parent, (int32_t)gr, (int32_t)gx);
        }
    }
}

// Path compression, a launch of its own: root[m] = the root of core point m (plain loads: pass 2 has completed).
__global__ __launch_bounds__(256) void phk_cl_compress_kernel(const int32_t *__restrict__ parent, uint64_t nc, int32_t *__restrict__ root) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nc) return;
    int32_t x = (int32_t)m;
    for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[m] = x;
}

// Label pass for the border points: each non-core point q (row nonc[q]) takes the smallest label of its core neighbours
// (core point m: row core[m], label clab[m]) by an integer atomic min; INT32_MAX = none (noise).
__global__ __launch_bounds__(CL_THREADS) void phk_cl_border_kernel(const double *__restrict__ X, uint64_t D, double t,
                                                                   const int32_t *__restrict__ nonc, uint64_t nn,
                                                                   const int32_t *__restrict__ core, const int32_t *__restrict__ clab,
                                                                   uint64_t nc, uint64_t qb0, uint32_t groups,
                                                                   int32_t *__restrict__ blab) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t qbase = (qb0 + blockIdx.x) * CL_T;
    const uint64_t T = (nc + CL_T - 1) / CL_T;
    const uint64_t j0 = T * blockIdx.y / groups, j1 = T * (blockIdx.y + 1) / groups;
    int32_t m4[4] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};
    for (uint64_t J = j0; J < j1; ++J) {
        double s[4][4];
        cl_tile({X, nonc, nn, qbase}, {X, core, nc, J * CL_T}, D, Qs, Cs, s);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t m = J * CL_T + tx + 16 * c;
            if (m < nc) {
                const int32_t l = clab[m];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (s[r][c] <= t) m4[r] = min(m4[r], l);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int32_t v = m4[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v = min(v, __shfl_xor(v, o));
        const uint64_t q = qbase + ty + 16 * r;
        if (tx == 0 && q < nn && v != INT32_MAX) atomicMin(&blab[q], v);
    }
}

// any NaN among n elements -> *flag != 0
__global__ __launch_bounds__(256) void phk_cl_nan_kernel(const double *__restrict__ X, uint64_t n, uint32_t *__restrict__ flag) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        bad |= X[i] != X[i];
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void phk_cl_fill_kernel(int32_t *__restrict__ p, uint64_t n, int32_t v, int iota) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = iota ? (int32_t)i : v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// PHK_ERR_NAN when any of the `count` doubles at d_p (device) is NaN; returns with the stream idle (dbscan_sweep.hip calls it too)
int cl_refuse_nan(phk_ctx *ctx, const char *fname, const double *d_p, uint64_t count) {
    void *flags;
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &flags));
    PHK_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), ctx->stream));
    const uint64_t blocks = std::min<uint64_t>(phk_div_up(count, 256), 4096);
    if (blocks)
        PHK_LAUNCH(ctx, "phk_cl_nan_kernel",
                   phk_cl_nan_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(d_p, count, (uint32_t *)flags));
    uint32_t bad = 0;
    PHK_HIP(hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (bad) {
        phk_set_error("%s: the data contain NaN", fname);
        return PHK_ERR_NAN;
    }
    return PHK_OK;
}

// X to the device (WS_WIDE) and the NaN check.  Returns the device copy.
static int cl_upload(phk_ctx *ctx, const char *fname, const double *X, uint64_t n, uint64_t D, uint64_t extra_bytes,
                     double **d_x, void **d_extra) {
    void *p;
    const uint64_t xb = (n * D * sizeof(double) + 255) & ~255ull;
    PHK_TRY(phk_ws(ctx, WS_WIDE, xb + extra_bytes, &p));
    PHK_TRY(phk_copy_to_device(ctx, p, X, n * D * sizeof(double)));
    PHK_TRY(cl_refuse_nan(ctx, fname, (const double *)p, n * D));
    *d_x = (double *)p;
    *d_extra = (char *)p + xb;
    return PHK_OK;
}

// workgroups per query block so that a launch fills the chip (~8 workgroups per CU), at most `tiles`
uint32_t cl_groups(phk_ctx *ctx, uint64_t qblocks, uint64_t tiles) {
    const uint64_t want = (uint64_t)ctx->num_cus * 8;
    uint64_t g = qblocks >= want ? 1 : phk_div_up(want, qblocks);
    if (g > tiles) g = tiles;
    return (uint32_t)(g ? g : 1);
}

// X = the rows on the host, or NULL with d_rows = the same rows already on the device (checked for NaN by their owner)
static int cl_silhouettes(phk_ctx *ctx, const double *X, const double *d_rows, uint64_t n, uint64_t D, const uint32_t *labels,
                          uint32_t n_labels, double *out) {
    PHK_ENTER(ctx, "phk_silhouettes");
    PHK_REQUIRE((X || d_rows) && labels && out, "phk_silhouettes: NULL pointer");
    PHK_REQUIRE(D >= 1 && n < (1ull << 31), "phk_silhouettes: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)D);
    PHK_REQUIRE(n_labels >= 2 && (uint64_t)n_labels <= n - 1 && n >= 3,
                "phk_silhouettes: Number of labels is %u. Valid values are 2 to n_samples - 1 (inclusive)", n_labels);
    const uint32_t K = n_labels;
    std::vector<uint32_t> sizes(K, 0);
    for (uint64_t i = 0; i < n; ++i) {
        PHK_REQUIRE(labels[i] < K, "phk_silhouettes: label %u of row %llu is not below n_labels = %u", labels[i],
                    (unsigned long long)i, K);
        ++sizes[labels[i]];
    }
    // rows sorted by label (stable), each cluster cut into chunks of at most CL_T rows
    std::vector<uint64_t> first(K + 1, 0);
    for (uint32_t c = 0; c < K; ++c) first[c + 1] = first[c] + sizes[c];
    std::vector<int32_t> perm(n);
    {
        std::vector<uint64_t> at(first.begin(), first.end() - 1);
        for (uint64_t i = 0; i < n; ++i) perm[at[labels[i]]++] = (int32_t)i;
    }
    std::vector<uint32_t> cstart, clen, ccl;
    std::vector<uint8_t> cflag;
    for (uint32_t c = 0; c < K; ++c)
        for (uint64_t s = first[c]; s < first[c + 1]; s += CL_T) {
            cstart.push_back((uint32_t)s);
            clen.push_back((uint32_t)std::min<uint64_t>(CL_T, first[c + 1] - s));
            ccl.push_back(c);
            cflag.push_back(s + CL_T >= first[c + 1]);
        }
    const uint64_t nch = cstart.size();
    // query batches: the cluster sums of a batch within 256 MiB; column groups cut at cluster ends
    uint64_t B = (256ull << 20) / ((uint64_t)K * sizeof(double));
    B = B < CL_T ? CL_T : (B / CL_T) * CL_T;
    if (B > n) B = n;
    const uint64_t qblocks = phk_div_up(B, CL_T);
    const uint32_t G = cl_groups(ctx, qblocks, nch);
    std::vector<uint32_t> gbeg(1, 0);
    for (uint64_t k = 0; k < nch && gbeg.size() < G; ++k)
        if (cflag[k] && (k + 1) * G >= nch * gbeg.size() && k + 1 < nch) gbeg.push_back((uint32_t)(k + 1));
    gbeg.push_back((uint32_t)nch);
    const uint32_t ng = (uint32_t)gbeg.size() - 1;

    const uint64_t o_perm = 0, o_lab = o_perm + n * 4, o_size = o_lab + n * 4, o_cs = o_size + K * 4ull, o_cl = o_cs + nch * 4,
                   o_cc = o_cl + nch * 4, o_gb = o_cc + nch * 4, o_cf = o_gb + (ng + 1) * 4ull;
    const uint64_t meta = (o_cf + nch + 255) & ~255ull;
    double *d_x;
    void *d_meta;
    if (X) {
        PHK_TRY(cl_upload(ctx, "phk_silhouettes", X, n, D, meta + B * K * sizeof(double) + n * sizeof(double), &d_x, &d_meta));
    } else {
        PHK_TRY(phk_ws(ctx, WS_WIDE, meta + B * K * sizeof(double) + n * sizeof(double), &d_meta));
        d_x = const_cast<double *>(d_rows);
    }
    char *mb = (char *)d_meta;
    double *d_sums = (double *)(mb + meta), *d_out = d_sums + B * K;
    PHK_HIP(hipMemcpyAsync(mb + o_perm, perm.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(mb + o_lab, labels, n * 4, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(mb + o_size, sizes.data(), K * 4ull, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(mb + o_cs, cstart.data(), nch * 4, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(mb + o_cl, clen.data(), nch * 4, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(mb + o_cc, ccl.data(), nch * 4, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(mb + o_gb, gbeg.data(), (ng + 1) * 4ull, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(mb + o_cf, cflag.data(), nch, hipMemcpyHostToDevice, ctx->stream));
    for (uint64_t q0 = 0; q0 < n; q0 += B) {
        const uint64_t nq = std::min(B, n - q0), qb = phk_div_up(nq, CL_T);
        const uint64_t step = std::max<uint64_t>(1, CL_MAX_BLOCKS / ng);
        for (uint64_t b0 = 0; b0 < qb; b0 += step) {
            const unsigned nb = (unsigned)std::min(step, qb - b0);
            PHK_LAUNCH(ctx, "phk_cl_silhouette_sums_kernel",
                       phk_cl_silhouette_sums_kernel<<<dim3(nb, ng), dim3(CL_THREADS), 0, ctx->stream>>>(
                           d_x, n, D, (const int32_t *)(mb + o_perm), (const uint32_t *)(mb + o_cs), (const uint32_t *)(mb + o_cl),
                           (const uint32_t *)(mb + o_cc), (const uint8_t *)(mb + o_cf), (const uint32_t *)(mb + o_gb),
                           q0 / CL_T + b0, q0, nq, K, d_sums));
        }
        PHK_LAUNCH(ctx, "phk_cl_silhouette_finish_kernel",
                   phk_cl_silhouette_finish_kernel<<<dim3((unsigned)phk_div_up(nq, 256)), dim3(256), 0, ctx->stream>>>(
                       d_sums, (const uint32_t *)(mb + o_lab), (const uint32_t *)(mb + o_size), q0, nq, K, d_out));
    }
    return phk_copy_to_host(ctx, out, d_out, n * sizeof(double));
}

extern "C" int phk_silhouettes(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const uint32_t *labels, uint32_t n_labels,
                               double *out) {
    PHK_REQUIRE(X, "phk_silhouettes: NULL pointer");
    return cl_silhouettes(ctx, X, nullptr, n, D, labels, n_labels, out);
}

int phk_silhouettes_resident(phk_ctx *ctx, const double *d_rows, uint64_t n, uint64_t D, const uint32_t *labels, uint32_t n_labels,
                             double *out) {
    return cl_silhouettes(ctx, nullptr, d_rows, n, D, labels, n_labels, out);
}

// the largest double t with sqrt(t) <= eps (sqrt correctly rounded and monotone): s <= t  <=>  sqrt(s) <= eps
double cl_eps_threshold(double eps) {
    double t = eps * eps;
    while (std::sqrt(t) > eps) t = std::nextafter(t, 0.0);
    for (;;) {
        const double u = std::nextafter(t, __builtin_inf());
        if (!(std::sqrt(u) <= eps)) return t;
        t = u;
    }
}

extern "C" int phk_dbscan(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, double eps, uint64_t min_samples, int64_t *labels,
                          uint8_t *core, uint64_t *n_clusters) {
    PHK_ENTER(ctx, "phk_dbscan");
    PHK_REQUIRE(eps > 0.0 && eps < __builtin_inf(), "phk_dbscan: eps must be finite and > 0 (got %g)", eps);
    PHK_REQUIRE(min_samples >= 1, "phk_dbscan: min_samples must be >= 1");
    PHK_REQUIRE(D >= 1 && n < (1ull << 31), "phk_dbscan: bad shape (%llu x %llu)", (unsigned long long)n, (unsigned long long)D);
    if (n == 0) {
        if (n_clusters) *n_clusters = 0;
        return PHK_OK;
    }
    PHK_REQUIRE(X && labels, "phk_dbscan: NULL pointer");
    const double t = cl_eps_threshold(eps);
    // device: X | cnt / parent [n] | root [n] | core rows [n] | non-core rows [n] | core labels [n] | border labels [n]
    double *d_x;
    void *d_extra;
    PHK_TRY(cl_upload(ctx, "phk_dbscan", X, n, D, 6 * n * sizeof(int32_t), &d_x, &d_extra));
    int32_t *d_cnt = (int32_t *)d_extra, *d_root = d_cnt + n, *d_core = d_root + n, *d_nonc = d_core + n, *d_clab = d_nonc + n,
            *d_blab = d_clab + n;
    // pass 1: neighbour counts
    PHK_HIP(hipMemsetAsync(d_cnt, 0, n * sizeof(int32_t), ctx->stream));
    const uint64_t T = (n + CL_T - 1) / CL_T;
    {
        const uint32_t G = cl_groups(ctx, T, T);
        const uint64_t step = std::max<uint64_t>(1, CL_MAX_BLOCKS / G);
        for (uint64_t b0 = 0; b0 < T; b0 += step)
            PHK_LAUNCH(ctx, "phk_cl_count_kernel",
                       phk_cl_count_kernel<<<dim3((unsigned)std::min(step, T - b0), G), dim3(CL_THREADS), 0, ctx->stream>>>(
                           d_x, n, D, t, b0, G, (uint32_t *)d_cnt));
    }
    std::vector<uint32_t> cnt(n);
    PHK_TRY(phk_copy_to_host(ctx, cnt.data(), d_cnt, n * sizeof(uint32_t)));
    std::vector<int32_t> corei, nonci;
    for (uint64_t i = 0; i < n; ++i) (cnt[i] >= min_samples ? corei : nonci).push_back((int32_t)i);
    const uint64_t nc = corei.size(), nn = nonci.size();
    std::vector<int32_t> clab(nc);
    uint64_t K = 0;
    if (nc) {
        // pass 2: union-find over the core points, then path compression
        PHK_HIP(hipMemcpyAsync(d_core, corei.data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
        int32_t *d_parent = d_cnt;
        PHK_LAUNCH(ctx, "phk_cl_fill_kernel",
                   phk_cl_fill_kernel<<<dim3((unsigned)phk_div_up(nc, 256)), dim3(256), 0, ctx->stream>>>(d_parent, nc, 0, 1));
        const uint64_t Tc = phk_div_up(nc, CL_T);
        const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(65535, CL_MAX_BLOCKS / Tc));
        for (uint64_t i0 = 0; i0 < Tc; i0 += step)
            PHK_LAUNCH(ctx, "phk_cl_union_kernel",
                       phk_cl_union_kernel<<<dim3((unsigned)Tc, (unsigned)std::min(step, Tc - i0)), dim3(CL_THREADS), 0, ctx->stream>>>(
                           d_x, D, t, d_core, nc, i0, d_parent));
        PHK_LAUNCH(ctx, "phk_cl_compress_kernel",
                   phk_cl_compress_kernel<<<dim3((unsigned)phk_div_up(nc, 256)), dim3(256), 0, ctx->stream>>>(d_parent, nc, d_root));
        std::vector<int32_t> root(nc);
        PHK_TRY(phk_copy_to_host(ctx, root.data(), d_root, nc * sizeof(int32_t)));
        // roots (the smallest core point of each component) ranked in row order: scikit-learn's cluster numbering
        for (uint64_t m = 0; m < nc; ++m) clab[m] = root[m] == (int32_t)m ? (int32_t)K++ : clab[root[m]];
    }
    std::vector<int32_t> blab(nn, INT32_MAX);
    if (nc && nn) {
        PHK_HIP(hipMemcpyAsync(d_nonc, nonci.data(), nn * 4, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(d_clab, clab.data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
        PHK_LAUNCH(ctx, "phk_cl_fill_kernel",
                   phk_cl_fill_kernel<<<dim3((unsigned)phk_div_up(nn, 256)), dim3(256), 0, ctx->stream>>>(d_blab, nn, INT32_MAX, 0));
        const uint64_t Tq = phk_div_up(nn, CL_T), Tc = phk_div_up(nc, CL_T);
        const uint32_t G = cl_groups(ctx, Tq, Tc);
        const uint64_t step = std::max<uint64_t>(1, CL_MAX_BLOCKS / G);
        for (uint64_t b0 = 0; b0 < Tq; b0 += step)
            PHK_LAUNCH(ctx, "phk_cl_border_kernel",
                       phk_cl_border_kernel<<<dim3((unsigned)std::min(step, Tq - b0), G), dim3(CL_THREADS), 0, ctx->stream>>>(
                           d_x, D, t, d_nonc, nn, d_core, d_clab, nc, b0, G, d_blab));
        PHK_TRY(phk_copy_to_host(ctx, blab.data(), d_blab, nn * sizeof(int32_t)));
    }
    for (uint64_t m = 0; m < nc; ++m) labels[corei[m]] = clab[m];
    for (uint64_t m = 0; m < nn; ++m) labels[nonci[m]] = blab[m] == INT32_MAX ? -1 : blab[m];
    if (core) {
        for (uint64_t i = 0; i < n; ++i) core[i] = 0;
        for (uint64_t m = 0; m < nc; ++m) core[corei[m]] = 1;
    }
    if (n_clusters) *n_clusters = K;
    return PHK_OK;
}
