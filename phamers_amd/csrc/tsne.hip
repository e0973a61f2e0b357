// tsne.hip -- the embedding of phamer_scorer.do_tsne (scripts/phamer.py:337-366) on the device (gfx950):
//   phk_pca_covariance / phk_pca_project : PCA(n_components).fit_transform around a host eigendecomposition
//   phk_tsne_neighbors                   : the k nearest other rows of every row, ordered by (distance, index)
//   phk_tsne_affinities                  : scikit-learn's _binary_search_perplexity per row, on float64 squared distances
//   phk_tsne_symmetrize                  : P = (P + P^T) / sum P as CSR, by a reverse adjacency (host, O(n k))
//   phk_tsne_gradient / _descend / _fit  : the KL gradient with the repulsive term summed EXACTLY over all pairs, and
//                                          scikit-learn's _gradient_descent / TSNE._tsne around it
// Everything is float64.  No floating-point atomics anywhere: every sum is taken in an order fixed by the shapes (n, D, k)
// alone, so the results are bit-identical from run to run and do not depend on the number of compute units.
#include "gram_tile.h"
#include "pair_tile.h"
#include "row_select.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

#define TS_EPS 2.220446049250313e-16   // scikit-learn's MACHINE_EPSILON = np.finfo(np.double).eps
#define TS_BYTES_256M (256ull << 20)

// ---- fixed-order sums --------------------------------------------------------------------------------------------------
// the sum of one value per thread of a 256-thread workgroup by a fixed tree (every thread returns it)
__device__ __forceinline__ double ts_block_sum(double v, double *sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// out[b] = sum of in[b * stride .. + m), b = blockIdx.x: thread t adds elements t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(256) void phk_ts_total_kernel(const double *__restrict__ in, uint64_t m, uint64_t stride,
                                                          double *__restrict__ out) {
    __shared__ double sh[256];
    const double *p = in + blockIdx.x * stride;
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < m; i += 256) s += p[i];
    s = ts_block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- PCA ---------------------------------------------------------------------------------------------------------------
// Rows are cut into chunks of `rows_per_chunk` (a function of (n, D) only); per-chunk partial sums meet in chunk order.
// pm[chunk][d] = sum of column d over the chunk's rows, in row order.
__global__ __launch_bounds__(256) void phk_pca_colsum_kernel(const double *__restrict__ X, uint64_t n, uint64_t D,
                                                            uint64_t rows_per_chunk, double *__restrict__ pm) {
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const uint64_t r0 = (uint64_t)blockIdx.y * rows_per_chunk, r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
    double s = 0.0;
    for (uint64_t r = r0; r < r1; ++r) s += X[r * D + d];
    pm[(uint64_t)blockIdx.y * D + d] = s;
}

// out[e] = (sum over chunks, in chunk order, of part[chunk][e]) / denom, e < m
__global__ __launch_bounds__(256) void phk_pca_fold_kernel(const double *__restrict__ part, uint64_t m, uint64_t chunks,
                                                          double denom, double *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    double s = 0.0;
    for (uint64_t c = 0; c < chunks; ++c) s += part[c * m + e];
    out[e] = s / denom;
}

// part[chunk][a][b] = sum over the chunk's rows of (X[r][a] - mean[a]) (X[r][b] - mean[b]) on the fp64 matrix pipe
// (v_mfma_f64_16x16x4_f64; operand and accumulator layout: gram_tile.h).  Here k runs over 4 rows of X, i and j over columns.
// Workgroup = 4 waves = a 64 x 64 block of the covariance, each wave 2 x 2 tiles.  grid (D / 64, D / 64, chunks).
__global__ __launch_bounds__(256) void phk_pca_cov_kernel(const double *__restrict__ X, const double *__restrict__ mean, uint64_t n,
                                                         uint64_t D, uint64_t rows_per_chunk, double *__restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const uint64_t a0 = (uint64_t)blockIdx.x * 64 + (wave >> 1) * 32, b0 = (uint64_t)blockIdx.y * 64 + (wave & 1) * 32;
    const uint64_t r0 = (uint64_t)blockIdx.z * rows_per_chunk, r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
    uint64_t ca[2], cb[2];
    double ma[2], mb[2];
    bool oka[2], okb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        ca[t] = a0 + 16 * t + li;
        cb[t] = b0 + 16 * t + li;
        oka[t] = ca[t] < D;
        okb[t] = cb[t] < D;
        ma[t] = oka[t] ? mean[ca[t]] : 0.0;
        mb[t] = okb[t] ? mean[cb[t]] : 0.0;
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (uint64_t r = r0; r < r1; r += 4) {
        const uint64_t row = r + kk;
        const bool okr = row < r1;
        double va[2], vb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            va[t] = (okr && oka[t]) ? X[row * D + ca[t]] - ma[t] : 0.0;
            vb[t] = (okr && okb[t]) ? X[row * D + cb[t]] - mb[t] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[s], vb[t], acc[s][t], 0, 0, 0);
    }
    double *out = part + (uint64_t)blockIdx.z * D * D;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint64_t a = a0 + 16 * s + kk + 4 * g, b = b0 + 16 * t + li;
                if (a < D && b < D) out[a * D + b] = acc[s][t][g];
            }
}

// rows per chunk of the PCA sums: at least 1024, and few enough chunks that their D x D partials fit 256 MiB
static uint64_t pca_chunk_rows(uint64_t n, uint64_t D) {
    const uint64_t cap = std::min<uint64_t>(65535, std::max<uint64_t>(1, TS_BYTES_256M / (D * D * sizeof(double))));   // (grid z)
    uint64_t R = std::max<uint64_t>(1024, phk_div_up(n, cap));
    return (R + 3) & ~3ull;
}

extern "C" int phk_pca_covariance(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, double *mean, double *cov) {
    PHK_ENTER(ctx, "phk_pca_covariance");
    PHK_REQUIRE(X && mean && cov, "phk_pca_covariance: NULL pointer");
    PHK_REQUIRE(n >= 2 && D >= 1 && D <= 8192 && n < (1ull << 31), "phk_pca_covariance: bad shape (%llu x %llu)",
                (unsigned long long)n, (unsigned long long)D);
    const uint64_t R = pca_chunk_rows(n, D), chunks = phk_div_up(n, R);
    const uint64_t xb = (n * D * 8 + 255) & ~255ull, mb = (D * 8 + 255) & ~255ull, cb = (D * D * 8 + 255) & ~255ull;
    void *p;
    PHK_TRY(phk_ws(ctx, WS_WIDE, xb + mb + cb + chunks * cb, &p));
    double *d_x = (double *)p, *d_mean = (double *)((char *)p + xb), *d_cov = (double *)((char *)p + xb + mb),
           *d_part = (double *)((char *)p + xb + mb + cb);
    PHK_TRY(phk_copy_to_device(ctx, d_x, X, n * D * 8));
    PHK_LAUNCH(ctx, "phk_pca_colsum_kernel",
               phk_pca_colsum_kernel<<<dim3((unsigned)phk_div_up(D, 256), (unsigned)chunks), dim3(256), 0, ctx->stream>>>(d_x, n, D, R,
                                                                                                                    d_part));
    PHK_LAUNCH(ctx, "phk_pca_fold_kernel",
               phk_pca_fold_kernel<<<dim3((unsigned)phk_div_up(D, 256)), dim3(256), 0, ctx->stream>>>(d_part, D, chunks, (double)n,
                                                                                                    d_mean));
    const unsigned dt = (unsigned)phk_div_up(D, 64);
    PHK_LAUNCH(ctx, "phk_pca_cov_kernel",
               phk_pca_cov_kernel<<<dim3(dt, dt, (unsigned)chunks), dim3(256), 0, ctx->stream>>>(d_x, d_mean, n, D, R, d_part));
    PHK_LAUNCH(ctx, "phk_pca_fold_kernel",
               phk_pca_fold_kernel<<<dim3((unsigned)phk_div_up(D * D, 256)), dim3(256), 0, ctx->stream>>>(d_part, D * D, chunks,
                                                                                                        (double)(n - 1), d_cov));
    PHK_TRY(phk_copy_to_host(ctx, mean, d_mean, D * 8));
    return phk_copy_to_host(ctx, cov, d_cov, D * D * 8);
}

extern "C" int phk_pca_project(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const double *mean, const double *V,
                               uint64_t n_components, double *out) {
    PHK_ENTER(ctx, "phk_pca_project");
    PHK_REQUIRE(X && mean && V && out, "phk_pca_project: NULL pointer");
    PHK_REQUIRE(n >= 1 && D >= 1 && n_components >= 1 && n_components <= D && n < (1ull << 31),
                "phk_pca_project: bad shape (%llu x %llu -> %llu)", (unsigned long long)n, (unsigned long long)D,
                (unsigned long long)n_components);
    const uint64_t nc = n_components;
    const uint64_t xb = (n * D * 8 + 255) & ~255ull, mb = (D * 8 + 255) & ~255ull, vb = (nc * D * 8 + 255) & ~255ull;
    void *p;
    PHK_TRY(phk_ws(ctx, WS_WIDE, xb + mb + vb + n * nc * 8, &p));
    double *d_x = (double *)p, *d_mean = (double *)((char *)p + xb), *d_v = (double *)((char *)p + xb + mb),
           *d_out = (double *)((char *)p + xb + mb + vb);
    PHK_TRY(phk_copy_to_device(ctx, d_x, X, n * D * 8));
    PHK_TRY(phk_copy_to_device(ctx, d_mean, mean, D * 8));
    PHK_TRY(phk_copy_to_device(ctx, d_v, V, nc * D * 8));
    // out[i][c] = sum_d (X[i][d] - mean[d]) V[c][d], in column order: the pair tile with a product in place of the squared
    // difference and the mean taken off the query side
    const uint64_t rt = phk_div_up(n, CL_T);
    for (uint64_t b0 = 0; b0 < rt; b0 += 32768) {   // (grid y < 65536)
        const uint64_t nb = std::min<uint64_t>(32768, rt - b0), rows = std::min<uint64_t>(n - b0 * CL_T, nb * CL_T);
        PHK_LAUNCH(ctx, "phk_pca_project_kernel",
                   cl_matrix_kernel<ClStoreValue, CL_PRODUCT, true>
                   <<<dim3((unsigned)phk_div_up(nc, CL_T), (unsigned)nb), dim3(CL_THREADS), 0, ctx->stream>>>(
                       d_x + b0 * CL_T * D, rows, 0, d_v, nc, D, d_out + b0 * CL_T * nc, d_mean));
    }
    return phk_copy_to_host(ctx, out, d_out, n * nc * 8);
}

// ---- neighbour graph ---------------------------------------------------------------------------------------------------
#define TS_KMAX 4096   // neighbours per row the selection sorts in LDS (perplexity <= 1365)

// the neighbour graph's distance rows: +inf for j = q (a row is not its own neighbour)
struct TsStoreOffDiagonal {
    __device__ double operator()(uint64_t q, uint64_t j, double s) const { return j == q ? __builtin_inf() : s; }
};

// One workgroup per query row of the batch: the k smallest of its n distances, ordered by (distance, index) (row_select.h),
// as indices and squared distances.
__global__ __launch_bounds__(256) void phk_ts_select_kernel(const double *__restrict__ D2, uint64_t n, uint32_t k, uint32_t kp,
                                                           uint64_t q0, int32_t *__restrict__ idx_out, double *__restrict__ d2_out) {
    __shared__ uint64_t skey[TS_KMAX];
    __shared__ int32_t sidx[TS_KMAX];
    __shared__ RsScratch sc;
    rs_select_sorted((const uint64_t *)(D2 + (uint64_t)blockIdx.x * n), n, k, kp, skey, sidx, sc);
    const uint64_t q = q0 + blockIdx.x;
    for (uint32_t e = threadIdx.x; e < k; e += 256) {
        idx_out[q * k + e] = sidx[e];
        d2_out[q * k + e] = __longlong_as_double((long long)skey[e]);
    }
}

extern "C" int phk_tsne_neighbors(phk_ctx *ctx, const double *Z, uint64_t n, uint64_t d, uint64_t k, int32_t *idx, double *d2) {
    PHK_ENTER(ctx, "phk_tsne_neighbors");
    PHK_REQUIRE(Z && idx && d2, "phk_tsne_neighbors: NULL pointer");
    PHK_REQUIRE(n >= 2 && d >= 1 && n < (1ull << 24), "phk_tsne_neighbors: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)d);
    PHK_REQUIRE(k >= 1 && k <= n - 1 && k <= TS_KMAX, "phk_tsne_neighbors: k = %llu is not in 1..min(n - 1, %d)",
                (unsigned long long)k, TS_KMAX);
    uint32_t kp = 2;
    while (kp < k) kp <<= 1;
    // query batches: the distance rows of a batch within 256 MiB, a multiple of the tile side
    uint64_t B = TS_BYTES_256M / (n * sizeof(double));
    B = B < CL_T ? CL_T : (B / CL_T) * CL_T;
    if (B > n) B = n;
    const uint64_t zb = (n * d * 8 + 255) & ~255ull, ib = (n * k * 4 + 255) & ~255ull, db = (n * k * 8 + 255) & ~255ull;
    void *p;
    PHK_TRY(phk_ws(ctx, WS_WIDE, zb + ib + db + phk_div_up(B, CL_T) * CL_T * n * 8, &p));
    double *d_z = (double *)p, *d_d2 = (double *)((char *)p + zb + ib), *d_rows = (double *)((char *)p + zb + ib + db);
    int32_t *d_idx = (int32_t *)((char *)p + zb);
    PHK_TRY(phk_copy_to_device(ctx, d_z, Z, n * d * 8));
    for (uint64_t q0 = 0; q0 < n; q0 += B) {
        const uint64_t nq = std::min(B, n - q0);
        // d_rows[q - q0][j] = s_qj for the query rows [q0, q0 + nq) of the batch (q0 is a multiple of the tile side) and every row j
        PHK_LAUNCH(ctx, "phk_ts_dist_kernel",
                   cl_matrix_kernel<TsStoreOffDiagonal>
                   <<<dim3((unsigned)phk_div_up(n, CL_T), (unsigned)phk_div_up(nq, CL_T)), dim3(CL_THREADS), 0, ctx->stream>>>(
                       d_z, q0 + nq, q0 / CL_T, d_z, n, d, d_rows, nullptr));
        PHK_LAUNCH(ctx, "phk_ts_select_kernel",
                   phk_ts_select_kernel<<<dim3((unsigned)nq), dim3(256), 0, ctx->stream>>>(d_rows, n, (uint32_t)k, kp, q0, d_idx,
                                                                                          d_d2));
    }
    PHK_TRY(phk_copy_to_host(ctx, idx, d_idx, n * k * 4));
    return phk_copy_to_host(ctx, d2, d_d2, n * k * 8);
}

// ---- conditional affinities --------------------------------------------------------------------------------------------
// scikit-learn's _binary_search_perplexity (sklearn/manifold/_utils.pyx), one thread per row: beta starts at 1, at most
// 100 steps, |H - log(perplexity)| <= 1e-5 ends the search, beta doubles / halves until both bounds exist, then bisects.
// The sums run over the neighbours in the order given.
__global__ __launch_bounds__(256) void phk_ts_affinity_kernel(const double *__restrict__ d2, uint64_t n, uint64_t k,
                                                             double desired_entropy, double *__restrict__ P,
                                                             double *__restrict__ beta_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *dr = d2 + i * k;
    double *pr = P + i * k;
    const double inf = __builtin_inf();
    double beta = 1.0, bmin = -inf, bmax = inf;
    for (int l = 0; l < 100; ++l) {
        double sum_p = 0.0;
        for (uint64_t j = 0; j < k; ++j) {
            const double p = exp(-dr[j] * beta);
            pr[j] = p;
            sum_p += p;
        }
        if (sum_p == 0.0) sum_p = 1e-8;
        double sdp = 0.0;
        for (uint64_t j = 0; j < k; ++j) {
            const double p = pr[j] / sum_p;
            pr[j] = p;
            sdp += dr[j] * p;
        }
        const double diff = log(sum_p) + beta * sdp - desired_entropy;
        if (fabs(diff) <= 1e-5) break;
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == inf ? beta * 2.0 : (beta + bmax) / 2.0;
        } else {
            bmax = beta;
            beta = bmin == -inf ? beta / 2.0 : (beta + bmin) / 2.0;
        }
    }
    beta_out[i] = beta;
}

extern "C" int phk_tsne_affinities(phk_ctx *ctx, const double *d2, uint64_t n, uint64_t k, double perplexity, double *P,
                                   double *beta) {
    PHK_ENTER(ctx, "phk_tsne_affinities");
    PHK_REQUIRE(d2 && P && beta, "phk_tsne_affinities: NULL pointer");
    PHK_REQUIRE(n >= 1 && k >= 1 && n < (1ull << 31), "phk_tsne_affinities: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)k);
    PHK_REQUIRE(perplexity > 0.0 && perplexity < __builtin_inf(), "phk_tsne_affinities: perplexity must be finite and > 0 (got %g)",
                perplexity);
    const uint64_t db = (n * k * 8 + 255) & ~255ull;
    void *p;
    PHK_TRY(phk_ws(ctx, WS_WIDE, 2 * db + n * 8, &p));
    double *d_d2 = (double *)p, *d_p = (double *)((char *)p + db), *d_beta = (double *)((char *)p + 2 * db);
    PHK_TRY(phk_copy_to_device(ctx, d_d2, d2, n * k * 8));
    PHK_LAUNCH(ctx, "phk_ts_affinity_kernel",
               phk_ts_affinity_kernel<<<dim3((unsigned)phk_div_up(n, 256)), dim3(256), 0, ctx->stream>>>(d_d2, n, k, std::log(perplexity),
                                                                                                       d_p, d_beta));
    PHK_TRY(phk_copy_to_host(ctx, P, d_p, n * k * 8));
    return phk_copy_to_host(ctx, beta, d_beta, n * 8);
}

// P = (P + P^T) / sum(P + P^T) over the union of the directed edges, as CSR with the columns of a row ascending.  The
// reverse adjacency is built once by a counting sort by target (sources ascending within a target), so every row gathers
// its incoming edges in a fixed order; the total is the sequential sum of the values in CSR order.  Host, O(n k log k).
extern "C" int phk_tsne_symmetrize(const int32_t *idx, const double *P, uint64_t n, uint64_t k, int64_t *indptr, int32_t *indices,
                                   double *values, uint64_t *nnz) {
    PHK_REQUIRE(idx && P && indptr && indices && values && nnz, "phk_tsne_symmetrize: NULL pointer");
    PHK_REQUIRE(n >= 1 && k >= 1 && n < (1ull << 31), "phk_tsne_symmetrize: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)k);
    std::vector<uint64_t> rptr(n + 1, 0);
    for (uint64_t e = 0; e < n * k; ++e) {
        PHK_REQUIRE(idx[e] >= 0 && (uint64_t)idx[e] < n, "phk_tsne_symmetrize: neighbour index %d is not a row", idx[e]);
        ++rptr[idx[e] + 1];
    }
    for (uint64_t j = 0; j < n; ++j) rptr[j + 1] += rptr[j];
    std::vector<int32_t> rsrc(n * k);
    std::vector<double> rval(n * k);
    {
        std::vector<uint64_t> at(rptr.begin(), rptr.end() - 1);
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t t = 0; t < k; ++t) {
                const uint64_t o = at[idx[i * k + t]]++;
                rsrc[o] = (int32_t)i;
                rval[o] = P[i * k + t];
            }
    }
    std::vector<std::pair<int32_t, double>> fwd(k);
    uint64_t m = 0;
    indptr[0] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        for (uint64_t t = 0; t < k; ++t) fwd[t] = std::make_pair(idx[i * k + t], P[i * k + t]);
        std::sort(fwd.begin(), fwd.end(), [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &b) {
            return a.first < b.first;
        });
        uint64_t a = 0, b = rptr[i];
        const uint64_t be = rptr[i + 1];
        while (a < k || b < be) {
            const int32_t ja = a < k ? fwd[a].first : INT32_MAX, jb = b < be ? rsrc[b] : INT32_MAX;
            const int32_t j = ja < jb ? ja : jb;
            double v = 0.0;
            if (ja == j) v += fwd[a++].second;
            if (jb == j) v += rval[b++];
            indices[m] = j;
            values[m] = v;
            ++m;
        }
        indptr[i + 1] = (int64_t)m;
    }
    double total = 0.0;
    for (uint64_t e = 0; e < m; ++e) total += values[e];
    if (total < TS_EPS) total = TS_EPS;
    for (uint64_t e = 0; e < m; ++e) values[e] /= total;
    *nnz = m;
    return PHK_OK;
}

// ---- gradient ----------------------------------------------------------------------------------------------------------
#define TS_T 256   // rows per workgroup = columns per LDS tile

// The repulsive sums of the rows [256 bx, 256 bx + 256) over the column tiles of range g = blockIdx.y (tiles
// [tiles g / G, tiles (g + 1) / G)): Z_i = sum_j w_ij, r_i = sum_j w_ij^2 (y_i - y_j), w_ij = 1 / (1 + |y_i - y_j|^2),
// j != i, in column order.  One thread per row; a tile of 256 points (4 KiB) is staged in LDS and read by broadcast.  The
// reciprocal is v_rcp_f64 refined by two Newton steps (full precision; 1 + |.|^2 >= 1, no scaling needed): one reciprocal
// and ~14 fp64 vector operations per pair.
__global__ __launch_bounds__(TS_T) void phk_ts_repulse_kernel(const double2 *__restrict__ Y, uint64_t n, uint32_t G, uint64_t tiles,
                                                             double *__restrict__ pz, double *__restrict__ prx,
                                                             double *__restrict__ pry) {
    __shared__ double2 S[TS_T];
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * TS_T + t;
    const uint32_t g = blockIdx.y;
    const double2 yi = i < n ? Y[i] : make_double2(0.0, 0.0);
    const uint64_t t0 = tiles * g / G, t1 = tiles * (g + 1) / G;
    double z = 0.0, rx = 0.0, ry = 0.0;
    for (uint64_t T = t0; T < t1; ++T) {
        const uint64_t cbase = T * TS_T;
        __syncthreads();
        S[t] = cbase + t < n ? Y[cbase + t] : make_double2(0.0, 0.0);
        __syncthreads();
        const int cnt = (int)(n - cbase < TS_T ? n - cbase : TS_T);
        const int self = (i >= cbase && i < cbase + TS_T) ? (int)(i - cbase) : -1;
        for (int c = 0; c < cnt; ++c) {
            const double2 yj = S[c];
            const double dx = yi.x - yj.x, dy = yi.y - yj.y;
            const double a = fma(dx, dx, fma(dy, dy, 1.0));
            double w = __builtin_amdgcn_rcp(a);
            w = fma(w, fma(-a, w, 1.0), w);
            w = fma(w, fma(-a, w, 1.0), w);
            w = c == self ? 0.0 : w;
            const double w2 = w * w;
            z += w;
            rx = fma(w2, dx, rx);
            ry = fma(w2, dy, ry);
        }
    }
    if (i < n) {
        pz[(uint64_t)g * n + i] = z;
        prx[(uint64_t)g * n + i] = rx;
        pry[(uint64_t)g * n + i] = ry;
    }
}

// folds a row's partials in range order: R[i] = r_i, and bz[block] = the block's sum of Z_i (fixed tree)
__global__ __launch_bounds__(256) void phk_ts_fold_kernel(const double *__restrict__ pz, const double *__restrict__ prx,
                                                         const double *__restrict__ pry, uint64_t n, uint32_t G,
                                                         double2 *__restrict__ R, double *__restrict__ bz) {
    __shared__ double sh[256];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double z = 0.0, rx = 0.0, ry = 0.0;
    if (i < n) {
        for (uint32_t g = 0; g < G; ++g) {
            z += pz[(uint64_t)g * n + i];
            rx += prx[(uint64_t)g * n + i];
            ry += pry[(uint64_t)g * n + i];
        }
        R[i] = make_double2(rx, ry);
    }
    z = ts_block_sum(z, sh);
    if (threadIdx.x == 0) bz[blockIdx.x] = z;
}

// One thread per row: the attractive sum over the row's CSR entries (in their order), grad_i = 4 (attr_i - r_i / Z), and
//   step != 0: scikit-learn's _gradient_descent update -- gains +0.2 where update and gradient differ in sign, else x 0.8,
//              floored at min_gain; update = momentum update - learning_rate gains grad; Ynew = Y + update
//   step == 0: grad_out[i] = grad_i
// With `check`, bkl[block] = the block's sum of p log(max(p, eps) / max(q, eps)), q = w / Z, over its rows' entries and
// bgn[block] = its sum of |gains grad|^2.  scal[0] = Z.
__global__ __launch_bounds__(256) void phk_ts_update_kernel(const double2 *__restrict__ Y, double2 *__restrict__ Ynew,
                                                           const double2 *__restrict__ R, const double *__restrict__ scal,
                                                           const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                           const double *__restrict__ values, double exaggeration, uint64_t n,
                                                           int step, double momentum, double learning_rate, double min_gain,
                                                           double2 *__restrict__ upd, double2 *__restrict__ gains,
                                                           double2 *__restrict__ grad_out, int check, double *__restrict__ bkl,
                                                           double *__restrict__ bgn) {
    __shared__ double sh[256];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const double Z = scal[0];
    double kl = 0.0, gn = 0.0;
    if (i < n) {
        const double2 yi = Y[i];
        double ax = 0.0, ay = 0.0;
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
            const double2 yj = Y[indices[e]];
            const double p = values[e] * exaggeration;
            const double dx = yi.x - yj.x, dy = yi.y - yj.y;
            const double w = 1.0 / fma(dx, dx, fma(dy, dy, 1.0));
            const double pw = p * w;
            ax = fma(pw, dx, ax);
            ay = fma(pw, dy, ay);
            if (check) kl += p * log(fmax(p, TS_EPS) / fmax(w / Z, TS_EPS));
        }
        const double2 r = R[i];
        const double gx = 4.0 * (ax - r.x / Z), gy = 4.0 * (ay - r.y / Z);
        if (step) {
            const double2 u = upd[i];
            double2 gg = gains[i];
            gg.x = u.x * gx < 0.0 ? gg.x + 0.2 : gg.x * 0.8;
            gg.y = u.y * gy < 0.0 ? gg.y + 0.2 : gg.y * 0.8;
            gg.x = fmax(gg.x, min_gain);
            gg.y = fmax(gg.y, min_gain);
            const double sx = gx * gg.x, sy = gy * gg.y;
            const double2 un = make_double2(momentum * u.x - learning_rate * sx, momentum * u.y - learning_rate * sy);
            gains[i] = gg;
            upd[i] = un;
            Ynew[i] = make_double2(yi.x + un.x, yi.y + un.y);
            gn = fma(sx, sx, sy * sy);
        } else {
            grad_out[i] = make_double2(gx, gy);
        }
    }
    if (check) {
        kl = ts_block_sum(kl, sh);
        gn = ts_block_sum(gn, sh);
        if (threadIdx.x == 0) {
            bkl[blockIdx.x] = kl;
            bgn[blockIdx.x] = gn;
        }
    }
}

__global__ __launch_bounds__(256) void phk_ts_fill_kernel(double *__restrict__ p, uint64_t m, double v) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) p[i] = v;
}

// the device side of a gradient / descent call: one workspace, carved
struct TsDev {
    uint64_t n = 0, nb = 0, tiles = 0;
    uint32_t G = 1;
    double2 *Y[2] = {nullptr, nullptr}, *R = nullptr, *upd = nullptr, *gains = nullptr, *grad = nullptr;
    double *pz = nullptr, *prx = nullptr, *pry = nullptr, *bz = nullptr, *bkl = nullptr, *bgn = nullptr, *scal = nullptr;
    int64_t *indptr = nullptr;
    int32_t *indices = nullptr;
    double *values = nullptr;
    int cur = 0;
};

// column ranges per row block: enough workgroups (~2048) to fill the chip at small n -- a function of n only
static uint32_t ts_ranges(uint64_t tiles) {
    const uint64_t g = std::max<uint64_t>(1, phk_div_up(2048, tiles));
    return (uint32_t)std::min<uint64_t>(g, tiles);
}

static int ts_setup(phk_ctx *ctx, const char *fname, const double *Y, uint64_t n, const int64_t *indptr, const int32_t *indices,
                    const double *values, TsDev *d) {
    PHK_REQUIRE(Y && indptr && indices && values, "%s: NULL pointer", fname);
    PHK_REQUIRE(n >= 2 && n < (1ull << 31), "%s: bad number of rows (%llu)", fname, (unsigned long long)n);
    PHK_REQUIRE(indptr[0] == 0, "%s: indptr[0] must be 0", fname);
    for (uint64_t i = 0; i < n; ++i) PHK_REQUIRE(indptr[i + 1] >= indptr[i], "%s: indptr must not decrease", fname);
    const uint64_t nnz = (uint64_t)indptr[n];
    for (uint64_t e = 0; e < nnz; ++e)
        PHK_REQUIRE(indices[e] >= 0 && (uint64_t)indices[e] < n, "%s: column index %d is not a row", fname, indices[e]);
    d->n = n;
    d->nb = phk_div_up(n, 256);
    d->tiles = phk_div_up(n, TS_T);
    d->G = ts_ranges(d->tiles);
    auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
    const uint64_t yb = al(n * 16), pb = al((uint64_t)d->G * n * 8), bb = al(d->nb * 8), ipb = al((n + 1) * 8), ixb = al(nnz * 4),
                   vb = al(nnz * 8);
    void *p;
    PHK_TRY(phk_ws(ctx, WS_WIDE, 6 * yb + 3 * pb + 3 * bb + 256 + ipb + ixb + vb, &p));
    char *c = (char *)p;
    auto take = [&c](uint64_t b) {
        char *r = c;
        c += b;
        return (void *)r;
    };
    d->Y[0] = (double2 *)take(yb);
    d->Y[1] = (double2 *)take(yb);
    d->R = (double2 *)take(yb);
    d->upd = (double2 *)take(yb);
    d->gains = (double2 *)take(yb);
    d->grad = (double2 *)take(yb);
    d->pz = (double *)take(pb);
    d->prx = (double *)take(pb);
    d->pry = (double *)take(pb);
    d->bz = (double *)take(bb);
    d->bkl = (double *)take(bb);
    d->bgn = (double *)take(bb);
    d->scal = (double *)take(256);
    d->indptr = (int64_t *)take(ipb);
    d->indices = (int32_t *)take(ixb);
    d->values = (double *)take(vb);
    d->cur = 0;
    PHK_TRY(phk_copy_to_device(ctx, d->Y[0], Y, n * 16));
    PHK_TRY(phk_copy_to_device(ctx, d->indptr, indptr, (n + 1) * 8));
    PHK_TRY(phk_copy_to_device(ctx, d->indices, indices, nnz * 4));
    PHK_TRY(phk_copy_to_device(ctx, d->values, values, nnz * 8));
    return PHK_OK;
}

// one evaluation of the gradient at Y[cur]; step: the update into Y[cur ^ 1] (the caller flips cur); check: scal[1] = KL,
// scal[2] = |gains grad|^2 afterwards
static int ts_iterate(phk_ctx *ctx, TsDev *d, double exaggeration, int step, double momentum, double learning_rate, double min_gain,
                      int check) {
    const uint64_t n = d->n;
    const unsigned nb = (unsigned)d->nb;
    PHK_LAUNCH(ctx, "phk_ts_repulse_kernel",
               phk_ts_repulse_kernel<<<dim3((unsigned)d->tiles, d->G), dim3(TS_T), 0, ctx->stream>>>(d->Y[d->cur], n, d->G, d->tiles,
                                                                                                    d->pz, d->prx, d->pry));
    PHK_LAUNCH(ctx, "phk_ts_fold_kernel",
               phk_ts_fold_kernel<<<dim3(nb), dim3(256), 0, ctx->stream>>>(d->pz, d->prx, d->pry, n, d->G, d->R, d->bz));
    PHK_LAUNCH(ctx, "phk_ts_total_kernel", phk_ts_total_kernel<<<dim3(1), dim3(256), 0, ctx->stream>>>(d->bz, d->nb, 0, d->scal));
    PHK_LAUNCH(ctx, "phk_ts_update_kernel",
               phk_ts_update_kernel<<<dim3(nb), dim3(256), 0, ctx->stream>>>(d->Y[d->cur], d->Y[d->cur ^ 1], d->R, d->scal, d->indptr,
                                                                           d->indices, d->values, exaggeration, n, step, momentum,
                                                                           learning_rate, min_gain, d->upd, d->gains, d->grad, check,
                                                                           d->bkl, d->bgn));
    if (check) {
        // bkl and bgn lie one after the other (stride = their distance): scal[1], scal[2]
        PHK_LAUNCH(ctx, "phk_ts_total_kernel",
                   phk_ts_total_kernel<<<dim3(2), dim3(256), 0, ctx->stream>>>(d->bkl, d->nb, (uint64_t)(d->bgn - d->bkl), d->scal + 1));
    }
    return PHK_OK;
}

// scikit-learn's _gradient_descent (sklearn/manifold/_t_sne.py) from iteration `it` to max_iter: update and gains start at
// 0 and 1; every n_check-th iteration the host reads (KL, |gains grad|^2) -- two doubles -- and decides.
static int ts_descent(phk_ctx *ctx, TsDev *d, double exaggeration, double momentum, double learning_rate, double min_gain,
                      uint64_t it, uint64_t max_iter, uint64_t n_check, uint64_t n_iter_without_progress, double min_grad_norm,
                      double *error_out, uint64_t *it_out) {
    const uint64_t m = d->n * 2;
    PHK_HIP(hipMemsetAsync(d->upd, 0, m * 8, ctx->stream));
    PHK_LAUNCH(ctx, "phk_ts_fill_kernel",
               phk_ts_fill_kernel<<<dim3((unsigned)phk_div_up(m, 256)), dim3(256), 0, ctx->stream>>>((double *)d->gains, m, 1.0));
    double error = DBL_MAX, best = DBL_MAX;
    uint64_t best_iter = it, i = it;
    for (uint64_t j = it; j < max_iter; ++j) {
        i = j;
        const bool check = (j + 1) % n_check == 0;
        const bool want = check || j == max_iter - 1;
        PHK_TRY(ts_iterate(ctx, d, exaggeration, 1, momentum, learning_rate, min_gain, want ? 1 : 0));
        d->cur ^= 1;
        if (want) {
            double two[2];
            PHK_HIP(hipMemcpyAsync(two, d->scal + 1, 16, hipMemcpyDeviceToHost, ctx->stream));
            PHK_HIP(hipStreamSynchronize(ctx->stream));
            error = two[0];
            if (check) {
                const double grad_norm = std::sqrt(two[1]);
                if (error < best) {
                    best = error;
                    best_iter = j;
                } else if (j - best_iter > n_iter_without_progress) {
                    break;
                }
                if (grad_norm <= min_grad_norm) break;
            }
        }
    }
    *error_out = error;
    *it_out = i;
    return PHK_OK;
}

extern "C" int phk_tsne_gradient(phk_ctx *ctx, const double *Y, uint64_t n, const int64_t *indptr, const int32_t *indices,
                                 const double *values, double exaggeration, double *kl, double *grad) {
    PHK_ENTER(ctx, "phk_tsne_gradient");
    PHK_REQUIRE(kl && grad, "phk_tsne_gradient: NULL pointer");
    TsDev d;
    PHK_TRY(ts_setup(ctx, "phk_tsne_gradient", Y, n, indptr, indices, values, &d));
    PHK_TRY(ts_iterate(ctx, &d, exaggeration, 0, 0.0, 0.0, 0.0, 1));
    PHK_TRY(phk_copy_to_host(ctx, kl, d.scal + 1, 8));
    return phk_copy_to_host(ctx, grad, d.grad, n * 16);
}

extern "C" int phk_tsne_descend(phk_ctx *ctx, double *Y, uint64_t n, const int64_t *indptr, const int32_t *indices,
                                const double *values, double exaggeration, double momentum, double learning_rate, double min_gain,
                                uint64_t n_steps, double *kl) {
    PHK_ENTER(ctx, "phk_tsne_descend");
    TsDev d;
    PHK_TRY(ts_setup(ctx, "phk_tsne_descend", Y, n, indptr, indices, values, &d));
    double error = 0.0;
    uint64_t it = 0;
    PHK_TRY(ts_descent(ctx, &d, exaggeration, momentum, learning_rate, min_gain, 0, n_steps, ~0ull, ~0ull, 0.0, &error, &it));
    if (kl) *kl = error;
    return phk_copy_to_host(ctx, Y, d.Y[d.cur], n * 16);
}

// TSNE._tsne: 250 iterations at momentum 0.5 with P x early_exaggeration (n_iter_without_progress 250), then up to max_iter
// at momentum 0.8 with P itself; min_gain 0.01, a check every 50 iterations.
extern "C" int phk_tsne_fit(phk_ctx *ctx, double *Y, uint64_t n, const int64_t *indptr, const int32_t *indices, const double *values,
                            double early_exaggeration, double learning_rate, uint64_t max_iter, uint64_t n_iter_without_progress,
                            double min_grad_norm, double *kl, uint64_t *n_iter) {
    PHK_ENTER(ctx, "phk_tsne_fit");
    PHK_REQUIRE(kl && n_iter, "phk_tsne_fit: NULL pointer");
    PHK_REQUIRE(max_iter >= 250, "phk_tsne_fit: max_iter must be at least 250 (got %llu)", (unsigned long long)max_iter);
    TsDev d;
    PHK_TRY(ts_setup(ctx, "phk_tsne_fit", Y, n, indptr, indices, values, &d));
    const uint64_t explore = 250;
    double error = 0.0;
    uint64_t it = 0;
    PHK_TRY(ts_descent(ctx, &d, early_exaggeration, 0.5, learning_rate, 0.01, 0, explore, 50, explore, min_grad_norm, &error, &it));
    if (it < explore || max_iter > explore)
        PHK_TRY(ts_descent(ctx, &d, 1.0, 0.8, learning_rate, 0.01, it + 1, max_iter, 50, n_iter_without_progress, min_grad_norm, &error,
                           &it));
    *kl = error;
    *n_iter = it;
    return phk_copy_to_host(ctx, Y, d.Y[d.cur], n * 16);
}
