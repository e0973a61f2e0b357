// hosts.hip -- likelihood-ranked reference lookup (gfx950): this project's own, DESIGN.md 4.21.
//
// likelihood.hip reduces S[q, r] = sum_j c_q[j] L[r, j] to one number per class; here the same product answers "which
// reference rows is the contig most likely to come from": the first `top` rows of every query in order of (S descending,
// row index ascending), with their S.  L is a log table built on the host -- the multinomial one of likelihood.py or the
// Markov one of hosts.py (log transition probabilities: S is then the log-likelihood of the contig's transitions under row
// r's chain) -- and the device does not know which.  S is what the shared Gram tile (gram_tile.h, uint32 A operand) gives
// for the pair, so the bits of a result do not depend on N, the batch split, the entry point or the run.
//
// Route, the one neighbors.hip proves: workgroup (chunk of GT_CHUNK rows, block of GT_QB queries); per row step the
// 128 x 64 tile of S goes through LDS, thread (query, half) scans its 32 rows of the step into a register list of T entries
// behind a "better than my worst" test, insertion by compare-exchange with static indices (nn_insert, row_list.h); the two
// halves of a query meet through LDS and phk_host_merge_kernel folds a query's chunks in chunk order.  The lists hold -S
// (exact), so that the neighbour lookup's ascending order (value, j) is (S descending, j ascending); that order is total,
// so the list a query ends with is the same whatever order its rows arrived in.  Rows past the chunk and excluded pairs
// (both group ids >= 0 and equal) enter the tile as NaN, which passes no test.
//
// The null of the z-score (hosts.fit_null): per reference row the mean and the sample standard deviation of
// l[p, r] = S[p, r] / n_p over the null rows p, in two passes over the product: phk_host_pairs_kernel writes l of a block of
// null rows, phk_host_column_kernel (one thread per column r) continues the running sum (pass 1) or the centred square sum
// (pass 2) in row order 0..P-1 -- the bits do not depend on the batch split.
#include <algorithm>

#include "density_shared.h"
#include "gram_tile.h"
#include "row_list.h"

#define HT_MAX_TOP PHK_HOSTS_MAX_TOP

// grid: x = chunk of GT_CHUNK rows of [0, M), y = block of GT_QB queries.  LDS: the step's tile, 64 KiB, entry (row, query)
// at column query ^ 4 (row & 15) as in phk_nn_partial_kernel.  pv / pj[chunk][query][T]: -S and row index, (+inf, NN_NOROW)
// where the chunk had fewer rows for the query.
template <bool FULL, int T>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_host_rank_kernel(
    const uint32_t *__restrict__ C, const int32_t *__restrict__ qg, uint64_t nq, const double *__restrict__ L,
    const int32_t *__restrict__ rg, uint64_t M, uint64_t D, double *__restrict__ pv, int32_t *__restrict__ pj) {
    __shared__ double tile[NN_STEP * GT_QB];
    const int li = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x;
    const uint64_t r0 = (uint64_t)c * GT_CHUNK;
    const uint64_t r1 = r0 + GT_CHUNK < M ? r0 + GT_CHUNK : M;
    const uint64_t q0 = (uint64_t)blockIdx.y * GT_QB + (uint64_t)wave * (GT_QT * 16);
    const int myq = threadIdx.x & (GT_QB - 1), half = threadIdx.x >> 7;

    int32_t qgrp[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = gram_query(q0, a, r);
            qgrp[a][r] = (qg && q < nq) ? qg[q] : -1;
        }
    double lv[T];
    int32_t lj[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        lv[i] = __builtin_inf();
        lj[i] = NN_NOROW;
    }

    for (uint64_t st = r0; st < r1; st += NN_STEP) {
        f64x4 acc[GT_QT][GT_RT];
        gram_tile<FULL, GT_QT, uint32_t>(C, nq, q0, L, r1, st, D, acc);
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const int row = 16 * t + li;
            const uint64_t j = st + row;
            const bool inside = j < r1;
            const int32_t rgj = (inside && rg) ? rg[j] : -1;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ql = wave * (GT_QT * 16) + 16 * a + kk + 4 * r;
                    const bool keep = inside && !(rgj >= 0 && rgj == qgrp[a][r]);
                    tile[row * GT_QB + (ql ^ (li << 2))] = keep ? -acc[a][t][r] : __builtin_nan("");
                }
        }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < NN_STEP / 2; ++i) {
            const int row = half * (NN_STEP / 2) + i;
            const double v = tile[row * GT_QB + (myq ^ ((row & 15) << 2))];
            const int32_t j = (int32_t)(st + row);
            if (nn_less(v, j, lv[T - 1], lj[T - 1])) nn_insert<T>(lv, lj, v, j);
        }
        __syncthreads();
    }
    // the upper half's lists -> LDS ([entry][query]: 12 T GT_QB bytes <= 24 KiB), the lower half takes them in, in order
    double *sv = tile;
    int32_t *sj = (int32_t *)(tile + T * GT_QB);
    if (half) {
#pragma unroll
        for (int i = 0; i < T; ++i) {
            sv[i * GT_QB + myq] = lv[i];
            sj[i * GT_QB + myq] = lj[i];
        }
    }
    __syncthreads();
    if (half) return;
#pragma unroll 1
    for (int i = 0; i < T; ++i) {
        const double v = sv[i * GT_QB + myq];
        const int32_t j = sj[i * GT_QB + myq];
        if (!nn_less(v, j, lv[T - 1], lj[T - 1])) break;   // (sorted: no later entry gets in either)
        nn_insert<T>(lv, lj, v, j);
    }
    const uint64_t q = (uint64_t)blockIdx.y * GT_QB + myq;
    if (q < nq) {
        const uint64_t o = ((uint64_t)c * nq + q) * T;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            pv[o + i] = lv[i];
            pj[o + i] = lj[i];
        }
    }
}

// one thread per query: the chunks' lists in chunk order into the query's list; its first `top` entries go to
// out_s / out_idx[q][top] (q counted from the batch's first query), the values as S again
template <int T>
__global__ __launch_bounds__(256) void phk_host_merge_kernel(const double *__restrict__ pv, const int32_t *__restrict__ pj,
                                                             uint64_t nq, uint32_t S, int top, double *__restrict__ out_s,
                                                             int32_t *__restrict__ out_idx) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    double lv[T];
    int32_t lj[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        lv[i] = __builtin_inf();
        lj[i] = NN_NOROW;
    }
    for (uint32_t c = 0; c < S; ++c) {
        const uint64_t o = ((uint64_t)c * nq + q) * T;
#pragma unroll 1
        for (int i = 0; i < T; ++i) {
            const double v = pv[o + i];
            const int32_t j = pj[o + i];
            if (!nn_less(v, j, lv[T - 1], lj[T - 1])) break;
            nn_insert<T>(lv, lj, v, j);
        }
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
        if (i < top) {
            out_s[q * top + i] = -lv[i];
            out_idx[q * top + i] = lj[i];
        }
}

// grid as the rank kernel's.  ell[p][r] = S[p, r] / n[p] for the nq null rows C (totals n, all > 0) against all M rows.
template <bool FULL>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_host_pairs_kernel(const uint32_t *__restrict__ C,
                                                                          const double *__restrict__ n, uint64_t nq,
                                                                          const double *__restrict__ L, uint64_t M, uint64_t D,
                                                                          double *__restrict__ ell) {
    const int li = threadIdx.x & 15, wave = threadIdx.x >> 6;
    const uint64_t r0 = (uint64_t)blockIdx.x * GT_CHUNK;
    const uint64_t r1 = r0 + GT_CHUNK < M ? r0 + GT_CHUNK : M;
    const uint64_t q0 = (uint64_t)blockIdx.y * GT_QB + (uint64_t)wave * (GT_QT * 16);
    double nk[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = gram_query(q0, a, r);
            nk[a][r] = q < nq ? n[q] : 1.0;
        }
    for (uint64_t st = r0; st < r1; st += NN_STEP) {
        f64x4 acc[GT_QT][GT_RT];
        gram_tile<FULL, GT_QT, uint32_t>(C, nq, q0, L, r1, st, D, acc);
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint64_t j = st + 16 * t + li;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint64_t q = gram_query(q0, a, r);
                    if (j < r1 && q < nq) ell[q * M + j] = acc[a][t][r] / nk[a][r];
                }
        }
    }
}

// one thread per column r: acc[r] continued over the nb rows of ell in row order -- pass 1: acc += l; pass 2:
// acc = fma(l - mu, l - mu, acc).  last: the pass ends with this block -- pass 1: mu[r] = acc / P; pass 2:
// sigma[r] = sqrt(acc / (P - 1)).
__global__ __launch_bounds__(256) void phk_host_column_kernel(const double *__restrict__ ell, uint64_t nb, uint64_t M, int pass,
                                                              int last, double P, double *__restrict__ acc,
                                                              double *__restrict__ mu, double *__restrict__ sigma) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    double s = acc[r];
    if (pass == 1) {
        for (uint64_t p = 0; p < nb; ++p) s += ell[p * M + r];
    } else {
        const double m = mu[r];
        for (uint64_t p = 0; p < nb; ++p) {
            const double d = ell[p * M + r] - m;
            s = fma(d, d, s);
        }
    }
    acc[r] = s;
    if (last) {
        if (pass == 1)
            mu[r] = s / P;
        else
            sigma[r] = sqrt(s / (P - 1.0));
    }
}

// ---- the resident table ------------------------------------------------------------------------------------------------
struct phk_host_table {
    uint64_t M = 0, D = 0;
    PhkDevMem logp;                // [M][D] float64
    PhkDevMem groups;              // [M] int32, or empty
    std::vector<int32_t> gsorted;  // the non-negative group ids, sorted (host): the rows a query has left
};

extern "C" int phk_host_table_create(phk_ctx *ctx, const double *log_table, uint64_t M, uint64_t D, const int32_t *groups,
                                     phk_host_table **out) {
    PHK_ENTER(ctx, "phk_host_table_create");
    PHK_REQUIRE(out, "phk_host_table_create: NULL out");
    *out = nullptr;
    PHK_REQUIRE(D > 0 && M > 0 && log_table, "phk_host_table_create: no reference rows");
    PHK_REQUIRE(M < (1ull << 31) && D < (1ull << 32), "phk_host_table_create: table too large");
    if (!phk_rows_finite(log_table, M * D)) {
        phk_set_error("phk_host_table_create: the log table holds a value that is not finite (a zero profile entry?)");
        return PHK_ERR_NAN;
    }
    phk_host_table *t = new phk_host_table();
    t->M = M, t->D = D;
    int rc = t->logp.alloc("phk_host_table_create", "log table", M * D * sizeof(double));
    if (rc == PHK_OK) rc = phk_copy_to_device(ctx, t->logp.ptr, log_table, M * D * sizeof(double));
    if (rc == PHK_OK && groups) {
        for (uint64_t i = 0; i < M; ++i)
            if (groups[i] >= 0) t->gsorted.push_back(groups[i]);
        std::sort(t->gsorted.begin(), t->gsorted.end());
        rc = t->groups.alloc("phk_host_table_create", "group ids", M * sizeof(int32_t));
        if (rc == PHK_OK && hipMemcpy(t->groups.ptr, groups, M * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            phk_set_error("phk_host_table_create: upload of the group ids failed");
            rc = PHK_ERR_HIP;
        }
    }
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        phk_set_error("phk_host_table_create: upload failed");
        rc = PHK_ERR_HIP;
    }
    if (rc != PHK_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return PHK_OK;
}

extern "C" int phk_host_table_destroy(phk_ctx *ctx, phk_host_table *t) {
    if (!t) return PHK_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete t;
    return PHK_OK;
}

static inline uint64_t ht_up256(uint64_t b) { return (b + 255) & ~255ull; }

template <int T>
static int ht_launch(phk_ctx *ctx, const uint32_t *d_c, const int32_t *d_qg, uint64_t nb, const double *d_L,
                     const int32_t *d_rg, uint64_t M, uint64_t D, uint32_t S, int top, double *pv, int32_t *pj, double *out_s,
                     int32_t *out_idx) {
    const dim3 grid(S, (unsigned)phk_div_up(nb, GT_QB));
    if (D % GT_KC == 0) {
        PHK_LAUNCH(ctx, "phk_host_rank_kernel", phk_host_rank_kernel<true, T><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                                                    d_c, d_qg, nb, d_L, d_rg, M, D, pv, pj));
    } else {
        PHK_LAUNCH(ctx, "phk_host_rank_kernel", phk_host_rank_kernel<false, T><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                                                    d_c, d_qg, nb, d_L, d_rg, M, D, pv, pj));
    }
    PHK_LAUNCH(ctx, "phk_host_merge_kernel",
               phk_host_merge_kernel<T><<<dim3((unsigned)phk_div_up(nb, 256)), dim3(256), 0, ctx->stream>>>(pv, pj, nb, S, top,
                                                                                                          out_s, out_idx));
    return PHK_OK;
}

// The ranking loop of both entries: count rows d_counts[N][D] on the device, host group ids (or NULL); idx[N][top] and
// s[N][top] go to the host arrays.  Queries run in batches of B against all S chunks, B as in lik_run: the partial lists
// within 256 MiB, a multiple of the query block, at most 2^20 (force_B != 0: that many, rounded up to the query block).
static int ht_run(phk_ctx *ctx, const char *fname, const phk_host_table *t, const uint32_t *d_counts, uint64_t N,
                  const int32_t *query_groups, int top, uint64_t force_B, int32_t *idx, double *s) {
    const uint64_t M = t->M, D = t->D;
    PHK_REQUIRE(top >= 1 && top <= HT_MAX_TOP, "%s: top = %d is not in 1..%d", fname, top, HT_MAX_TOP);
    PHK_REQUIRE((uint64_t)top <= M, "%s: top = %d exceeds the %llu reference rows", fname, top, (unsigned long long)M);
    const bool grouped = query_groups && t->groups.ptr;
    if (grouped) {   // the rows every query has left, known from the group histogram before any launch
        for (uint64_t q = 0; q < N; ++q) {
            if (query_groups[q] < 0) continue;
            const auto range = std::equal_range(t->gsorted.begin(), t->gsorted.end(), query_groups[q]);
            const uint64_t left = M - (uint64_t)(range.second - range.first);
            PHK_REQUIRE((uint64_t)top <= left, "%s: top = %d exceeds the %llu reference rows query %llu (group %d) has left",
                        fname, top, (unsigned long long)left, (unsigned long long)q, (int)query_groups[q]);
        }
    }
    const int T = top <= 8 ? 8 : 16;
    const uint32_t S = (uint32_t)phk_div_up(M, GT_CHUNK);
    uint64_t B = (256ull << 20) / ((uint64_t)S * T * 12);
    B = B > (1ull << 20) ? (1ull << 20) : B;
    B = B < GT_QB ? GT_QB : (B / GT_QB) * GT_QB;
    if (force_B) B = phk_div_up(force_B, GT_QB) * GT_QB;
    if (B > N) B = N;
    void *part, *d_out, *d_q = nullptr;
    PHK_TRY(phk_ws(ctx, WS_KDE, ht_up256((uint64_t)S * B * T * 8) + (uint64_t)S * B * T * 4, &part));
    PHK_TRY(phk_ws(ctx, WS_OUT, ht_up256(N * top * 8) + N * top * 4, &d_out));
    double *pv = (double *)part;
    int32_t *pj = (int32_t *)((char *)part + ht_up256((uint64_t)S * B * T * 8));
    double *d_s = (double *)d_out;
    int32_t *d_idx = (int32_t *)((char *)d_out + ht_up256(N * top * 8));
    const int32_t *d_qg = nullptr;
    if (grouped) {
        PHK_TRY(phk_ws(ctx, WS_SUB, N * sizeof(int32_t), &d_q));
        PHK_TRY(phk_copy_to_device(ctx, d_q, query_groups, N * sizeof(int32_t)));
        d_qg = (const int32_t *)d_q;
    }
    const double *d_L = t->logp.as<double>();
    const int32_t *d_rg = grouped ? t->groups.as<int32_t>() : nullptr;
    for (uint64_t b = 0; b < N; b += B) {
        const uint64_t nb = N - b < B ? N - b : B;
        const uint32_t *c = d_counts + b * D;
        const int32_t *g = d_qg ? d_qg + b : nullptr;
        if (T == 8)
            PHK_TRY(ht_launch<8>(ctx, c, g, nb, d_L, d_rg, M, D, S, top, pv, pj, d_s + b * top, d_idx + b * top));
        else
            PHK_TRY(ht_launch<16>(ctx, c, g, nb, d_L, d_rg, M, D, S, top, pv, pj, d_s + b * top, d_idx + b * top));
    }
    PHK_TRY(phk_copy_to_host(ctx, idx, d_idx, N * top * sizeof(int32_t)));
    return phk_copy_to_host(ctx, s, d_s, N * top * sizeof(double));
}

extern "C" int phk_host_rank(phk_ctx *ctx, const phk_host_table *t, const uint32_t *counts, uint64_t N, uint64_t D,
                             const int32_t *query_groups, int top, uint64_t batch_rows, int32_t *idx, double *s) {
    PHK_ENTER(ctx, "phk_host_rank");
    PHK_REQUIRE(t, "phk_host_rank: NULL table");
    PHK_REQUIRE(D == t->D, "phk_host_rank: the counts have %llu columns, the table %llu", (unsigned long long)D,
                (unsigned long long)t->D);
    if (N == 0) return PHK_OK;
    PHK_REQUIRE(counts && idx && s, "phk_host_rank: NULL pointer");
    void *d_c;
    PHK_TRY(phk_ws(ctx, WS_COUNTS, N * D * sizeof(uint32_t), &d_c));
    PHK_TRY(phk_copy_to_device(ctx, d_c, counts, N * D * sizeof(uint32_t)));
    return ht_run(ctx, "phk_host_rank", t, (const uint32_t *)d_c, N, query_groups, top, batch_rows, idx, s);
}

extern "C" int phk_batch_host_rank(phk_ctx *ctx, const phk_host_table *t, const phk_batch *b, int top, int32_t *idx,
                                   double *s) {
    PHK_ENTER(ctx, "phk_batch_host_rank");
    PHK_REQUIRE(t && b, "phk_batch_host_rank: NULL table/batch");
    PHK_REQUIRE(b->D == t->D, "phk_batch_host_rank: the batch has %llu columns, the table %llu", (unsigned long long)b->D,
                (unsigned long long)t->D);
    if (b->n == 0) return PHK_OK;
    PHK_REQUIRE(idx && s, "phk_batch_host_rank: NULL pointer");
    return ht_run(ctx, "phk_batch_host_rank", t, b->d_counts, b->n, nullptr, top, 0, idx, s);
}

extern "C" int phk_host_null_fit(phk_ctx *ctx, const phk_host_table *t, const uint32_t *counts, uint64_t P, uint64_t D,
                                 uint64_t batch_rows, double *mu, double *sigma) {
    PHK_ENTER(ctx, "phk_host_null_fit");
    PHK_REQUIRE(t, "phk_host_null_fit: NULL table");
    PHK_REQUIRE(D == t->D, "phk_host_null_fit: the counts have %llu columns, the table %llu", (unsigned long long)D,
                (unsigned long long)t->D);
    PHK_REQUIRE(P >= 2, "phk_host_null_fit: a standard deviation needs at least 2 null rows, got %llu", (unsigned long long)P);
    PHK_REQUIRE(counts && mu && sigma, "phk_host_null_fit: NULL pointer");
    const uint64_t M = t->M;
    std::vector<double> n(P);
    for (uint64_t p = 0; p < P; ++p) {
        uint64_t sum = 0;
        for (uint64_t j = 0; j < D; ++j) sum += counts[p * D + j];
        PHK_REQUIRE(sum > 0, "phk_host_null_fit: null row %llu has no counts", (unsigned long long)p);
        n[p] = (double)sum;
    }
    uint64_t B = (256ull << 20) / (M * sizeof(double));
    B = B < GT_QB ? GT_QB : (B / GT_QB) * GT_QB;
    if (batch_rows) B = phk_div_up(batch_rows, GT_QB) * GT_QB;
    if (B > P) B = P;
    void *d_c, *d_n, *d_ell, *d_o;
    PHK_TRY(phk_ws(ctx, WS_COUNTS, P * D * sizeof(uint32_t), &d_c));
    PHK_TRY(phk_ws(ctx, WS_SUB, P * sizeof(double), &d_n));
    PHK_TRY(phk_ws(ctx, WS_DIST, B * M * sizeof(double), &d_ell));
    PHK_TRY(phk_ws(ctx, WS_OUT, 3 * M * sizeof(double), &d_o));
    PHK_TRY(phk_copy_to_device(ctx, d_c, counts, P * D * sizeof(uint32_t)));
    PHK_TRY(phk_copy_to_device(ctx, d_n, n.data(), P * sizeof(double)));
    double *d_acc = (double *)d_o, *d_mu = d_acc + M, *d_sigma = d_mu + M;
    const uint32_t S = (uint32_t)phk_div_up(M, GT_CHUNK);
    const bool full = D % GT_KC == 0;
    for (int pass = 1; pass <= 2; ++pass) {
        PHK_HIP(hipMemsetAsync(d_acc, 0, M * sizeof(double), ctx->stream));
        for (uint64_t b = 0; b < P; b += B) {
            const uint64_t nb = P - b < B ? P - b : B;
            const dim3 grid(S, (unsigned)phk_div_up(nb, GT_QB));
            const uint32_t *c = (const uint32_t *)d_c + b * D;
            if (full) {
                PHK_LAUNCH(ctx, "phk_host_pairs_kernel", phk_host_pairs_kernel<true><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                                                             c, (const double *)d_n + b, nb, t->logp.as<double>(), M, D, (double *)d_ell));
            } else {
                PHK_LAUNCH(ctx, "phk_host_pairs_kernel", phk_host_pairs_kernel<false><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                                                             c, (const double *)d_n + b, nb, t->logp.as<double>(), M, D, (double *)d_ell));
            }
            PHK_LAUNCH(ctx, "phk_host_column_kernel",
                       phk_host_column_kernel<<<dim3((unsigned)phk_div_up(M, 256)), dim3(256), 0, ctx->stream>>>(
                           (const double *)d_ell, nb, M, pass, b + nb == P ? 1 : 0, (double)P, d_acc, d_mu, d_sigma));
        }
    }
    // (the copies below wait for the stream: the upload of n has finished before the vector goes)
    PHK_TRY(phk_copy_to_host(ctx, mu, d_mu, M * sizeof(double)));
    return phk_copy_to_host(ctx, sigma, d_sigma, M * sizeof(double));
}
