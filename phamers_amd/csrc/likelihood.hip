// likelihood.hip -- length-aware multinomial likelihood scoring (gfx950): this project's own method, DESIGN.md 4.20.
//
// A contig is its integer count row c (D bins); a class is a mixture of multinomials, one component per reference row r:
//     p_r[j]   = (x_r[j] + a) / (sum_j x_r[j] + D a)            (built on the host; the device sees log p_r only)
//     S[q, r]  = sum_j c_q[j] log p_r[j]                         (the multinomial coefficient cancels in the ratio)
//     l_C(q)   = logsumexp_{r in C, group(r) != group(q)} S[q, r] - log n_eff(q, C)
//     score(q) = l_+(q) - l_-(q)                                 (nats)
// Everything is float64.  S is an N x M product on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64, gram_tile.h) whose A
// operand is the resident uint32 count rows themselves, converted in registers (exact), and whose B operand is the log
// table [M][D]; no normalised copy of the queries exists.
//
// Shape of the work, as density.hip: the rows of each class are cut into chunks of GT_CHUNK rows (a cut that depends on
// the class sizes only); workgroup (chunk, query block) keeps a running (max, sum) of its chunk's terms per lane and query
// -- one exp per pair --, folds the 16 lanes of a query with a fixed butterfly and writes the pair to a partials array;
// phk_lik_merge_kernel folds a query's chunks in chunk order.  The reduction order of one query is fixed by the table
// alone: the same for any N, batch split or entry point.
#include <algorithm>

#include "density_shared.h"
#include "gram_tile.h"

// grid: x = chunk (class-major: the n_cpos chunks of [0, n_pos), then those of [n_pos, M)), y = block of GT_QB queries.
// part[chunk][q] = (max term, sum of exp(term - max)) over the chunk's rows whose group is not the query's; (-inf, 0) when
// there is none.  qg / rg: group ids of the queries / the table's rows (NULL = none); a pair is left out when both ids are
// >= 0 and equal.
template <bool FULL>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_lik_partial_kernel(
    const uint32_t *__restrict__ C, const int32_t *__restrict__ qg, uint64_t nq, const double *__restrict__ L,
    const int32_t *__restrict__ rg, uint64_t n_pos, uint64_t M, uint64_t D, uint32_t n_cpos, double2 *__restrict__ part) {
    const int li = threadIdx.x & 15, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x;
    const bool pos = c < n_cpos;
    const uint64_t r0 = pos ? (uint64_t)c * GT_CHUNK : n_pos + (uint64_t)(c - n_cpos) * GT_CHUNK;
    const uint64_t seg_end = pos ? n_pos : M;
    const uint64_t r1 = r0 + GT_CHUNK < seg_end ? r0 + GT_CHUNK : seg_end;
    const uint64_t q0 = (uint64_t)blockIdx.y * GT_QB + (uint64_t)wave * (GT_QT * 16);

    int32_t qgrp[GT_QT][4];
    double mx[GT_QT][4], sm[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = gram_query(q0, a, r);
            qgrp[a][r] = (qg && q < nq) ? qg[q] : -1;
            mx[a][r] = -__builtin_inf();
            sm[a][r] = 0.0;
        }

    for (uint64_t st = r0; st < r1; st += GT_RT * 16) {
        f64x4 acc[GT_QT][GT_RT];
        gram_tile<FULL, GT_QT, uint32_t>(C, nq, q0, L, r1, st, D, acc);
        // epilogue: one exp per (query, row) -- exp(-|e - m|) serves both the new term and the rescale of the old sum
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint64_t j = st + 16 * t + li;
            const bool inside = j < r1;
            const int32_t rgj = (inside && rg) ? rg[j] : -1;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double e = acc[a][t][r];
                    const double d = e - mx[a][r];
                    const double x = exp(-fabs(d));
                    const bool up = d > 0.0;
                    if (inside && !(rgj >= 0 && rgj == qgrp[a][r])) {
                        sm[a][r] = up ? fma(sm[a][r], x, 1.0) : sm[a][r] + x;
                        mx[a][r] = up ? e : mx[a][r];
                    }
                }
        }
    }
    // the 16 lanes that share a query (same k-slot): fixed butterfly
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const double m2 = __shfl_xor(mx[a][r], o), s2 = __shfl_xor(sm[a][r], o);
                kde_merge(mx[a][r], sm[a][r], m2, s2);
            }
    if (li == 0) {
#pragma unroll
        for (int a = 0; a < GT_QT; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t q = gram_query(q0, a, r);
                if (q < nq) part[(uint64_t)c * nq + q] = make_double2(mx[a][r], sm[a][r]);
            }
    }
}

// one thread per query: fold the chunks of each class in chunk order, l_C = max + log(sum) - log(n_eff), score = l+ - l-
// (n_cneg == 0: one class, l- = 0 and score = l+).  n_eff of query q: neff[q] / neff[nq_all + q] (positive / negative)
// when the call has groups, else the class sizes.  The logarithm of n_eff is taken here, by the function that takes the
// sum's: a query without counts has sum == n_eff and scores exactly 0.
__global__ __launch_bounds__(256) void phk_lik_merge_kernel(const double2 *__restrict__ part, uint64_t nq, uint32_t n_cpos,
                                                            uint32_t n_cneg, const uint32_t *__restrict__ neff_pos,
                                                            const uint32_t *__restrict__ neff_neg, double n_pos, double n_neg,
                                                            double *__restrict__ lp_out, double *__restrict__ ln_out,
                                                            double *__restrict__ score_out) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    double mp = -__builtin_inf(), sp = 0.0, mn = -__builtin_inf(), sn = 0.0;
    for (uint32_t c = 0; c < n_cpos; ++c) {
        const double2 p = part[(uint64_t)c * nq + q];
        kde_merge(mp, sp, p.x, p.y);
    }
    for (uint32_t c = n_cpos; c < n_cpos + n_cneg; ++c) {
        const double2 p = part[(uint64_t)c * nq + q];
        kde_merge(mn, sn, p.x, p.y);
    }
    const double lp = mp + (log(sp) - log(neff_pos ? (double)neff_pos[q] : n_pos));
    const double ln = n_cneg ? mn + (log(sn) - log(neff_neg ? (double)neff_neg[q] : n_neg)) : 0.0;
    lp_out[q] = lp;
    ln_out[q] = ln;
    score_out[q] = lp - ln;
}

// ---- the resident table ----------------------------------------------------------------------------------------------
struct phk_lik_table {
    uint64_t n_pos = 0, n_neg = 0, D = 0;
    PhkDevMem logp;                       // [n_pos + n_neg][D] float64, positive rows first
    PhkDevMem groups;                     // [n_pos + n_neg] int32, or empty
    std::vector<int32_t> gpos, gneg;      // the non-negative group ids of each class, sorted (host): n_eff of a query
};

extern "C" int phk_lik_table_create(phk_ctx *ctx, const double *log_pos, uint64_t n_pos, const int32_t *groups_pos,
                                    const double *log_neg, uint64_t n_neg, const int32_t *groups_neg, uint64_t D,
                                    phk_lik_table **out) {
    PHK_ENTER(ctx, "phk_lik_table_create");
    PHK_REQUIRE(out, "phk_lik_table_create: NULL out");
    *out = nullptr;
    PHK_REQUIRE(D > 0 && n_pos > 0 && log_pos, "phk_lik_table_create: no positive rows");
    PHK_REQUIRE(n_neg == 0 || log_neg, "phk_lik_table_create: NULL negative rows");
    PHK_REQUIRE(n_pos + n_neg < (1ull << 32) && D < (1ull << 32), "phk_lik_table_create: table too large");
    if (!phk_rows_finite(log_pos, n_pos * D) || (n_neg && !phk_rows_finite(log_neg, n_neg * D))) {
        phk_set_error("phk_lik_table_create: the log table holds a value that is not finite (a zero profile entry?)");
        return PHK_ERR_NAN;
    }
    phk_lik_table *t = new phk_lik_table();
    t->n_pos = n_pos, t->n_neg = n_neg, t->D = D;
    const uint64_t M = n_pos + n_neg;
    int rc = t->logp.alloc("phk_lik_table_create", "log table", M * D * sizeof(double));
    if (rc == PHK_OK) rc = phk_copy_to_device(ctx, t->logp.ptr, log_pos, n_pos * D * sizeof(double));
    if (rc == PHK_OK && n_neg)
        rc = phk_copy_to_device(ctx, t->logp.as<double>() + n_pos * D, log_neg, n_neg * D * sizeof(double));
    if (rc == PHK_OK && (groups_pos || groups_neg)) {
        std::vector<int32_t> g(M, -1);
        if (groups_pos) std::copy(groups_pos, groups_pos + n_pos, g.begin());
        if (groups_neg) std::copy(groups_neg, groups_neg + n_neg, g.begin() + n_pos);
        for (uint64_t i = 0; i < M; ++i)
            if (g[i] >= 0) (i < n_pos ? t->gpos : t->gneg).push_back(g[i]);
        std::sort(t->gpos.begin(), t->gpos.end());
        std::sort(t->gneg.begin(), t->gneg.end());
        rc = t->groups.alloc("phk_lik_table_create", "group ids", M * sizeof(int32_t));
        if (rc == PHK_OK && hipMemcpy(t->groups.ptr, g.data(), M * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            phk_set_error("phk_lik_table_create: upload of the group ids failed");
            rc = PHK_ERR_HIP;
        }
    }
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        phk_set_error("phk_lik_table_create: upload failed");
        rc = PHK_ERR_HIP;
    }
    if (rc != PHK_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return PHK_OK;
}

extern "C" int phk_lik_table_destroy(phk_ctx *ctx, phk_lik_table *t) {
    if (!t) return PHK_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete t;
    return PHK_OK;
}

static uint32_t lik_rows_outside(const std::vector<int32_t> &sorted, uint64_t n, int32_t g) {
    if (g < 0) return (uint32_t)n;
    const auto range = std::equal_range(sorted.begin(), sorted.end(), g);
    return (uint32_t)(n - (uint64_t)(range.second - range.first));
}

// The scoring loop of both entries: count rows d_counts[N][D] on the device, host group ids (or NULL); the three results
// go to the host arrays.  Queries run in batches of B against all S chunks: B keeps the partials within 256 MiB, is a
// multiple of the query block and at most 2^20 (force_B != 0: that many, rounded up to the query block; for tests).
static int lik_run(phk_ctx *ctx, const char *fname, const phk_lik_table *t, const uint32_t *d_counts, uint64_t N,
                   const int32_t *query_groups, uint64_t force_B, double *l_pos, double *l_neg, double *scores) {
    const uint64_t M = t->n_pos + t->n_neg, D = t->D;
    const uint32_t n_cpos = (uint32_t)phk_div_up(t->n_pos, GT_CHUNK), n_cneg = (uint32_t)phk_div_up(t->n_neg, GT_CHUNK);
    const uint32_t S = n_cpos + n_cneg;
    const bool grouped = query_groups && t->groups.ptr;
    // n_eff of every query, known from the group histograms before any launch
    std::vector<uint32_t> neff;
    if (grouped) {
        neff.resize(2 * N);
        for (uint64_t q = 0; q < N; ++q) {
            neff[q] = lik_rows_outside(t->gpos, t->n_pos, query_groups[q]);
            neff[N + q] = lik_rows_outside(t->gneg, t->n_neg, query_groups[q]);
            PHK_REQUIRE(neff[q] > 0 && (t->n_neg == 0 || neff[N + q] > 0),
                        "%s: query %llu (group %d) leaves no %s row to score against", fname, (unsigned long long)q,
                        (int)query_groups[q], neff[q] ? "negative" : "positive");
        }
    }
    uint64_t B = (256ull << 20) / ((uint64_t)S * sizeof(double2));
    B = B > (1ull << 20) ? (1ull << 20) : B;
    B = B < GT_QB ? GT_QB : (B / GT_QB) * GT_QB;
    if (force_B) B = phk_div_up(force_B, GT_QB) * GT_QB;
    if (B > N) B = N;
    void *part, *d_out, *d_q = nullptr;
    PHK_TRY(phk_ws(ctx, WS_KDE, (uint64_t)S * B * sizeof(double2), &part));
    PHK_TRY(phk_ws(ctx, WS_OUT, 3 * N * sizeof(double), &d_out));
    const int32_t *d_qg = nullptr;
    const uint32_t *d_neff = nullptr;
    if (grouped) {
        PHK_TRY(phk_ws(ctx, WS_SUB, 3 * N * sizeof(uint32_t), &d_q));
        PHK_TRY(phk_copy_to_device(ctx, d_q, query_groups, N * sizeof(int32_t)));
        PHK_TRY(phk_copy_to_device(ctx, (uint32_t *)d_q + N, neff.data(), 2 * N * sizeof(uint32_t)));
        d_qg = (const int32_t *)d_q;
        d_neff = (const uint32_t *)d_q + N;
    }
    double *d_lp = (double *)d_out, *d_ln = d_lp + N, *d_sc = d_ln + N;
    const double *d_L = t->logp.as<double>();
    const int32_t *d_rg = grouped ? t->groups.as<int32_t>() : nullptr;
    const bool full = D % GT_KC == 0;
    for (uint64_t s = 0; s < N; s += B) {
        const uint64_t nb = N - s < B ? N - s : B;
        const dim3 grid(S, (unsigned)phk_div_up(nb, GT_QB));
        if (full) {
            PHK_LAUNCH(ctx, "phk_lik_partial_kernel",
                       phk_lik_partial_kernel<true><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                           d_counts + s * D, d_qg ? d_qg + s : nullptr, nb, d_L, d_rg, t->n_pos, M, D, n_cpos, (double2 *)part));
        } else {
            PHK_LAUNCH(ctx, "phk_lik_partial_kernel",
                       phk_lik_partial_kernel<false><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                           d_counts + s * D, d_qg ? d_qg + s : nullptr, nb, d_L, d_rg, t->n_pos, M, D, n_cpos, (double2 *)part));
        }
        PHK_LAUNCH(ctx, "phk_lik_merge_kernel",
                   phk_lik_merge_kernel<<<dim3((unsigned)phk_div_up(nb, 256)), dim3(256), 0, ctx->stream>>>(
                       (const double2 *)part, nb, n_cpos, n_cneg, d_neff ? d_neff + s : nullptr,
                       d_neff ? d_neff + N + s : nullptr, (double)t->n_pos, (double)t->n_neg, d_lp + s, d_ln + s, d_sc + s));
    }
    // (the copies below wait for the stream: the upload of neff has finished before the vector goes)
    if (l_pos) PHK_TRY(phk_copy_to_host(ctx, l_pos, d_lp, N * sizeof(double)));
    if (l_neg) PHK_TRY(phk_copy_to_host(ctx, l_neg, d_ln, N * sizeof(double)));
    PHK_TRY(phk_copy_to_host(ctx, scores, d_sc, N * sizeof(double)));
    return PHK_OK;
}

extern "C" int phk_lik_score(phk_ctx *ctx, const phk_lik_table *t, const uint32_t *counts, uint64_t N, uint64_t D,
                             const int32_t *query_groups, uint64_t batch_rows, double *l_pos, double *l_neg, double *scores) {
    PHK_ENTER(ctx, "phk_lik_score");
    PHK_REQUIRE(t, "phk_lik_score: NULL table");
    PHK_REQUIRE(D == t->D, "phk_lik_score: the counts have %llu columns, the table %llu", (unsigned long long)D,
                (unsigned long long)t->D);
    if (N == 0) return PHK_OK;
    PHK_REQUIRE(counts && scores, "phk_lik_score: NULL pointer");
    void *d_c;
    PHK_TRY(phk_ws(ctx, WS_COUNTS, N * D * sizeof(uint32_t), &d_c));
    PHK_TRY(phk_copy_to_device(ctx, d_c, counts, N * D * sizeof(uint32_t)));
    return lik_run(ctx, "phk_lik_score", t, (const uint32_t *)d_c, N, query_groups, batch_rows, l_pos, l_neg, scores);
}

extern "C" int phk_batch_lik_score(phk_ctx *ctx, const phk_lik_table *t, const phk_batch *b, double *l_pos, double *l_neg,
                                   double *scores) {
    PHK_ENTER(ctx, "phk_batch_lik_score");
    PHK_REQUIRE(t && b, "phk_batch_lik_score: NULL table/batch");
    PHK_REQUIRE(b->D == t->D, "phk_batch_lik_score: the batch has %llu columns, the table %llu", (unsigned long long)b->D,
                (unsigned long long)t->D);
    if (b->n == 0) return PHK_OK;
    PHK_REQUIRE(scores, "phk_batch_lik_score: NULL scores");
    return lik_run(ctx, "phk_batch_lik_score", t, b->d_counts, b->n, nullptr, 0, l_pos, l_neg, scores);
}
