// density.hip -- Gaussian kernel density scoring (gfx950): phamer_scorer.density_score_points (scripts/phamer.py:275-287)
// and learning.get_density (scripts/learning.py:107-115, scikit-learn KernelDensity(kernel='gaussian').score_samples).
//
// Per query q and class c (rows j of the class that are not masked out):
//     e_j = -max(|q|^2 + |r_j|^2 - 2 q.r_j, 0) / (2 h_c^2)
//     L_c = logsumexp_j(e_j) - log(n_c_eff) - (D/2) log(2 pi) - D log(h_c)
//     score = L_+ - L_-
// Everything is float64: the Gram product on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64), the norms, the exponent and exp.
// No row can be skipped ("Density"): the kernel is dense.
//
// Shape of the work.  The rows of each class are cut into chunks of GT_CHUNK rows (a cut that depends on the class sizes
// only); workgroup (chunk, query block) keeps, per query, a running (max, sum) of its chunk's terms and writes it to a
// partials array; phk_kde_merge_kernel folds a query's chunks in chunk order.  The reduction order of one query is thus
// fixed by the model alone -- the same for any N, batch split or entry point.
#include "density_shared.h"
#include "gram_tile.h"
#include "score_model.h"

// |x|^2 of rows of X[n][D], float64, one wave per row: lanes stride the columns in order, then a fixed butterfly.  Used
// for the model's rows and for the queries alike.
__global__ __launch_bounds__(256) void phk_kde_rownorm_kernel(const double *__restrict__ X, uint64_t n, uint64_t D,
                                                              double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= n) return;
    const double *x = X + r * D;
    double s = 0.0;
    for (uint64_t k = lane; k < D; k += 64) s = fma(x[k], x[k], s);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[r] = s;
}

// grid: x = chunk (class-major: the n_cpos chunks of [0, n_pos), then those of [n_pos, M)), y = block of GT_QB queries.
// part[chunk][q] = (max term, sum of exp(term - max)) over the chunk's unmasked rows; (-inf, 0) when it has none.
// Two workgroups per CU (two waves per SIMD, 220 registers, no spills): 64.6 ms per 2^20 queries against 93.7 ms at one wave
// per SIMD (284 registers), same results (profiles/density/README.md).
template <bool FULL>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_kde_partial_kernel(
    const double *__restrict__ Q, const double *__restrict__ qn, uint64_t nq, const double *__restrict__ R,
    const double *__restrict__ rn, const uint8_t *__restrict__ mask, uint64_t n_pos, uint64_t M, uint64_t D,
    uint32_t n_cpos, double inv2h2_pos, double inv2h2_neg, double2 *__restrict__ part) {
    const int li = threadIdx.x & 15, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x;
    const bool pos = c < n_cpos;
    const uint64_t r0 = pos ? (uint64_t)c * GT_CHUNK : n_pos + (uint64_t)(c - n_cpos) * GT_CHUNK;
    const uint64_t seg_end = pos ? n_pos : M;
    const uint64_t r1 = r0 + GT_CHUNK < seg_end ? r0 + GT_CHUNK : seg_end;
    const double inv2h2 = pos ? inv2h2_pos : inv2h2_neg;
    const uint64_t q0 = (uint64_t)blockIdx.y * GT_QB + (uint64_t)wave * (GT_QT * 16);

    double qnorm[GT_QT][4], mx[GT_QT][4], sm[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = gram_query(q0, a, r);
            qnorm[a][r] = q < nq ? qn[q] : 0.0;
            mx[a][r] = -__builtin_inf();
            sm[a][r] = 0.0;
        }

    for (uint64_t st = r0; st < r1; st += GT_RT * 16) {
        f64x4 acc[GT_QT][GT_RT];
        gram_tile<FULL>(Q, nq, q0, R, r1, st, D, acc);
        // epilogue: one exp per (query, row) -- exp(-|e - m|) serves both the new term and the rescale of the old sum
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint64_t j = st + 16 * t + li;
            const bool valid = j < r1 && !(mask && mask[j]);
            const double rnj = valid ? rn[j] : 0.0;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double d2 = fmax(qnorm[a][r] + rnj - 2.0 * acc[a][t][r], 0.0);
                    const double e = -d2 * inv2h2;
                    const double d = e - mx[a][r];
                    const double x = exp(-fabs(d));
                    const bool up = d > 0.0;
                    if (valid) {
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

// one thread per query: fold the chunks of each class in chunk order, normalise, score = L+ - L- (n_cneg == 0: L+ alone).
// A NaN query row (zero-count contig) scores NaN and is counted in *nan_rows.
__global__ __launch_bounds__(256) void phk_kde_merge_kernel(const double2 *__restrict__ part, const double *__restrict__ qn,
                                                            uint64_t nq, uint32_t n_cpos, uint32_t n_cneg, double lognorm_pos,
                                                            double lognorm_neg, double *__restrict__ out,
                                                            uint32_t *__restrict__ nan_rows) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (qn[q] != qn[q]) {
        out[q] = __builtin_nan("");
        if (nan_rows) atomicAdd(nan_rows, 1u);
        return;
    }
    double mp = -__builtin_inf(), sp = 0.0, mn = -__builtin_inf(), sn = 0.0;
    for (uint32_t c = 0; c < n_cpos; ++c) {
        const double2 p = part[(uint64_t)c * nq + q];
        kde_merge(mp, sp, p.x, p.y);
    }
    for (uint32_t c = n_cpos; c < n_cpos + n_cneg; ++c) {
        const double2 p = part[(uint64_t)c * nq + q];
        kde_merge(mn, sn, p.x, p.y);
    }
    const double lp = mp + log(sp) - lognorm_pos;
    out[q] = n_cneg ? lp - (mn + log(sn) - lognorm_neg) : lp;
}

// |x|^2 of the n rows of d_X[n][D] -> d_out[n]
int phk_launch_rownorm(phk_ctx *ctx, const double *d_X, uint64_t n, uint64_t D, double *d_out) {
    PHK_LAUNCH(ctx, "phk_kde_rownorm_kernel",
               phk_kde_rownorm_kernel<<<dim3((unsigned)phk_div_up(n, 4)), dim3(256), 0, ctx->stream>>>(d_X, n, D, d_out));
    return PHK_OK;
}

// The scoring loop shared by the model path and the standalone entry: queries d_Q[N][D] (or uint32 count rows normalised
// into the workspace first), train rows d_R[M][D] with norms d_rn, classes [0, n_pos) and [n_pos, M).
static int kde_run(phk_ctx *ctx, const double *d_Q, const uint32_t *d_counts, uint64_t N, const double *d_R, const double *d_rn,
                   const uint8_t *d_mask, uint64_t n_pos, uint64_t M, uint64_t D, double h_pos, double h_neg, uint64_t eff_pos,
                   uint64_t eff_neg, double *d_out, uint32_t *d_status) {
    const uint32_t n_cpos = (uint32_t)phk_div_up(n_pos, GT_CHUNK), n_cneg = (uint32_t)phk_div_up(M - n_pos, GT_CHUNK);
    const uint32_t S = n_cpos + n_cneg;
    const double lp = kde_lognorm(eff_pos ? eff_pos : 1, D, h_pos), ln = n_cneg ? kde_lognorm(eff_neg, D, h_neg) : 0.0;
    const double i2p = 1.0 / (2.0 * h_pos * h_pos), i2n = n_cneg ? 1.0 / (2.0 * h_neg * h_neg) : 0.0;
    const bool full = D % GT_KC == 0;
    return gram_query_batches(
        ctx, d_Q, d_counts, N, D, S, sizeof(double2),
        [&](const double *q, const double *qn, uint64_t nb, void *part, uint64_t s) -> int {
            const dim3 grid(S, (unsigned)phk_div_up(nb, GT_QB));
            if (full) {
                PHK_LAUNCH(ctx, "phk_kde_partial_kernel",
                           phk_kde_partial_kernel<true><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                               q, qn, nb, d_R, d_rn, d_mask, n_pos, M, D, n_cpos, i2p, i2n, (double2 *)part));
            } else {
                PHK_LAUNCH(ctx, "phk_kde_partial_kernel",
                           phk_kde_partial_kernel<false><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                               q, qn, nb, d_R, d_rn, d_mask, n_pos, M, D, n_cpos, i2p, i2n, (double2 *)part));
            }
            PHK_LAUNCH(ctx, "phk_kde_merge_kernel",
                       phk_kde_merge_kernel<<<dim3((unsigned)phk_div_up(nb, 256)), dim3(256), 0, ctx->stream>>>(
                           (const double2 *)part, qn, nb, n_cpos, n_cneg, lp, ln, d_out + s, d_status));
            return PHK_OK;
        });
}

// ---- model side ------------------------------------------------------------------------------------------------------
int phk_model_build_density(phk_ctx *ctx, phk_model *m) {
    m->h_pos = 0.005;   // scripts/phamer.py:82-83
    m->h_neg = 0.01;
    m->eff_pos = m->n_pos;
    m->eff_neg = m->n_neg;
    PHK_HIP(hipMalloc((void **)&m->d_rn, m->M * sizeof(double)));
    PHK_TRY(phk_launch_rownorm(ctx, m->d_R64, m->M, m->D, m->d_rn));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    return PHK_OK;
}

int phk_score_density(phk_ctx *ctx, const phk_model *m, const double *d_Q, const uint32_t *d_counts, uint64_t N,
                      double *d_scores, uint32_t *d_status) {
    PHK_REQUIRE(m->eff_pos > 0 && m->eff_neg > 0,
                "phk_score: density needs unmasked rows in both classes (%llu positive, %llu negative)",
                (unsigned long long)m->eff_pos, (unsigned long long)m->eff_neg);
    return kde_run(ctx, d_Q, d_counts, N, m->d_R64, m->d_rn, m->has_mask ? m->d_col_mask : nullptr, m->n_pos, m->M, m->D,
                   m->h_pos, m->h_neg, m->eff_pos, m->eff_neg, d_scores, d_status);
}

extern "C" int phk_model_set_bandwidths(phk_ctx *ctx, phk_model *m, double h_pos, double h_neg) {
    PHK_ENTER(ctx, "phk_model_set_bandwidths");
    PHK_REQUIRE(m, "phk_model_set_bandwidths: NULL model");
    PHK_REQUIRE(kde_bandwidth_ok(h_pos) && kde_bandwidth_ok(h_neg),
                "phk_model_set_bandwidths: bandwidths must be finite and > 0 (got %g, %g)", h_pos, h_neg);
    m->h_pos = h_pos;
    m->h_neg = h_neg;
    return PHK_OK;
}

// ---- standalone KernelDensity.score_samples ----------------------------------------------------------------------------
extern "C" int phk_kde_log_density(phk_ctx *ctx, const double *Q, uint64_t N, const double *X, uint64_t M, uint64_t D,
                                   double h, double *out) {
    PHK_ENTER(ctx, "phk_kde_log_density");
    PHK_REQUIRE(kde_bandwidth_ok(h), "phk_kde_log_density: bandwidth must be finite and > 0 (got %g)", h);
    PHK_REQUIRE(D > 0 && M > 0 && X, "phk_kde_log_density: empty data");
    if (N == 0) return PHK_OK;
    PHK_REQUIRE(Q && out, "phk_kde_log_density: NULL pointer");
    void *d_x, *d_q, *d_o, *d_flags;
    PHK_TRY(phk_ws(ctx, WS_WIDE, M * D * sizeof(double) + M * sizeof(double), &d_x));
    double *d_rn = (double *)d_x + M * D;
    PHK_TRY(phk_ws(ctx, WS_OUT, N * sizeof(double), &d_o));
    PHK_TRY(phk_ws(ctx, WS_SUB, N * D * sizeof(double), &d_q));
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &d_flags));
    PHK_TRY(phk_copy_to_device(ctx, d_x, X, M * D * sizeof(double)));
    PHK_TRY(phk_copy_to_device(ctx, d_q, Q, N * D * sizeof(double)));
    PHK_HIP(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), ctx->stream));
    PHK_TRY(phk_launch_rownorm(ctx, (const double *)d_x, M, D, d_rn));
    PHK_TRY(kde_run(ctx, (const double *)d_q, nullptr, N, (const double *)d_x, d_rn, nullptr, M, M, D, h, h, M, 0, (double *)d_o,
                    (uint32_t *)d_flags));
    uint32_t nan_rows = 0;
    PHK_HIP(hipMemcpyAsync(&nan_rows, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (nan_rows) {
        phk_set_error("phk_kde_log_density: %u query row(s) contain NaN", nan_rows);
        return PHK_ERR_NAN;
    }
    return phk_copy_to_host(ctx, out, d_o, N * sizeof(double));
}
