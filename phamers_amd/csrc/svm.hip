// svm.hip -- Nu-SVC (RBF kernel, binary labels) on the GPU (gfx950): phamer_scorer.svm_score_points (scripts/phamer.py:
// 258-266), i.e. scikit-learn's NuSVC().fit(train, labels).predict(points), following scikit-learn's libsvm fork
// (sklearn/svm/src/libsvm/svm.cpp) without shrinking.
//
// Training.
//   * Rows are taken in libsvm's grouped order (svm_group_classes): label-0 rows first with y = +1, then label-1 rows with
//     y = -1, each class in its original order.
//   * Q[i][j] = (float)(y_i y_j exp(-gamma (|x_i|^2 + |x_j|^2 - 2 x_i.x_j))), n x n float32 (libsvm's Qfloat), from the
//     fp64 MFMA Gram tile of gram_tile.h; QD_ii = 1 exactly (libsvm's x_square[i] + x_square[i] - 2 dot(x_i, x_i) = 0).
//   * Solver_NU runs in ONE workgroup of SVM_T threads: thread t owns rows t, t + SVM_T, ...  An iteration is
//     (i) two block-wide (value, index) arg-max reductions with the sequential scan's last-index ties,
//     (ii) the j choice over rows Q_ip / Q_in (min obj_diff, last index on ties) plus the two second maxima,
//     (iii) the two-variable update by thread 0, (iv) G += Q_i d_i + Q_j d_j by the row owners.
//     A launch runs at most SVM_STEPS iterations and leaves (alpha, G, iteration, done) in global memory; the host
//     relaunches until the stop test holds.
//   * calculate_rho is a sequential pass (one thread, row order, as libsvm sums).
//   All solver arithmetic is compiled without fp contraction: libsvm rounds every product.
//
// Decision.  dec(q) = sum_sv coef_sv exp(-gamma |q - x_sv|^2) - rho on the same Gram tile (gram_tile.h, shared with density.hip)
// with a weighted-sum epilogue.  Support vectors are cut into chunks of GT_CHUNK (a cut that depends on the model only),
// a workgroup sums one chunk for a block of queries, and the merge kernel folds a query's chunks in chunk order: a query's
// value is bit-identical for any batch split and entry point.  The method's score is 1.0 where libsvm's value is <= 0
// (scikit-learn's predict gives classes_[1] = 1.0 there), else 0.0.
#include <cmath>
#include <vector>

#include "gram_tile.h"
#include "score_model.h"
#include "svm_shared.h"

// The Gram tile: grid x = chunk of GT_CHUNK rows of R, y = block of GT_QB rows of A.  d2 = max(|a|^2 + |r|^2 - 2 a.r, 0).
// GRAM = true:  Qf[a][r] = (float)(y_a y_r exp(-gamma d2)) (A = R = the training rows, nq = nr = n; Qf[i][i] = 1).
// GRAM = false: part[chunk][a] = sum over the chunk's rows r of coef[r] exp(-gamma d2), lanes folded by a fixed butterfly.
template <bool FULL, bool GRAM>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_svm_tile_kernel(
    const double *__restrict__ A, const double *__restrict__ an, uint64_t nq, const double *__restrict__ R,
    const double *__restrict__ rn, uint64_t nr, uint64_t D, double gamma, const double *__restrict__ coef,
    const int8_t *__restrict__ y, float *__restrict__ Qf, double *__restrict__ part) {
    const int li = threadIdx.x & 15, wave = threadIdx.x >> 6;
    const uint64_t r0 = (uint64_t)blockIdx.x * GT_CHUNK;
    const uint64_t r1 = r0 + GT_CHUNK < nr ? r0 + GT_CHUNK : nr;
    const uint64_t q0 = (uint64_t)blockIdx.y * GT_QB + (uint64_t)wave * (GT_QT * 16);

    double qnorm[GT_QT][4], sm[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = gram_query(q0, a, r);
            qnorm[a][r] = q < nq ? an[q] : 0.0;
            sm[a][r] = 0.0;
        }

    for (uint64_t st = r0; st < r1; st += GT_RT * 16) {
        f64x4 acc[GT_QT][GT_RT];
        gram_tile<FULL>(A, nq, q0, R, r1, st, D, acc);
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint64_t j = st + 16 * t + li;
            const bool valid = j < r1;
            const double rnj = valid ? rn[j] : 0.0;
            const double cj = (!GRAM && valid) ? coef[j] : 0.0;
            const double yj = (GRAM && valid) ? (double)y[j] : 0.0;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double d2 = fmax(qnorm[a][r] + rnj - 2.0 * acc[a][t][r], 0.0);
                    const double k = exp(-gamma * d2);
                    if (GRAM) {
                        const uint64_t q = gram_query(q0, a, r);
                        if (valid && q < nq) Qf[q * nr + j] = q == j ? 1.0f : (float)((double)y[q] * yj * k);
                    } else if (valid) {
                        sm[a][r] += cj * k;
                    }
                }
        }
    }
    if (GRAM) return;
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) sm[a][r] += __shfl_xor(sm[a][r], o);
    if (li == 0) {
#pragma unroll
        for (int a = 0; a < GT_QT; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t q = gram_query(q0, a, r);
                if (q < nq) part[(uint64_t)blockIdx.x * nq + q] = sm[a][r];
            }
    }
}

// one thread per query: the chunks in chunk order, minus rho.  SCORE: 1.0 where the value is <= 0, else 0.0; a NaN query
// row scores NaN and is counted in *nan_rows.  Otherwise the value itself.
template <bool SCORE>
__global__ __launch_bounds__(256) void phk_svm_merge_kernel(const double *__restrict__ part, const double *__restrict__ qn,
                                                            uint64_t nq, uint32_t n_chunks, double rho,
                                                            double *__restrict__ out, uint32_t *__restrict__ nan_rows) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (qn[q] != qn[q]) {
        out[q] = __builtin_nan("");
        if (nan_rows) atomicAdd(nan_rows, 1u);
        return;
    }
    double s = 0.0;
    for (uint32_t c = 0; c < n_chunks; ++c) s += part[(uint64_t)c * nq + q];
    const double dec = s - rho;
    out[q] = SCORE ? (dec <= 0.0 ? 1.0 : 0.0) : dec;
}

// ---- solver ------------------------------------------------------------------------------------------------------------
// Solver::Solve's gradient start: G[j] = sum over rows i with alpha_i > 0, in row order, of alpha_i Q[i][j]
__global__ __launch_bounds__(256) void phk_svm_grad_init_kernel(const float *__restrict__ Qf, const double *__restrict__ alpha,
                                                                uint64_t n, double *__restrict__ G) {
#pragma clang fp contract(off)
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double g = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        const double a = alpha[i];
        if (a > 0.0) g = g + a * (double)Qf[i * n + j];
    }
    G[j] = g;
}

// Solver_NU (svm_solve_steps, svm_shared.h): at most max_steps iterations from the state in (alpha, G, ctl).
__global__ __launch_bounds__(SVM_T) void phk_svm_solve_kernel(const float *__restrict__ Qf, const int8_t *__restrict__ y,
                                                              uint64_t n, double eps, int32_t max_iter, int32_t max_steps,
                                                              double *__restrict__ alpha, double *__restrict__ G,
                                                              SvmCtl *__restrict__ ctl) {
    __shared__ SvmShared sh;
    if (ctl->done) return;
    int iter = ctl->iter;
    const bool finished = svm_solve_steps<SVM_T>(Qf, y, n, eps, max_iter, max_steps, alpha, G, iter, sh);
    if (threadIdx.x == 0) {
        if (finished) ctl->done = 1;
        ctl->iter = iter;
    }
}

// Solver_NU::calculate_rho, one thread, row order
__global__ __launch_bounds__(64) void phk_svm_rho_kernel(const int8_t *__restrict__ y, uint64_t n,
                                                         const double *__restrict__ alpha, const double *__restrict__ G,
                                                         SvmCtl *__restrict__ ctl) {
    if (threadIdx.x == 0) svm_calculate_rho(y, n, alpha, G, ctl);
}

// rows idx[0..n) of X[][D] -> out[n][D]
__global__ __launch_bounds__(256) void phk_svm_gather_kernel(const double *__restrict__ X, uint64_t D,
                                                             const uint32_t *__restrict__ idx, uint64_t n,
                                                             double *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * D) return;
    const uint64_t r = e / D, c = e - r * D;
    out[e] = X[(uint64_t)idx[r] * D + c];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
namespace {

bool svm_gamma_ok(double g) { return g > 0.0 && g < __builtin_inf(); }

}   // namespace

int svm_launch_gram(phk_ctx *ctx, const double *d_Xg, const double *xn, uint64_t n, uint64_t D, double gamma, const int8_t *dy,
                    float *Qf) {
    const dim3 grid((unsigned)phk_div_up(n, GT_CHUNK), (unsigned)phk_div_up(n, GT_QB));
    if (D % GT_KC == 0) {
        PHK_LAUNCH(ctx, "phk_svm_gram_kernel",
                   (phk_svm_tile_kernel<true, true><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                       d_Xg, xn, n, d_Xg, xn, n, D, gamma, nullptr, dy, Qf, nullptr)));
    } else {
        PHK_LAUNCH(ctx, "phk_svm_gram_kernel",
                   (phk_svm_tile_kernel<false, true><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                       d_Xg, xn, n, d_Xg, xn, n, D, gamma, nullptr, dy, Qf, nullptr)));
    }
    return PHK_OK;
}

int svm_launch_gather(phk_ctx *ctx, const double *d_X, uint64_t D, const uint32_t *d_idx, uint64_t n, double *d_out) {
    PHK_LAUNCH(ctx, "phk_svm_gather_kernel",
               phk_svm_gather_kernel<<<dim3((unsigned)phk_div_up(n * D, 256)), dim3(256), 0, ctx->stream>>>(d_X, D, d_idx, n,
                                                                                                            d_out));
    return PHK_OK;
}

// svm_check_parameter (svm.cpp:3129) for nu-SVC with two classes of n0 / n1 rows, and the other arguments
static int svm_check(uint64_t n0, uint64_t n1, double nu, double gamma, double tol) {
    PHK_REQUIRE(n0 > 0 && n1 > 0, "phk_nusvc_fit: the number of classes has to be greater than one; got 1 class");
    PHK_REQUIRE(nu > 0.0 && nu <= 1.0, "phk_nusvc_fit: nu <= 0 or nu > 1 (got %g)", nu);
    PHK_REQUIRE(!(nu * (double)(n0 + n1) / 2 > (double)(n0 < n1 ? n0 : n1)), "phk_nusvc_fit: specified nu is infeasible");
    PHK_REQUIRE(svm_gamma_ok(gamma), "phk_nusvc_fit: gamma must be finite and > 0 (got %g)", gamma);
    PHK_REQUIRE(tol > 0.0 && tol < __builtin_inf(), "phk_nusvc_fit: tol must be finite and > 0 (got %g)", tol);
    PHK_REQUIRE(n0 + n1 <= SVM_MAX_ROWS, "phk_nusvc_fit: %llu training rows (at most %u)", (unsigned long long)(n0 + n1),
                SVM_MAX_ROWS);
    return PHK_OK;
}

// The fit on device rows d_Xg[n][D] in grouped order (n0 rows y = +1, then y = -1).  Out: libsvm's coefficients
// alpha_i y_i / r for every grouped row (0 where alpha_i = 0), rho / r, the iteration count.
static int svm_fit_grouped(phk_ctx *ctx, const double *d_Xg, uint64_t n0, uint64_t n, uint64_t D, double nu, double gamma,
                           double tol, int32_t max_iter, std::vector<double> &coef, double *rho, int32_t *n_iter) {
    PhkDevMem b[5];   // the fit's buffers, freed on every way out
    PHK_TRY(b[0].alloc("phk_nusvc_fit", "row norms", n * sizeof(double)));
    PHK_TRY(b[1].alloc("phk_nusvc_fit", "Q", n * n * sizeof(float)));
    PHK_TRY(b[2].alloc("phk_nusvc_fit", "alpha and G", 2 * n * sizeof(double)));
    PHK_TRY(b[3].alloc("phk_nusvc_fit", "y", n));
    PHK_TRY(b[4].alloc("phk_nusvc_fit", "control words", sizeof(SvmCtl)));
    double *xn = b[0].as<double>(), *alpha = b[2].as<double>(), *G = alpha + n;
    float *Qf = b[1].as<float>();
    int8_t *dy = b[3].as<int8_t>();
    SvmCtl *dctl = b[4].as<SvmCtl>();

    // solve_nu_svc: y, and alpha filled class by class up to nu l / 2 (nu_l = sum of nu * C_i, C_i = 1)
    std::vector<int8_t> y(n);
    std::vector<double> a0(n);
    {
#pragma clang fp contract(off)
        double nu_l = 0.0;
        for (uint64_t i = 0; i < n; ++i) nu_l += nu * 1.0;
        double sp = nu_l / 2, sn = nu_l / 2;
        for (uint64_t i = 0; i < n; ++i) {
            y[i] = i < n0 ? 1 : -1;
            if (y[i] == 1) {
                a0[i] = 1.0 < sp ? 1.0 : sp;
                sp -= a0[i];
            } else {
                a0[i] = 1.0 < sn ? 1.0 : sn;
                sn -= a0[i];
            }
        }
    }
    SvmCtl c0 = {0, 0, 0.0, 0.0};
    PHK_HIP(hipMemcpyAsync(dy, y.data(), n, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(alpha, a0.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(dctl, &c0, sizeof(SvmCtl), hipMemcpyHostToDevice, ctx->stream));
    PHK_TRY(phk_launch_rownorm(ctx, d_Xg, n, D, xn));
    PHK_TRY(svm_launch_gram(ctx, d_Xg, xn, n, D, gamma, dy, Qf));
    PHK_LAUNCH(ctx, "phk_svm_grad_init_kernel",
               phk_svm_grad_init_kernel<<<dim3((unsigned)phk_div_up(n, 256)), dim3(256), 0, ctx->stream>>>(Qf, alpha, n, G));
    SvmCtl c;
    for (;;) {
        PHK_LAUNCH(ctx, "phk_svm_solve_kernel",
                   phk_svm_solve_kernel<<<dim3(1), dim3(SVM_T), 0, ctx->stream>>>(Qf, dy, n, tol, max_iter, SVM_STEPS, alpha,
                                                                                   G, dctl));
        PHK_HIP(hipMemcpyAsync(&c, dctl, sizeof(SvmCtl), hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        if (c.done) break;
    }
    PHK_LAUNCH(ctx, "phk_svm_rho_kernel", phk_svm_rho_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(dy, n, alpha, G, dctl));
    std::vector<double> a(n);
    PHK_HIP(hipMemcpyAsync(a.data(), alpha, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipMemcpyAsync(&c, dctl, sizeof(SvmCtl), hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    // solve_nu_svc: alpha_i *= y_i / r, rho /= r
    coef.assign(n, 0.0);
    for (uint64_t i = 0; i < n; ++i) coef[i] = a[i] * ((double)y[i] / c.r);
    *rho = c.rho / c.r;
    // scikit-learn refuses a fit whose support-vector coefficients or intercept are not finite (sklearn/svm/_base.py, fit):
    // r = 0, e.g. two identical rows with opposite labels and nothing else
    bool finite = std::isfinite(*rho);
    for (uint64_t i = 0; i < n; ++i) finite = finite && (a[i] == 0.0 || std::isfinite(coef[i]));
    PHK_REQUIRE(finite, "phk_nusvc_fit: The dual coefficients or intercepts are not finite. The input data may contain large "
                        "values and need to be preprocessed.");
    *n_iter = c.iter;
    return PHK_OK;
}

// Decision over support vectors d_sv[n_sv][D] (norms d_svn, coefficients d_coef) for queries d_Q[N][D] or uint32 count
// rows (normalised into the workspace first).  SCORE: the method's 1.0 / 0.0 (NaN rows NaN, counted in d_status); else
// libsvm's value.
int svm_decision_run(phk_ctx *ctx, const double *d_Q, const uint32_t *d_counts, uint64_t N, const double *d_sv,
                     const double *d_svn, const double *d_coef, uint64_t n_sv, uint64_t D, double gamma, double rho, bool score,
                     double *d_out, uint32_t *d_status) {
    const uint32_t S = (uint32_t)phk_div_up(n_sv, GT_CHUNK);
    const bool full = D % GT_KC == 0;
    return gram_query_batches(
        ctx, d_Q, d_counts, N, D, S, sizeof(double),
        [&](const double *q, const double *qn, uint64_t nb, void *part, uint64_t s) -> int {
            const dim3 grid(S, (unsigned)phk_div_up(nb, GT_QB));
            if (full) {
                PHK_LAUNCH(ctx, "phk_svm_partial_kernel",
                           (phk_svm_tile_kernel<true, false><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                               q, qn, nb, d_sv, d_svn, n_sv, D, gamma, d_coef, nullptr, nullptr, (double *)part)));
            } else {
                PHK_LAUNCH(ctx, "phk_svm_partial_kernel",
                           (phk_svm_tile_kernel<false, false><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                               q, qn, nb, d_sv, d_svn, n_sv, D, gamma, d_coef, nullptr, nullptr, (double *)part)));
            }
            const dim3 mg((unsigned)phk_div_up(nb, 256));
            if (score) {
                PHK_LAUNCH(ctx, "phk_svm_merge_kernel",
                           phk_svm_merge_kernel<true><<<mg, dim3(256), 0, ctx->stream>>>((const double *)part, qn, nb, S, rho,
                                                                                       d_out + s, d_status));
            } else {
                PHK_LAUNCH(ctx, "phk_svm_merge_kernel",
                           phk_svm_merge_kernel<false><<<mg, dim3(256), 0, ctx->stream>>>((const double *)part, qn, nb, S, rho,
                                                                                        d_out + s, d_status));
            }
            return PHK_OK;
        });
}

// ---- standalone NuSVC ---------------------------------------------------------------------------------------------------
extern "C" int phk_nusvc_fit(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const double *labels, double nu,
                             double gamma, double tol, int32_t max_iter, int32_t *support, double *dual_coef, double *rho,
                             int32_t *n_sv, int32_t *n_iter) {
    PHK_ENTER(ctx, "phk_nusvc_fit");
    PHK_REQUIRE(X && labels && support && dual_coef && rho && n_sv && n_iter && D > 0, "phk_nusvc_fit: NULL pointer or D = 0");
    PHK_REQUIRE(max_iter == -1 || max_iter > 0, "phk_nusvc_fit: max_iter must be -1 or > 0 (got %d)", max_iter);
    // svm_group_classes: label 0 first, then label 1
    std::vector<uint32_t> perm;
    perm.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        PHK_REQUIRE(labels[i] == 0.0 || labels[i] == 1.0, "phk_nusvc_fit: labels must be 0 or 1 (row %llu: %g)",
                    (unsigned long long)i, labels[i]);
        if (labels[i] == 0.0) perm.push_back((uint32_t)i);
    }
    const uint64_t n0 = perm.size();
    for (uint64_t i = 0; i < n; ++i)
        if (labels[i] == 1.0) perm.push_back((uint32_t)i);
    PHK_TRY(svm_check(n0, n - n0, nu, gamma, tol));
    void *d_x, *d_xg, *d_idx;
    PHK_TRY(phk_ws(ctx, WS_WIDE, n * D * sizeof(double), &d_x));
    PHK_TRY(phk_ws(ctx, WS_SUB, n * D * sizeof(double), &d_xg));
    PHK_TRY(phk_ws(ctx, WS_OFFSETS, n * sizeof(uint32_t), &d_idx));
    PHK_TRY(phk_copy_to_device(ctx, d_x, X, n * D * sizeof(double)));
    PHK_HIP(hipMemcpyAsync(d_idx, perm.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PHK_LAUNCH(ctx, "phk_svm_gather_kernel",
               phk_svm_gather_kernel<<<dim3((unsigned)phk_div_up(n * D, 256)), dim3(256), 0, ctx->stream>>>(
                   (const double *)d_x, D, (const uint32_t *)d_idx, n, (double *)d_xg));
    std::vector<double> coef;
    PHK_TRY(svm_fit_grouped(ctx, (const double *)d_xg, n0, n, D, nu, gamma, tol, max_iter, coef, rho, n_iter));
    int32_t k = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (coef[i] != 0.0) {
            support[k] = (int32_t)perm[i];
            dual_coef[k] = coef[i];
            ++k;
        }
    *n_sv = k;
    return PHK_OK;
}

extern "C" int phk_nusvc_decision(phk_ctx *ctx, const double *SV, uint64_t n_sv, uint64_t D, const double *dual_coef,
                                  double rho, double gamma, const double *Q, uint64_t N, double *dec) {
    PHK_ENTER(ctx, "phk_nusvc_decision");
    PHK_REQUIRE(svm_gamma_ok(gamma), "phk_nusvc_decision: gamma must be finite and > 0 (got %g)", gamma);
    PHK_REQUIRE(D > 0 && n_sv > 0 && SV && dual_coef, "phk_nusvc_decision: empty model");
    if (N == 0) return PHK_OK;
    PHK_REQUIRE(Q && dec, "phk_nusvc_decision: NULL pointer");
    void *d_sv, *d_q, *d_o, *d_flags;
    PHK_TRY(phk_ws(ctx, WS_WIDE, n_sv * D * sizeof(double) + 2 * n_sv * sizeof(double), &d_sv));
    double *d_svn = (double *)d_sv + n_sv * D, *d_coef = d_svn + n_sv;
    PHK_TRY(phk_ws(ctx, WS_OUT, N * sizeof(double), &d_o));
    PHK_TRY(phk_ws(ctx, WS_SUB, N * D * sizeof(double), &d_q));
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &d_flags));
    PHK_TRY(phk_copy_to_device(ctx, d_sv, SV, n_sv * D * sizeof(double)));
    PHK_HIP(hipMemcpyAsync(d_coef, dual_coef, n_sv * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PHK_TRY(phk_copy_to_device(ctx, d_q, Q, N * D * sizeof(double)));
    PHK_HIP(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), ctx->stream));
    PHK_TRY(phk_launch_rownorm(ctx, (const double *)d_sv, n_sv, D, d_svn));
    PHK_TRY(svm_decision_run(ctx, (const double *)d_q, nullptr, N, (const double *)d_sv, d_svn, d_coef, n_sv, D, gamma, rho,
                             false, (double *)d_o, (uint32_t *)d_flags));
    PHK_TRY(phk_copy_to_host(ctx, dec, d_o, N * sizeof(double)));
    return PHK_OK;
}

// ---- model side ---------------------------------------------------------------------------------------------------------
void phk_model_free_svm(phk_model *m) {
    if (m->d_sv) (void)hipFree(m->d_sv);
    m->d_sv = nullptr;
    m->n_sv = 0;
    m->svm_fitted = false;
}

extern "C" int phk_model_fit_svm(phk_ctx *ctx, phk_model *m, double nu, double gamma, double tol) {
    PHK_ENTER(ctx, "phk_model_fit_svm");
    PHK_REQUIRE(m, "phk_model_fit_svm: NULL model");
    // the model's unmasked train rows in libsvm's grouped order: negative rows (label 0) first, then positive rows
    std::vector<uint8_t> mask(m->M, 0);
    if (m->has_mask) PHK_HIP(hipMemcpy(mask.data(), m->d_col_mask, m->M, hipMemcpyDeviceToHost));
    std::vector<uint32_t> idx;
    idx.reserve(m->M);
    for (uint64_t r = m->n_pos; r < m->M; ++r)
        if (!mask[r]) idx.push_back((uint32_t)r);
    const uint64_t n0 = idx.size();
    for (uint64_t r = 0; r < m->n_pos; ++r)
        if (!mask[r]) idx.push_back((uint32_t)r);
    const uint64_t n = idx.size(), D = m->D;
    PHK_TRY(svm_check(n0, n - n0, nu, gamma, tol));
    void *d_xg, *d_idx;
    PHK_TRY(phk_ws(ctx, WS_SUB, n * D * sizeof(double), &d_xg));
    PHK_TRY(phk_ws(ctx, WS_OFFSETS, n * sizeof(uint32_t), &d_idx));
    PHK_HIP(hipMemcpyAsync(d_idx, idx.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PHK_LAUNCH(ctx, "phk_svm_gather_kernel",
               phk_svm_gather_kernel<<<dim3((unsigned)phk_div_up(n * D, 256)), dim3(256), 0, ctx->stream>>>(
                   m->d_R64, D, (const uint32_t *)d_idx, n, (double *)d_xg));
    std::vector<double> coef;
    double rho;
    int32_t it;
    PHK_TRY(svm_fit_grouped(ctx, (const double *)d_xg, n0, n, D, nu, gamma, tol, -1, coef, &rho, &it));
    // support vectors (grouped order) -> the model: rows, norms, coefficients
    std::vector<uint32_t> sv;
    std::vector<double> sc;
    for (uint64_t i = 0; i < n; ++i)
        if (coef[i] != 0.0) {
            sv.push_back(idx[i]);
            sc.push_back(coef[i]);
        }
    const uint64_t ns = sv.size();
    PHK_REQUIRE(ns > 0, "phk_model_fit_svm: no support vectors");
    phk_model_free_svm(m);   // (a refused fit keeps the previous one)
    PHK_HIP(hipMalloc((void **)&m->d_sv, ns * D * sizeof(double) + 2 * ns * sizeof(double)));
    m->d_svn = m->d_sv + ns * D;
    m->d_svcoef = m->d_svn + ns;
    PHK_HIP(hipMemcpyAsync(d_idx, sv.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(m->d_svcoef, sc.data(), ns * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PHK_LAUNCH(ctx, "phk_svm_gather_kernel",
               phk_svm_gather_kernel<<<dim3((unsigned)phk_div_up(ns * D, 256)), dim3(256), 0, ctx->stream>>>(
                   m->d_R64, D, (const uint32_t *)d_idx, ns, m->d_sv));
    PHK_TRY(phk_launch_rownorm(ctx, m->d_sv, ns, D, m->d_svn));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    m->n_sv = ns;
    m->svm_rho = rho;
    m->svm_gamma = gamma;
    m->svm_iter = it;
    m->svm_fitted = true;
    return PHK_OK;
}

int phk_score_svm(phk_ctx *ctx, const phk_model *m, const double *d_Q, const uint32_t *d_counts, uint64_t N, double *d_scores,
                  uint32_t *d_status) {
    PHK_REQUIRE(m->svm_fitted, "phk_score: the svm method needs phk_model_fit_svm first");
    return svm_decision_run(ctx, d_Q, d_counts, N, m->d_sv, m->d_svn, m->d_svcoef, m->n_sv, m->D, m->svm_gamma, m->svm_rho,
                            true, d_scores, d_status);
}
