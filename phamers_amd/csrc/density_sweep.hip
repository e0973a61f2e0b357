// density_sweep.hip -- the Gaussian KDE log-density of density.hip at MANY bandwidths from one pass over the pairs (gfx950):
// out[b][i] = KernelDensity('gaussian', bandwidth=h[b]).fit(X).score_samples(Q)[i], optionally leaving pair (i, i) out (the
// leave-one-out densities behind a choice of the density method's bandwidths, phamers_amd/bandwidth.py).
//
// The pair distances do not depend on the bandwidth, only the epilogue e = -d^2 / 2 h^2 does: one Gram tile (gram_tile.h,
// v_mfma_f64_16x16x4_f64) feeds up to KS_NB bandwidths per pass; more bandwidths run as further passes over the resident rows.
//
// Bit for bit phk_kde_log_density's result per bandwidth: the same chunks of GT_CHUNK rows, the same
// lane order over a chunk's rows, the same 16-lane butterfly and the same chunk-order merge.  phk_kde_partial_kernel keeps a
// running (max, sum) per query; here the sum is kept per bandwidth and the maximum is DERIVED: the kernel there compares the
// exact product -d^2 c with the running maximum (a fused multiply-add) and stores the rounded product, so its maximum is
// always fl(-min d^2 * c), c = 1 / 2 h^2 -- rounding is monotone -- and one running minimum of d^2 serves every bandwidth.
#include "density_shared.h"
#include "gram_tile.h"

#define KS_NB PHK_KDE_SWEEP_PER_PASS   // bandwidths per pass (learning.DENSITY_SWEEP_PER_PASS)
// Two shapes of the kernel, the same bits from both: <NB = KS_NB, QT = 1> -- one 16-query tile per wave, half of GT_QT: the room
// eight sums per query take -- and, for a pass of at most KS_NB_WIDE bandwidths, <NB = KS_NB_WIDE, QT = GT_QT>:
// phk_kde_partial_kernel's own tile, where every row operand serves two query tiles.
#define KS_NB_WIDE 2

template <int NB>
struct KdeSweepCoef {
    double v[NB];
};

// grid: x = chunk of GT_CHUNK rows of R, y = block of GT_WAVES * QT * 16 queries.
// part[(b * gridDim.x + chunk) * nq + q] = (max term, sum of exp(term - max)) of bandwidth b over the chunk's rows but row
// self0 + q when `exclude`; (-inf, 0) when that leaves none.  c.v[b] = 1 / 2 h_b^2 for b < nb <= NB.
// Two workgroups per CU (two waves per SIMD) in both shapes, see DESIGN.md section 4.16 for the register counts.
template <bool FULL, int NB, int QT>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_kde_sweep_partial_kernel(
    const double *__restrict__ Q, const double *__restrict__ qn, uint64_t nq, const double *__restrict__ R,
    const double *__restrict__ rn, uint64_t M, uint64_t D, KdeSweepCoef<NB> c, uint32_t nb, uint64_t self0, int exclude,
    double2 *__restrict__ part) {
// every product below that the result depends on is written out: nothing is left to contraction
#pragma clang fp contract(off)
    const int li = threadIdx.x & 15, wave = threadIdx.x >> 6;
    const uint32_t ch = blockIdx.x;
    const uint64_t r0 = (uint64_t)ch * GT_CHUNK;
    const uint64_t r1 = r0 + GT_CHUNK < M ? r0 + GT_CHUNK : M;
    const uint64_t q0 = (uint64_t)blockIdx.y * (GT_WAVES * QT * 16) + (uint64_t)wave * (QT * 16);
    const double inf = __builtin_inf();

    double qnorm[QT][4], dmin[QT][4], sm[NB][QT][4];
    uint64_t self[QT][4];
#pragma unroll
    for (int a = 0; a < QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = gram_query(q0, a, r);
            qnorm[a][r] = q < nq ? qn[q] : 0.0;
            self[a][r] = exclude ? self0 + q : ~0ull;   // no row has that index
            dmin[a][r] = inf;
#pragma unroll
            for (int b = 0; b < NB; ++b) sm[b][a][r] = 0.0;
        }

    for (uint64_t st = r0; st < r1; st += GT_RT * 16) {
        f64x4 acc[QT][GT_RT];
        gram_tile<FULL, QT>(Q, nq, q0, R, r1, st, D, acc);
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint64_t j = st + 16 * t + li;
            const bool valid = j < r1;
            const double rnj = valid ? rn[j] : 0.0;
#pragma unroll
            for (int a = 0; a < QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = valid && j != self[a][r];
                    const double d2 = fmax(__builtin_fma(-2.0, acc[a][t][r], qnorm[a][r] + rnj), 0.0);
                    const double lo = dmin[a][r];
                    const bool any = lo < inf;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        if ((uint32_t)b >= nb) break;
                        const double mx = any ? -lo * c.v[b] : -inf;   // the running maximum of bandwidth b
                        const double d = __builtin_fma(-d2, c.v[b], -mx);
                        const double x = exp(-fabs(d));
                        if (ok) sm[b][a][r] = d > 0.0 ? __builtin_fma(sm[b][a][r], x, 1.0) : sm[b][a][r] + x;
                    }
                    if (ok) dmin[a][r] = d2 < lo ? d2 : lo;
                }
        }
    }
    // the 16 lanes that share a query: the butterfly of phk_kde_partial_kernel, per bandwidth
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if ((uint32_t)b >= nb) break;
#pragma unroll
        for (int a = 0; a < QT; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double m = dmin[a][r] < inf ? -dmin[a][r] * c.v[b] : -inf, s = sm[b][a][r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const double m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
                    kde_merge(m, s, m2, s2);
                }
                const uint64_t q = gram_query(q0, a, r);
                if (li == 0 && q < nq) part[((uint64_t)b * gridDim.x + ch) * nq + q] = make_double2(m, s);
            }
    }
}

// thread (x = query, y = bandwidth of the pass): fold the chunks in chunk order and normalise, as phk_kde_merge_kernel does
// for one class.  out[b * ldo + q]; a NaN query row gives NaN and is counted once (nan_rows: the first pass only).
template <int NB>
__global__ __launch_bounds__(256) void phk_kde_sweep_merge_kernel(const double2 *__restrict__ part,
                                                                  const double *__restrict__ qn, uint64_t nq, uint32_t S,
                                                                  KdeSweepCoef<NB> lognorm, double *__restrict__ out,
                                                                  uint64_t ldo, uint32_t *__restrict__ nan_rows) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = blockIdx.y;
    if (q >= nq) return;
    if (qn[q] != qn[q]) {
        out[(uint64_t)b * ldo + q] = __builtin_nan("");
        if (nan_rows && b == 0) atomicAdd(nan_rows, 1u);
        return;
    }
    double m = -__builtin_inf(), s = 0.0;
    for (uint32_t ch = 0; ch < S; ++ch) {
        const double2 p = part[((uint64_t)b * S + ch) * nq + q];
        kde_merge(m, s, p.x, p.y);
    }
    double ln = lognorm.v[0];
#pragma unroll
    for (int i = 1; i < NB; ++i) ln = b == (uint32_t)i ? lognorm.v[i] : ln;
    out[(uint64_t)b * ldo + q] = m + log(s) - ln;
}

// one pass of nbw <= NB bandwidths over a batch of nq queries (queries s .. s + nq of the call)
template <int NB, int QT>
static int kde_sweep_launch_partial(phk_ctx *ctx, const double *q, const double *qn, uint64_t nq, const double *d_x,
                                    const double *d_rn, uint64_t M, uint64_t D, const KdeSweepCoef<NB> &c, uint32_t nbw, uint64_t s,
                                    int exclude, double2 *part) {
    const dim3 grid((unsigned)phk_div_up(M, GT_CHUNK), (unsigned)phk_div_up(nq, GT_WAVES * QT * 16));
    if (D % GT_KC == 0) {
        PHK_LAUNCH(ctx, "phk_kde_sweep_partial_kernel",
                   phk_kde_sweep_partial_kernel<true, NB, QT><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                       q, qn, nq, d_x, d_rn, M, D, c, nbw, s, exclude, part));
    } else {
        PHK_LAUNCH(ctx, "phk_kde_sweep_partial_kernel",
                   phk_kde_sweep_partial_kernel<false, NB, QT><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                       q, qn, nq, d_x, d_rn, M, D, c, nbw, s, exclude, part));
    }
    return PHK_OK;
}

extern "C" int phk_kde_sweep(phk_ctx *ctx, const double *Q, uint64_t N, const double *X, uint64_t M, uint64_t D,
                             const double *h, uint32_t B, int exclude_self, uint64_t batch_rows, double *out) {
    PHK_ENTER(ctx, "phk_kde_sweep");
    PHK_REQUIRE(B >= 1 && h, "phk_kde_sweep: no bandwidths");
    for (uint32_t b = 0; b < B; ++b)
        PHK_REQUIRE(kde_bandwidth_ok(h[b]), "phk_kde_sweep: bandwidths must be finite and > 0 (got %g at index %u)", h[b], b);
    PHK_REQUIRE(D > 0 && M > 0 && X, "phk_kde_sweep: empty data");
    if (exclude_self) {
        PHK_REQUIRE(N == M, "phk_kde_sweep: exclude_self needs the data rows as queries (%llu queries, %llu rows)",
                    (unsigned long long)N, (unsigned long long)M);
        PHK_REQUIRE(M > 1, "phk_kde_sweep: exclude_self leaves no row of a one-row data set");
    }
    if (N == 0) return PHK_OK;
    PHK_REQUIRE(Q && out, "phk_kde_sweep: NULL pointer");
    void *d_x, *d_q, *d_o, *d_flags;
    PHK_TRY(phk_ws(ctx, WS_WIDE, M * D * sizeof(double) + M * sizeof(double), &d_x));
    double *d_rn = (double *)d_x + M * D;
    PHK_TRY(phk_ws(ctx, WS_OUT, (uint64_t)B * N * sizeof(double), &d_o));
    PHK_TRY(phk_ws(ctx, WS_SUB, N * D * sizeof(double), &d_q));
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &d_flags));
    PHK_TRY(phk_copy_to_device(ctx, d_x, X, M * D * sizeof(double)));
    PHK_TRY(phk_copy_to_device(ctx, d_q, Q, N * D * sizeof(double)));
    PHK_HIP(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), ctx->stream));
    PHK_TRY(phk_launch_rownorm(ctx, (const double *)d_x, M, D, d_rn));

    const uint32_t S = (uint32_t)phk_div_up(M, GT_CHUNK);
    const uint32_t per = B < KS_NB ? B : KS_NB;
    const uint64_t n_eff = exclude_self ? M - 1 : M;
    PHK_TRY(gram_query_batches(
        ctx, (const double *)d_q, nullptr, N, D, S, (uint64_t)per * sizeof(double2),
        [&](const double *q, const double *qn, uint64_t nb, void *part, uint64_t s) -> int {
            for (uint32_t b0 = 0; b0 < B; b0 += KS_NB) {
                const uint32_t nbw = B - b0 < KS_NB ? B - b0 : KS_NB;
                KdeSweepCoef<KS_NB> c, ln;
                for (uint32_t b = 0; b < KS_NB; ++b) {
                    const double hb = h[b0 + (b < nbw ? b : nbw - 1)];
                    c.v[b] = 1.0 / (2.0 * hb * hb);
                    ln.v[b] = kde_lognorm(n_eff, D, hb);
                }
                if (nbw <= KS_NB_WIDE) {
                    KdeSweepCoef<KS_NB_WIDE> cw;
                    for (uint32_t b = 0; b < KS_NB_WIDE; ++b) cw.v[b] = c.v[b];
                    PHK_TRY((kde_sweep_launch_partial<KS_NB_WIDE, GT_QT>(ctx, q, qn, nb, (const double *)d_x, d_rn, M, D, cw, nbw, s,
                                                                         exclude_self != 0, (double2 *)part)));
                } else {
                    PHK_TRY((kde_sweep_launch_partial<KS_NB, 1>(ctx, q, qn, nb, (const double *)d_x, d_rn, M, D, c, nbw, s,
                                                                exclude_self != 0, (double2 *)part)));
                }
                PHK_LAUNCH(ctx, "phk_kde_sweep_merge_kernel",
                           phk_kde_sweep_merge_kernel<KS_NB><<<dim3((unsigned)phk_div_up(nb, 256), nbw), dim3(256), 0, ctx->stream>>>(
                               (const double2 *)part, qn, nb, S, ln, (double *)d_o + (uint64_t)b0 * N + s, N,
                               b0 == 0 ? (uint32_t *)d_flags : nullptr));
            }
            return PHK_OK;
        },
        batch_rows));
    uint32_t nan_rows = 0;
    PHK_HIP(hipMemcpyAsync(&nan_rows, d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (nan_rows) {
        phk_set_error("phk_kde_sweep: %u query row(s) contain NaN", nan_rows);
        return PHK_ERR_NAN;
    }
    return phk_copy_to_host(ctx, out, d_o, (uint64_t)B * N * sizeof(double));
}
