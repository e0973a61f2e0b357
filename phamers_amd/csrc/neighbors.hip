// neighbors.hip -- nearest-reference lookup (gfx950): the k nearest reference rows of every query row with their distances,
// what scikit-learn's NearestNeighbors(algorithm='brute').kneighbors returns over learning.distances
// (scripts/learning.py:47-66) and what learning.knn (scripts/learning.py:118-128) folds into a vote.
//
// Contract: d2(q, j) = the fma chain of pair_tile.h (direct differences, column order); the
// result of a query is the first k rows in order of (d2, j), distances sqrt(d2) -- bit for bit, whatever N, the batch
// split, the entry point or the route.
//
// Route.  (1) Proposal: phk_nn_partial_kernel, the third client of the fp64 MFMA Gram tile (gram_tile.h), keeps per
// (chunk of GT_CHUNK rows, query) the KC smallest Gram-form values a~ = max(|q|^2 + |x|^2 - 2 q.x, 0) ordered by (a~, j);
// phk_nn_merge_kernel folds a query's chunks in chunk order.  (2) Refinement: phk_nn_refine_kernel recomputes d2 of the KC
// candidates with the exact chain and orders them by (d2, j).  (3) Certificate: with E >= |a~ - d^2| for every row of the
// query and eps the chain's relative error, a row that was not kept has a~ >= a~_(KC), hence a chain value of at least
// (a~_(KC) - E)(1 - eps); the query is certified when d2_(k) + E_exact < a~_(KC) - E with E_exact = 2 eps max(d2_(k),
// a~_(KC) - E), or when every unmasked row was kept.  (4) Fallback: the other queries are gathered, run through the pair
// tile against all rows (phk_launch_dist2) and selected in order of (d2, j) by row_select.h (phk_nn_select_kernel).
#include "gram_tile.h"
#include "row_list.h"
#include "row_select.h"
#include "score_model.h"

#define NN_KMAX 28

// max_j rn[j] over all rows (masked ones included: the bound only grows), one workgroup
__global__ __launch_bounds__(256) void phk_nn_rnmax_kernel(const double *__restrict__ rn, uint64_t M, double *__restrict__ out) {
    __shared__ double s[256];
    double m = 0.0;
    for (uint64_t j = threadIdx.x; j < M; j += 256) m = fmax(m, rn[j]);
    s[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s[0];
}

// grid: x = chunk of GT_CHUNK rows of [0, M), y = block of GT_QB queries.  Per row step the 128 x 64 tile of a~ goes through
// LDS (64 KiB; entry (row, query) at column query ^ 4 (row & 15): the 64 lanes of a store hit every bank twice, the 64
// lanes of a load -- consecutive queries of one row -- once); thread (query = tid & 127, half = tid >> 7) then scans its 32
// rows of the step into a register list behind a "smaller than my worst" test.  Masked rows and rows past the chunk enter
// the tile as NaN and never pass that test.  At the end the two halves of a query meet through LDS.
// pa / pj[chunk][query][KC]: values and row indices, (+inf, NN_NOROW) where the chunk had fewer unmasked rows.
template <bool FULL, int KC>
__global__ __launch_bounds__(GT_WAVES * 64, KC <= 16 ? 2 : 1) void phk_nn_partial_kernel(
    const double *__restrict__ Q, const double *__restrict__ qn, uint64_t nq, const double *__restrict__ R,
    const double *__restrict__ rn, const uint8_t *__restrict__ mask, uint64_t M, uint64_t D, double *__restrict__ pa,
    int32_t *__restrict__ pj) {
    __shared__ double tile[NN_STEP * GT_QB];
    const int li = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x;
    const uint64_t r0 = (uint64_t)c * GT_CHUNK;
    const uint64_t r1 = r0 + GT_CHUNK < M ? r0 + GT_CHUNK : M;
    const uint64_t q0 = (uint64_t)blockIdx.y * GT_QB + (uint64_t)wave * (GT_QT * 16);
    const int myq = threadIdx.x & (GT_QB - 1), half = threadIdx.x >> 7;

    double qnorm[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = gram_query(q0, a, r);
            qnorm[a][r] = q < nq ? qn[q] : 0.0;
        }
    double lv[KC];
    int32_t lj[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        lv[i] = __builtin_inf();
        lj[i] = NN_NOROW;
    }

    for (uint64_t st = r0; st < r1; st += NN_STEP) {
        f64x4 acc[GT_QT][GT_RT];
        gram_tile<FULL>(Q, nq, q0, R, r1, st, D, acc);
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const int row = 16 * t + li;
            const uint64_t j = st + row;
            const bool valid = j < r1 && !(mask && mask[j]);
            const double rnj = valid ? rn[j] : 0.0;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ql = wave * (GT_QT * 16) + 16 * a + kk + 4 * r;
                    const double d2 = fmax(qnorm[a][r] + rnj - 2.0 * acc[a][t][r], 0.0);
                    tile[row * GT_QB + (ql ^ (li << 2))] = valid ? d2 : __builtin_nan("");
                }
        }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < NN_STEP / 2; ++i) {
            const int row = half * (NN_STEP / 2) + i;
            const double v = tile[row * GT_QB + (myq ^ ((row & 15) << 2))];
            const int32_t j = (int32_t)(st + row);
            if (nn_less(v, j, lv[KC - 1], lj[KC - 1])) nn_insert<KC>(lv, lj, v, j);
        }
        __syncthreads();
    }
    // the upper half's lists -> LDS ([entry][query]: 12 KC GT_QB bytes <= 48 KiB), the lower half takes them in, in order
    double *sv = tile;
    int32_t *sj = (int32_t *)(tile + KC * GT_QB);
    if (half) {
#pragma unroll
        for (int i = 0; i < KC; ++i) {
            sv[i * GT_QB + myq] = lv[i];
            sj[i * GT_QB + myq] = lj[i];
        }
    }
    __syncthreads();
    if (half) return;
#pragma unroll 1
    for (int i = 0; i < KC; ++i) {
        const double v = sv[i * GT_QB + myq];
        const int32_t j = sj[i * GT_QB + myq];
        if (!nn_less(v, j, lv[KC - 1], lj[KC - 1])) break;   // (sorted: no later entry gets in either)
        nn_insert<KC>(lv, lj, v, j);
    }
    const uint64_t q = (uint64_t)blockIdx.y * GT_QB + myq;
    if (q < nq) {
        const uint64_t o = ((uint64_t)c * nq + q) * KC;
#pragma unroll
        for (int i = 0; i < KC; ++i) {
            pa[o + i] = lv[i];
            pj[o + i] = lj[i];
        }
    }
}

// one thread per query: the chunks' lists in chunk order into the query's final KC candidates, ordered by (a~, j)
template <int KC>
__global__ __launch_bounds__(256) void phk_nn_merge_kernel(const double *__restrict__ pa, const int32_t *__restrict__ pj,
                                                           uint64_t nq, uint32_t S, double *__restrict__ ca,
                                                           int32_t *__restrict__ cj) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    double lv[KC];
    int32_t lj[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        lv[i] = __builtin_inf();
        lj[i] = NN_NOROW;
    }
    for (uint32_t c = 0; c < S; ++c) {
        const uint64_t o = ((uint64_t)c * nq + q) * KC;
#pragma unroll 1
        for (int i = 0; i < KC; ++i) {
            const double v = pa[o + i];
            const int32_t j = pj[o + i];
            if (!nn_less(v, j, lv[KC - 1], lj[KC - 1])) break;
            nn_insert<KC>(lv, lj, v, j);
        }
    }
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        ca[q * KC + i] = lv[i];
        cj[q * KC + i] = lj[i];
    }
}

// Error bounds of the certificate, u = 2^-53, s = |q| + max_j |x_j| from the computed norms.
// nn_bound = (2 D + 64) u s^2 >= |a~ - d2| for every row, d2 the chain value: the two norms (phk_kde_rownorm_kernel: chains
// of ceil(D / 64) fma + 6 butterfly additions: (D / 64 + 7) u s^2), the MFMA dot product of at most D + 31 terms in any order,
// doubled ((D + 31) / 2 u s^2), the two combining roundings (2 u s^2; the doubling and the clamp at 0 add nothing) -- and
// the chain's own distance from the true value, (D + 4) u s^2.  nn_eps >= the chain's relative error alone.
__device__ __forceinline__ double nn_bound(uint64_t D, double qn, double rnmax) {
    const double s = sqrt(qn) + sqrt(rnmax);
    return 0x1p-53 * (double)(2 * D + 64) * s * s;
}
__device__ __forceinline__ double nn_eps(uint64_t D) { return 0x1p-53 * (double)(D + 4); }

// KC threads per query: thread (query, c) recomputes d2 of candidate c with the chain of pair_tile.h, the KC pairs
// are ordered by (d2, j) by rank, the first k go to the output (out_* at the call's query s + q) and thread 0 decides the
// certificate; an uncertified query is appended to flist.  A NaN query row is counted in *nan_rows and left alone.
// det_*: optional details of the call (the bound, the fallback flag, the Gram-form values of the k returned rows).
template <int KC>
__global__ __launch_bounds__(256) void phk_nn_refine_kernel(
    const double *__restrict__ Q, const double *__restrict__ qn, uint64_t nq, const double *__restrict__ R, uint64_t D,
    const double *__restrict__ ca, const int32_t *__restrict__ cj, int k, int all_kept, const double *__restrict__ rnmax,
    uint64_t s, int32_t *__restrict__ out_idx, double *__restrict__ out_dist, uint32_t *__restrict__ flist,
    uint32_t *__restrict__ n_fall, uint32_t *__restrict__ nan_rows, double *__restrict__ det_E, double *__restrict__ det_a,
    uint8_t *__restrict__ det_fb) {
    __shared__ double sd[256], sa[256], od[256], oa[256];
    __shared__ int32_t sj[256], oj[256];
    const int t = threadIdx.x, ql = t / KC, c = t % KC;
    const uint64_t q = (uint64_t)blockIdx.x * (256 / KC) + ql;
    const bool live = q < nq;
    const bool isnan = live && qn[q] != qn[q];
    const int32_t j = live ? cj[q * KC + c] : NN_NOROW;
    double d2 = __builtin_inf();
    if (live && !isnan && j != NN_NOROW) {
        const double *x = Q + q * D, *y = R + (uint64_t)j * D;
        double acc = 0.0;
        for (uint64_t i = 0; i < D; ++i) {
            const double d = x[i] - y[i];
            acc = fma(d, d, acc);
        }
        d2 = acc;
    }
    sd[t] = d2;
    sj[t] = j;
    sa[t] = live ? ca[q * KC + c] : __builtin_inf();
    __syncthreads();
    int rank = 0;
    for (int e = 0; e < KC; ++e) {
        const double de = sd[ql * KC + e];
        const int32_t je = sj[ql * KC + e];
        rank += (de < d2 || (de == d2 && (je < j || (je == j && e < c)))) ? 1 : 0;
    }
    od[ql * KC + rank] = d2;
    oj[ql * KC + rank] = j;
    oa[ql * KC + rank] = sa[t];
    __syncthreads();
    if (!live) return;
    if (isnan) {
        if (c == 0) atomicAdd(nan_rows, 1u);
        return;
    }
    if (c < k) {
        out_idx[(s + q) * k + c] = oj[ql * KC + c];
        out_dist[(s + q) * k + c] = sqrt(od[ql * KC + c]);
        if (det_a) det_a[(s + q) * k + c] = oa[ql * KC + c];
    }
    if (c == 0) {
        const double E = nn_bound(D, qn[q], rnmax[0]);
        const double T = sa[ql * KC + KC - 1] - E;   // every row that was not kept has a true d^2 of at least this
        const double dk = od[ql * KC + k - 1];
        const bool cert = all_kept || dk + 2.0 * nn_eps(D) * fmax(dk, T) < T;
        if (!cert) flist[atomicAdd(n_fall, 1u)] = (uint32_t)q;
        if (det_E) {
            det_E[s + q] = E;
            det_fb[s + q] = cert ? 0 : 1;
        }
    }
}

// rows[f][:] = Q[flist[f]][:]
__global__ __launch_bounds__(256) void phk_nn_gather_kernel(const double *__restrict__ Q, uint64_t D, const uint32_t *__restrict__ flist,
                                                            uint64_t nf, double *__restrict__ rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf * D) return;
    rows[i] = Q[(uint64_t)flist[i / D] * D + i % D];
}

// One workgroup per fallen-back query: the k smallest of its M squared distances by (d2, j) (row_select.h, 32 slots), as
// indices, distances and the kept Gram-form values.  Masked rows are +inf and k <= the unmasked rows.
__global__ __launch_bounds__(256) void phk_nn_select_kernel(const double *__restrict__ D2, uint64_t M, uint32_t k,
                                                            const uint32_t *__restrict__ flist, uint64_t s,
                                                            int32_t *__restrict__ out_idx, double *__restrict__ out_dist,
                                                            const double *__restrict__ ca, const int32_t *__restrict__ cj, int KC,
                                                            double *__restrict__ det_a) {
    __shared__ uint64_t skey[32];
    __shared__ int32_t sidx[32];
    __shared__ RsScratch sc;
    const int t = threadIdx.x;
    rs_select_sorted((const uint64_t *)(D2 + (uint64_t)blockIdx.x * M), M, k, 32, skey, sidx, sc);
    const uint64_t ql = flist[blockIdx.x], q = s + ql;
    if (t < (int)k) {
        out_idx[q * k + t] = sidx[t];
        out_dist[q * k + t] = sqrt(__longlong_as_double((long long)skey[t]));
        if (det_a) {   // the Gram-form value of a returned row the proposal kept; NaN for one it did not keep
            double a = __builtin_nan("");
            for (int e = 0; e < KC; ++e)
                if (cj[ql * KC + e] == sidx[t]) a = ca[ql * KC + e];
            det_a[q * k + t] = a;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct NnLists {
    double *pa, *ca;
    int32_t *pj, *cj;
};

template <int KC>
static int nn_propose(phk_ctx *ctx, const double *q, const double *qn, uint64_t nb, const double *d_R, const double *d_rn,
                      const uint8_t *d_mask, uint64_t M, uint64_t D, uint32_t S, const NnLists &l) {
    const dim3 grid(S, (unsigned)phk_div_up(nb, GT_QB));
    if (D % GT_KC == 0) {
        PHK_LAUNCH(ctx, "phk_nn_partial_kernel", phk_nn_partial_kernel<true, KC><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                                                     q, qn, nb, d_R, d_rn, d_mask, M, D, l.pa, l.pj));
    } else {
        PHK_LAUNCH(ctx, "phk_nn_partial_kernel", phk_nn_partial_kernel<false, KC><<<grid, dim3(GT_WAVES * 64), 0, ctx->stream>>>(
                                                     q, qn, nb, d_R, d_rn, d_mask, M, D, l.pa, l.pj));
    }
    PHK_LAUNCH(ctx, "phk_nn_merge_kernel", phk_nn_merge_kernel<KC><<<dim3((unsigned)phk_div_up(nb, 256)), dim3(256), 0, ctx->stream>>>(
                                               l.pa, l.pj, nb, S, l.ca, l.cj));
    return PHK_OK;
}

struct NnRefineArgs {
    int k, all_kept;
    const double *rnmax;
    uint64_t s;
    int32_t *out_idx;
    double *out_dist;
    uint32_t *flist, *n_fall, *nan_rows;
    double *det_E, *det_a;
    uint8_t *det_fb;
};

template <int KC>
static int nn_refine(phk_ctx *ctx, const double *q, const double *qn, uint64_t nb, const double *d_R, uint64_t D,
                     const NnLists &l, const NnRefineArgs &a) {
    PHK_LAUNCH(ctx, "phk_nn_refine_kernel",
               phk_nn_refine_kernel<KC><<<dim3((unsigned)phk_div_up(nb, 256 / KC)), dim3(256), 0, ctx->stream>>>(
                   q, qn, nb, d_R, D, l.ca, l.cj, a.k, a.all_kept, a.rnmax, a.s, a.out_idx, a.out_dist, a.flist, a.n_fall,
                   a.nan_rows, a.det_E, a.det_a, a.det_fb));
    return PHK_OK;
}

static inline uint64_t nn_up256(uint64_t b) { return (b + 255) & ~255ull; }

// The k nearest of the M rows d_R (norms d_rn, optional mask, `unmasked` rows left) for the queries d_Q[N][D] or the
// uint32 count rows d_counts[N][D]; idx[N][k] / dist[N][k] to the host.
static int nn_run(phk_ctx *ctx, const char *fname, const double *d_Q, const uint32_t *d_counts, uint64_t N, const double *d_R,
                  const double *d_rn, const uint8_t *d_mask, uint64_t M, uint64_t unmasked, uint64_t D, int k,
                  uint64_t batch_rows, int32_t *idx, double *dist) {
    const int KC = k <= 4 ? 8 : (k <= 12 ? 16 : 32);
    const uint32_t S = (uint32_t)phk_div_up(M, GT_CHUNK);
    void *p;
    PHK_TRY(phk_ws(ctx, WS_OUT, nn_up256(N * k * 8) + N * k * 4, &p));
    double *d_dist = (double *)p;
    int32_t *d_idx = (int32_t *)((char *)p + nn_up256(N * k * 8));
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &p));
    uint32_t *d_nan = (uint32_t *)p, *d_nfall = (uint32_t *)p + 4;
    double *d_rnmax = (double *)p + 1;
    PHK_HIP(hipMemsetAsync(p, 0, 64, ctx->stream));
    double *det_E = nullptr, *det_a = nullptr;
    uint8_t *det_fb = nullptr;
    ctx->nn_det_n = 0;
    if (ctx->nn_keep) {
        PHK_TRY(phk_ws(ctx, WS_NND, nn_up256(N * 8) + nn_up256(N * k * 8) + N, &p));
        det_E = (double *)p;
        det_a = (double *)((char *)p + nn_up256(N * 8));
        det_fb = (uint8_t *)p + nn_up256(N * 8) + nn_up256(N * k * 8);
    }
    PHK_LAUNCH(ctx, "phk_nn_rnmax_kernel", phk_nn_rnmax_kernel<<<dim3(1), dim3(256), 0, ctx->stream>>>(d_rn, M, d_rnmax));
    const int all_kept = unmasked <= (uint64_t)KC;
    uint64_t fell = 0;
    PHK_TRY(gram_query_batches(
        ctx, d_Q, d_counts, N, D, S, (uint64_t)KC * 12,
        [&](const double *q, const double *qn, uint64_t nb, void *part, uint64_t s) -> int {
            void *w;
            PHK_TRY(phk_ws(ctx, WS_NN, nb * KC * 12 + nb * 4, &w));
            NnLists l;
            l.pa = (double *)part;
            l.pj = (int32_t *)((char *)part + (uint64_t)S * nb * KC * 8);
            l.ca = (double *)w;
            l.cj = (int32_t *)((char *)w + nb * KC * 8);
            uint32_t *flist = (uint32_t *)((char *)w + nb * KC * 12);
            const NnRefineArgs a = {k, all_kept, d_rnmax, s, d_idx, d_dist, flist, d_nfall, d_nan, det_E, det_a, det_fb};
            if (KC == 8) {
                PHK_TRY(nn_propose<8>(ctx, q, qn, nb, d_R, d_rn, d_mask, M, D, S, l));
                PHK_TRY(nn_refine<8>(ctx, q, qn, nb, d_R, D, l, a));
            } else if (KC == 16) {
                PHK_TRY(nn_propose<16>(ctx, q, qn, nb, d_R, d_rn, d_mask, M, D, S, l));
                PHK_TRY(nn_refine<16>(ctx, q, qn, nb, d_R, D, l, a));
            } else {
                PHK_TRY(nn_propose<32>(ctx, q, qn, nb, d_R, d_rn, d_mask, M, D, S, l));
                PHK_TRY(nn_refine<32>(ctx, q, qn, nb, d_R, D, l, a));
            }
            uint32_t nf = 0;
            PHK_HIP(hipMemcpyAsync(&nf, d_nfall, 4, hipMemcpyDeviceToHost, ctx->stream));
            PHK_HIP(hipStreamSynchronize(ctx->stream));
            if (!nf) return PHK_OK;
            fell += nf;
            PHK_HIP(hipMemsetAsync(d_nfall, 0, 4, ctx->stream));
            // fallback: every row, the exact chain, an ordered select; F queries at a time (<= 256 MiB of distances)
            uint64_t F = (256ull << 20) / (M * sizeof(double));
            F = F < 1 ? 1 : (F > nf ? nf : F);
            void *rows, *d2;
            PHK_TRY(phk_ws(ctx, WS_NNF, F * D * sizeof(double), &rows));
            PHK_TRY(phk_ws(ctx, WS_DIST, F * M * sizeof(double), &d2));
            for (uint64_t f0 = 0; f0 < nf; f0 += F) {
                const uint64_t fb = nf - f0 < F ? nf - f0 : F;
                PHK_LAUNCH(ctx, "phk_nn_gather_kernel",
                           phk_nn_gather_kernel<<<dim3((unsigned)phk_div_up(fb * D, 256)), dim3(256), 0, ctx->stream>>>(
                               q, D, flist + f0, fb, (double *)rows));
                PHK_TRY(phk_launch_dist2(ctx, (const double *)rows, fb, d_R, M, D, (double *)d2));
                if (d_mask) PHK_TRY(phk_launch_mask_dist(ctx, (double *)d2, fb, M, d_mask));
                PHK_LAUNCH(ctx, "phk_nn_select_kernel",
                           phk_nn_select_kernel<<<dim3((unsigned)fb), dim3(256), 0, ctx->stream>>>(
                               (const double *)d2, M, (uint32_t)k, flist + f0, s, d_idx, d_dist, l.ca, l.cj, KC, det_a));
            }
            return PHK_OK;
        },
        batch_rows));
    uint32_t nan_rows = 0;
    PHK_HIP(hipMemcpyAsync(&nan_rows, d_nan, 4, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (nan_rows) {
        phk_set_error("%s: %u query row(s) contain NaN", fname, nan_rows);
        return PHK_ERR_NAN;
    }
    ctx->nn_queries += N;
    ctx->nn_fell_back += fell;
    if (ctx->nn_keep) {
        ctx->nn_det_n = N;
        ctx->nn_det_k = k;
    }
    PHK_TRY(phk_copy_to_host(ctx, idx, d_idx, N * k * 4));
    return phk_copy_to_host(ctx, dist, d_dist, N * k * 8);
}

static int nn_check_k(const char *fname, int k, uint64_t unmasked, uint64_t M) {
    PHK_REQUIRE(k >= 1 && k <= NN_KMAX, "%s: k = %d is not in 1..%d", fname, k, NN_KMAX);
    PHK_REQUIRE((uint64_t)k <= unmasked, "%s: k = %d exceeds the %llu unmasked reference rows", fname, k,
                (unsigned long long)unmasked);
    PHK_REQUIRE(M < (1ull << 31), "%s: %llu reference rows do not fit int32 indices", fname, (unsigned long long)M);
    return PHK_OK;
}

extern "C" int phk_neighbors(phk_ctx *ctx, const double *Q, uint64_t N, const double *X, uint64_t M, uint64_t D, int k,
                             uint64_t batch_rows, int32_t *idx, double *dist) {
    PHK_ENTER(ctx, "phk_neighbors");
    PHK_REQUIRE(D > 0 && M > 0 && X, "phk_neighbors: empty data");
    PHK_TRY(nn_check_k("phk_neighbors", k, M, M));
    PHK_REQUIRE(N == 0 || (Q && idx && dist), "phk_neighbors: NULL pointer");
    if (N == 0) return PHK_OK;
    void *d_x, *d_q;
    PHK_TRY(phk_ws(ctx, WS_WIDE, M * D * sizeof(double) + M * sizeof(double), &d_x));
    double *d_rn = (double *)d_x + M * D;
    PHK_TRY(phk_ws(ctx, WS_SUB, N * D * sizeof(double), &d_q));
    PHK_TRY(phk_copy_to_device(ctx, d_x, X, M * D * sizeof(double)));
    PHK_TRY(phk_copy_to_device(ctx, d_q, Q, N * D * sizeof(double)));
    PHK_TRY(phk_launch_rownorm(ctx, (const double *)d_x, M, D, d_rn));
    return nn_run(ctx, "phk_neighbors", (const double *)d_q, nullptr, N, (const double *)d_x, d_rn, nullptr, M, M, D, k,
                  batch_rows, idx, dist);
}

extern "C" int phk_model_neighbors(phk_ctx *ctx, const phk_model *m, const double *Q, uint64_t N, int k, int32_t *idx,
                                   double *dist) {
    PHK_ENTER(ctx, "phk_model_neighbors");
    PHK_REQUIRE(m, "phk_model_neighbors: NULL model");
    const uint64_t unmasked = m->has_mask ? m->eff_pos + m->eff_neg : m->M;
    PHK_TRY(nn_check_k("phk_model_neighbors", k, unmasked, m->M));
    PHK_REQUIRE(N == 0 || (Q && idx && dist), "phk_model_neighbors: NULL pointer");
    if (N == 0) return PHK_OK;
    void *d_q;
    PHK_TRY(phk_ws(ctx, WS_SUB, N * m->D * sizeof(double), &d_q));
    PHK_TRY(phk_copy_to_device(ctx, d_q, Q, N * m->D * sizeof(double)));
    return nn_run(ctx, "phk_model_neighbors", (const double *)d_q, nullptr, N, m->d_R64, m->d_rn,
                  m->has_mask ? m->d_col_mask : nullptr, m->M, unmasked, m->D, k, 0, idx, dist);
}

extern "C" int phk_batch_neighbors(phk_ctx *ctx, const phk_model *m, const phk_batch *b, int k, int32_t *idx, double *dist) {
    PHK_ENTER(ctx, "phk_batch_neighbors");
    PHK_REQUIRE(m && b, "phk_batch_neighbors: NULL model/batch");
    PHK_REQUIRE(b->D == m->D, "phk_batch_neighbors: batch has %llu columns, model %llu", (unsigned long long)b->D,
                (unsigned long long)m->D);
    const uint64_t unmasked = m->has_mask ? m->eff_pos + m->eff_neg : m->M;
    PHK_TRY(nn_check_k("phk_batch_neighbors", k, unmasked, m->M));
    PHK_REQUIRE(b->n == 0 || (idx && dist), "phk_batch_neighbors: NULL pointer");
    if (b->n == 0) return PHK_OK;
    return nn_run(ctx, "phk_batch_neighbors", nullptr, b->d_counts, b->n, m->d_R64, m->d_rn,
                  m->has_mask ? m->d_col_mask : nullptr, m->M, unmasked, m->D, k, 0, idx, dist);
}

extern "C" int phk_neighbors_stats(phk_ctx *ctx, uint64_t out[2]) {
    PHK_REQUIRE(ctx && out, "phk_neighbors_stats: NULL pointer");
    out[0] = ctx->nn_queries;
    out[1] = ctx->nn_fell_back;
    ctx->nn_queries = ctx->nn_fell_back = 0;
    return PHK_OK;
}

extern "C" int phk_neighbors_keep_details(phk_ctx *ctx, int on) {
    PHK_REQUIRE(ctx, "phk_neighbors_keep_details: NULL ctx");
    ctx->nn_keep = on != 0;
    ctx->nn_det_n = 0;
    return PHK_OK;
}

extern "C" int phk_neighbors_details(phk_ctx *ctx, uint64_t N, int k, double *E, double *approx_d2, uint8_t *fell_back) {
    PHK_ENTER(ctx, "phk_neighbors_details");
    PHK_REQUIRE(E && approx_d2 && fell_back, "phk_neighbors_details: NULL pointer");
    PHK_REQUIRE(ctx->nn_det_n > 0 && ctx->nn_det_n == N && ctx->nn_det_k == k,
                "phk_neighbors_details: no kept details of a %llu x %d call (phk_neighbors_keep_details)", (unsigned long long)N, k);
    const char *p = (const char *)ctx->ws[WS_NND].ptr;
    PHK_TRY(phk_copy_to_host(ctx, E, p, N * 8));
    PHK_TRY(phk_copy_to_host(ctx, approx_d2, p + nn_up256(N * 8), N * k * 8));
    return phk_copy_to_host(ctx, fell_back, p + nn_up256(N * 8) + nn_up256(N * k * 8), N);
}
