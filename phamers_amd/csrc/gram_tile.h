// gram_tile.h -- the float64 Gram tile on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64) shared by the dense scorers
// (density.hip: Gaussian KDE; svm.hip: the Nu-SVC kernel matrix and decision), and the query-batch loop around it.
// A workgroup = GT_WAVES waves x GT_QT * 16 queries against one chunk of GT_CHUNK rows; per row step a wave holds
// GT_QT x GT_RT tiles of 16 x 16 dot products q.r, K streamed GT_KC columns at a time.
//
// Layout of one MFMA, lane = (li = lane & 15, kk = lane >> 4): the lane supplies A[i = li][k = kk] and B[k = kk][j = li] and
// holds C/D[row = kk + 4 reg][col = li], reg = 0..3.  Here i = query 16 a + li of the wave, j = row 16 t + li of the step.
// Column permutation: k-slot kk takes the 8 consecutive columns kc + 8 kk .. kc + 8 kk + 7 of a K step, one per MFMA, on
// BOTH operands -- so A and B are 64-byte vector loads and every product still meets its own column.
#pragma once
#include "phk_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define GT_QT 2        // 16-query tiles per wave
#define GT_RT 4        // 16-row tiles per row step
#define GT_KC 32       // columns per K step (8 per lane)
#define GT_WAVES 4
#define GT_QB (GT_WAVES * GT_QT * 16)   // queries per workgroup (128)
#define GT_CHUNK 256   // rows per workgroup

// Loads 8 consecutive doubles of row `row` at column c0 (FULL: D % GT_KC == 0, aligned vector loads).
template <bool FULL>
__device__ __forceinline__ void gram_load8(const double *__restrict__ X, uint64_t D, uint64_t row, bool ok, uint64_t c0,
                                           double v[8]) {
    if (FULL) {
        if (ok) {
            const double2 *p = (const double2 *)(X + row * D + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double2 t = p[i];
                v[2 * i] = t.x;
                v[2 * i + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.0;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (ok && c0 + i < D) ? X[row * D + c0 + i] : 0.0;
    }
}

// The same 8 columns of a uint32 count row, converted in registers (exact: every uint32 is a float64): the A operand of the
// likelihood scorer (likelihood.hip), which multiplies the integer counts themselves.
template <bool FULL>
__device__ __forceinline__ void gram_load8(const uint32_t *__restrict__ X, uint64_t D, uint64_t row, bool ok, uint64_t c0,
                                           double v[8]) {
    if (FULL) {
        if (ok) {
            const uint4 *p = (const uint4 *)(X + row * D + c0);
            const uint4 t0 = p[0], t1 = p[1];
            v[0] = (double)t0.x, v[1] = (double)t0.y, v[2] = (double)t0.z, v[3] = (double)t0.w;
            v[4] = (double)t1.x, v[5] = (double)t1.y, v[6] = (double)t1.z, v[7] = (double)t1.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.0;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (ok && c0 + i < D) ? (double)X[row * D + c0 + i] : 0.0;
    }
}

// The query that entry acc[a][t][r] of this lane belongs to (q0 = the wave's first query); its row is st + 16 t + li.
__device__ __forceinline__ uint64_t gram_query(uint64_t q0, int a, int r) {
    return q0 + 16 * a + ((threadIdx.x & 63) >> 4) + 4 * r;
}

// acc[a][t] = Q[q0 + 16 a ..][:] . R[st + 16 t ..][:] over all D columns, in column-step order (queries at or past nq and
// rows at or past r1 enter as zeros).  QT: the 16-query tiles the wave holds (GT_QT unless a kernel narrows its tile; a tile's
// products do not depend on it).  TQ: the element type of the query rows, double or uint32_t (count rows, see gram_load8).
template <bool FULL, int QT = GT_QT, typename TQ = double>
__device__ __forceinline__ void gram_tile(const TQ *__restrict__ Q, uint64_t nq, uint64_t q0, const double *__restrict__ R,
                                          uint64_t r1, uint64_t st, uint64_t D, f64x4 acc[QT][GT_RT]) {
    const int li = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int a = 0; a < QT; ++a)
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) acc[a][t] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (uint64_t kc = 0; kc < D; kc += GT_KC) {
        double qa[QT][8];
#pragma unroll
        for (int a = 0; a < QT; ++a) {
            const uint64_t q = q0 + 16 * a + li;
            gram_load8<FULL>(Q, D, q, q < nq, kc + 8 * kk, qa[a]);
        }
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint64_t j = st + 16 * t + li;
            double rb[8];
            gram_load8<FULL>(R, D, j, j < r1, kc + 8 * kk, rb);
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int a = 0; a < QT; ++a)
                    acc[a][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[a][s], rb[s], acc[a][t], 0, 0, 0);
        }
    }
}

// The host loop of both scorers: queries d_Q[N][D], or uint32 count rows d_counts[N][D] normalised into the workspace
// first, in batches of B queries against S chunks.  B: the partials (part_bytes per chunk and query) and the normalised
// count rows within 256 MiB each, a multiple of the query block.  Per batch, score(q, qn, nb, part, s) gets the batch's nb
// rows q with their norms qn, the partials array and the offset s of the batch's first query, and launches the caller's
// partial and merge kernels.  force_B != 0: that many queries per batch instead (rounded to the query block; for tests).
template <typename F>
static int gram_query_batches(phk_ctx *ctx, const double *d_Q, const uint32_t *d_counts, uint64_t N, uint64_t D, uint32_t S,
                              uint64_t part_bytes, F score, uint64_t force_B = 0) {
    uint64_t B = (256ull << 20) / ((uint64_t)S * part_bytes);
    const uint64_t Bq = (256ull << 20) / (D * sizeof(double));
    B = B < Bq ? B : Bq;
    B = B > (1ull << 20) ? (1ull << 20) : B;
    B = B < GT_QB ? GT_QB : (B / GT_QB) * GT_QB;
    if (force_B) B = phk_div_up(force_B, GT_QB) * GT_QB;
    if (B > N) B = N;
    void *part, *q64 = nullptr;
    PHK_TRY(phk_ws(ctx, WS_KDE, (uint64_t)S * B * part_bytes + B * sizeof(double), &part));
    double *qn = (double *)((char *)part + (uint64_t)S * B * part_bytes);
    if (d_counts) PHK_TRY(phk_ws(ctx, WS_Q64, B * D * sizeof(double), &q64));
    for (uint64_t s = 0; s < N; s += B) {
        const uint64_t nb = N - s < B ? N - s : B;
        const double *q = d_Q ? d_Q + s * D : (const double *)q64;
        if (d_counts) PHK_TRY(phk_launch_normalize_u32(ctx, d_counts + s * D, nb, D, (double *)q64));
        PHK_TRY(phk_launch_rownorm(ctx, q, nb, D, qn));
        PHK_TRY(score(q, (const double *)qn, nb, part, s));
    }
    return PHK_OK;
}
