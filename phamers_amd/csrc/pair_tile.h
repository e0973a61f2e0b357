// pair_tile.h -- the 64 x 64 pair tile of float64 DIRECT-DIFFERENCE squared distances shared by the all-pairs passes
// (cluster.hip: silhouettes and DBSCAN; tsne.hip: the neighbour graph).  256 threads, each thread a 4 x 4 block of pairs
// (queries ty + 16 r, columns tx + 16 c); KC columns of both row sets are staged in LDS per step.
// s_ij = sum_k (x_ik - x_jk)^2 accumulated by fma in column order: the same bits for (i, j) and (j, i), for any tiling.
#pragma once
#include "phk_common.h"

#define CL_T 64      // rows per tile side
#define CL_KC 16     // columns per LDS step
#define CL_PAD 1     // LDS row pad (doubles)
#define CL_THREADS 256
#define CL_MAX_BLOCKS (1ull << 22)   // workgroups per launch (x 256 threads < 2^32 work-items)

// Stage columns [k0, k0 + CL_KC) of 64 rows into S[k][r] (zero outside the matrix).  Row r of the tile is row
// idx[base + r] of X when idx is given, else row base + r; rows at or past `rows` load as zeros.
__device__ __forceinline__ void cl_stage(const double *__restrict__ X, uint64_t D, const int32_t *__restrict__ idx, uint64_t rows,
                                         uint64_t base, uint64_t k0, double (*S)[CL_T + CL_PAD]) {
    const int t = threadIdx.x, r = t >> 2, kq = (t & 3) * 4;
    const uint64_t g = base + r;
    const bool ok = g < rows;
    const uint64_t row = ok ? (idx ? (uint64_t)idx[g] : g) : 0;
    const double *p = X + row * D + k0 + kq;
#pragma unroll
    for (int i = 0; i < 4; ++i) S[kq + i][r] = (ok && k0 + kq + i < D) ? p[i] : 0.0;
}

// s[r][c] = sum over all D columns of (q - x)^2 for the thread's 16 pairs of the tile (query rows qbase.., column rows
// cbase..), in column order.
__device__ __forceinline__ void cl_tile(const double *__restrict__ X, uint64_t D, const int32_t *__restrict__ qidx, uint64_t qrows,
                                        uint64_t qbase, const int32_t *__restrict__ cidx, uint64_t crows, uint64_t cbase,
                                        double (*Qs)[CL_T + CL_PAD], double (*Cs)[CL_T + CL_PAD], double s[4][4]) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[r][c] = 0.0;
    for (uint64_t k0 = 0; k0 < D; k0 += CL_KC) {
        __syncthreads();
        cl_stage(X, D, qidx, qrows, qbase, k0, Qs);
        cl_stage(X, D, cidx, crows, cbase, k0, Cs);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CL_KC; ++k) {
            double q[4], x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = Qs[k][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = Cs[k][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = q[r] - x[c];
                    s[r][c] = fma(d, d, s[r][c]);
                }
        }
    }
}
