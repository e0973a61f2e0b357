// pair_tile.h -- the 64 x 64 pair tile of float64 chains shared by every exact all-pairs pass: the distance matrices of
// scoring and the nearest-reference fallback (score.hip), silhouettes and DBSCAN (cluster.hip), the neighbour graph and the
// PCA projection (tsne.hip), the k sweep (sweep.hip).  256 threads, each thread a 4 x 4 block of pairs (queries ty + 16 r,
// columns tx + 16 c); KC columns of both row sets are staged in LDS per step.
// CL_SQDIFF: s_ij = sum_k (q_ik - x_jk)^2 accumulated as acc = fma(q - x, q - x, acc) in column order -- the DIRECT-
// DIFFERENCE squared distance every exact answer is held to: the same bits for (i, j) and (j, i), for any tiling.
// CL_PRODUCT: s_ij = sum_k q_ik x_jk, acc = fma(q, x, acc), in the same order.
#pragma once
#include "phk_common.h"

#define CL_T 64      // rows per tile side
#define CL_KC 16     // columns per LDS step
#define CL_PAD 1     // LDS row pad (doubles)
#define CL_THREADS 256
#define CL_MAX_BLOCKS (1ull << 22)   // workgroups per launch (x 256 threads < 2^32 work-items)

enum ClOp { CL_SQDIFF, CL_PRODUCT };

// One side of a tile: row r of the tile is row idx[base + r] of X when idx is given, else row base + r; rows at or past
// `rows` are zeros.  (Passed by value: by reference phk_cl_count_kernel takes six more registers and loses a wave.)
struct ClSide {
    const double *X;
    const int32_t *idx;
    uint64_t rows, base;
};

// Stage columns [k0, k0 + CL_KC) of the side's 64 rows into S[k][r] (zero outside the matrix); with SHIFT, less shift[k].
template <bool SHIFT>
__device__ __forceinline__ void cl_stage(const ClSide a, uint64_t D, uint64_t k0, const double *__restrict__ shift,
                                         double (*S)[CL_T + CL_PAD]) {
    const int t = threadIdx.x, r = t >> 2, kq = (t & 3) * 4;
    const uint64_t g = a.base + r;
    const bool ok = g < a.rows;
    const uint64_t row = ok ? (a.idx ? (uint64_t)a.idx[g] : g) : 0;
    const double *p = a.X + row * D + k0 + kq;
    if constexpr (SHIFT) {   // (all eight loads before the first use: one wait per step)
        double v[4], m[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = ok && k0 + kq + i < D;
            v[i] = in ? p[i] : 0.0;
            m[i] = in ? shift[k0 + kq + i] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) S[kq + i][r] = v[i] - m[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) S[kq + i][r] = (ok && k0 + kq + i < D) ? p[i] : 0.0;
    }
}

// s[r][c] = the chain OP over all D columns for the thread's 16 pairs of the tile (query side q, column side c), in column
// order.  With SHIFT, shift[k] is subtracted from column k of the query side.
template <ClOp OP = CL_SQDIFF, bool SHIFT = false>
__device__ __forceinline__ void cl_tile(const ClSide q, const ClSide c, uint64_t D, double (*Qs)[CL_T + CL_PAD],
                                        double (*Cs)[CL_T + CL_PAD], double s[4][4], const double *__restrict__ shift = nullptr) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[r][j] = 0.0;
    for (uint64_t k0 = 0; k0 < D; k0 += CL_KC) {
        __syncthreads();
        cl_stage<SHIFT>(q, D, k0, shift, Qs);
        cl_stage<false>(c, D, k0, nullptr, Cs);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CL_KC; ++k) {
            double qv[4], xv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) qv[r] = Qs[k][ty + 16 * r];
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[j] = Cs[k][tx + 16 * j];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (OP == CL_PRODUCT) {
                        s[r][j] = fma(qv[r], xv[j], s[r][j]);
                    } else {
                        const double d = qv[r] - xv[j];
                        s[r][j] = fma(d, d, s[r][j]);
                    }
                }
        }
    }
}

// The tile written out as a matrix: out[i - 64 ytile0][j] = store(i, j, s_ij) for the query rows i < qrows of Q from tile
// row ytile0 on and the rows j < crows of X (out's first row is the first query row of the launch).  STORE's operator()
// gives the stored value.  grid (column tiles, query tiles of the launch).
template <class STORE, ClOp OP = CL_SQDIFF, bool SHIFT = false>
__global__ __launch_bounds__(CL_THREADS) void cl_matrix_kernel(const double *__restrict__ Q, uint64_t qrows, uint64_t ytile0,
                                                              const double *__restrict__ X, uint64_t crows, uint64_t D,
                                                              double *__restrict__ out, const double *__restrict__ shift) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t qbase = (ytile0 + blockIdx.y) * CL_T, cbase = (uint64_t)blockIdx.x * CL_T;
    double s[4][4];
    cl_tile<OP, SHIFT>({Q, nullptr, qrows, qbase}, {X, nullptr, crows, cbase}, D, Qs, Cs, s, shift);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t i = qbase + ty + 16 * r;
        if (i >= qrows) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t j = cbase + tx + 16 * c;
            if (j < crows) out[(i - ytile0 * CL_T) * crows + j] = STORE()(i, j, s[r][c]);
        }
    }
}

struct ClStoreValue {
    __device__ double operator()(uint64_t, uint64_t, double s) const { return s; }
};
