// mixture_body.h -- the bodies of the mixture E-step's three kernels, shared by the single-table kernels of
// mixture.hip and the stacked kernels of mixture_sweep.hip (4.25): one statement of the arithmetic, so that a job of a sweep
// and the single call give the same bits.  A body takes the indices a kernel would read from blockIdx as arguments; every
// argument is uniform over the workgroup.
#pragma once
#include "density_shared.h"
#include "gram_tile.h"

#define MIX_KMAX 256     // components: one chunk of the tile
#define MIX_RB 1024      // rows per reduction block
#define MIX_CT 64        // components and columns per wave of the expect kernel

// Row tile `tile` (GT_QB rows) of the count rows C[nq][D] against the table L[K][D], logw[Kp]: S, then r, into R[nq][Kp];
// l_i into row_ll.  ARGMAX: also the component of the largest r (lowest index on ties) and that r, into amax and rmax.
template <bool FULL, bool ARGMAX>
__device__ __forceinline__ void mix_resp_body(const uint32_t *__restrict__ C, uint64_t nq, uint64_t tile,
                                              const double *__restrict__ L, const double *__restrict__ logw, uint32_t K,
                                              uint32_t Kp, uint64_t D, double *R, double *__restrict__ row_ll,
                                              int32_t *__restrict__ amax, double *__restrict__ rmax) {
    const int li = threadIdx.x & 15, wave = threadIdx.x >> 6;
    const uint64_t q0 = tile * GT_QB + (uint64_t)wave * (GT_QT * 16);
    const double ninf = -__builtin_inf();

    double mx[GT_QT][4], sm[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[a][r] = ninf, sm[a][r] = 0.0;

    for (uint32_t st = 0; st < Kp; st += GT_RT * 16) {
        f64x4 acc[GT_QT][GT_RT];
        gram_tile<FULL, GT_QT, uint32_t>(C, nq, q0, L, K, st, D, acc);
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint32_t j = st + 16 * t + li;      // < Kp: the weights are padded with -inf
            const double w = logw[j];
            const bool live = w > ninf;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double e = acc[a][t][r] + w;
                    const double d = e - mx[a][r];
                    const double x = exp(-fabs(d));
                    const bool up = d > 0.0;
                    if (live) {
                        sm[a][r] = up ? fma(sm[a][r], x, 1.0) : sm[a][r] + x;
                        mx[a][r] = up ? e : mx[a][r];
                    }
                    const uint64_t q = gram_query(q0, a, r);
                    if (q < nq) R[q * Kp + j] = live ? e : ninf;
                }
        }
    }
    // the 16 lanes that share a row: fixed butterfly, every lane ends with the row's pair
    double ll[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const double m2 = __shfl_xor(mx[a][r], o), s2 = __shfl_xor(sm[a][r], o);
                kde_merge(mx[a][r], sm[a][r], m2, s2);
            }
            ll[a][r] = mx[a][r] + log(sm[a][r]);
        }
    // r = exp(S - l): every lane reads back what it wrote itself; the largest r of the row, lowest index on ties
    double best[GT_QT][4];
    int32_t bidx[GT_QT][4];
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) best[a][r] = -1.0, bidx[a][r] = 0x7fffffff;
    for (uint32_t st = 0; st < Kp; st += GT_RT * 16) {
#pragma unroll
        for (int t = 0; t < GT_RT; ++t) {
            const uint32_t j = st + 16 * t + li;
#pragma unroll
            for (int a = 0; a < GT_QT; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint64_t q = gram_query(q0, a, r);
                    if (q < nq) {
                        const double e = R[q * Kp + j];
                        const double p = e > ninf ? exp(e - ll[a][r]) : 0.0;
                        R[q * Kp + j] = p;
                        if (ARGMAX && j < K && p > best[a][r]) best[a][r] = p, bidx[a][r] = (int32_t)j;   // j rises: the first of equals stays
                    }
                }
        }
    }
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (ARGMAX) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const double b2 = __shfl_xor(best[a][r], o);
                    const int32_t i2 = __shfl_xor(bidx[a][r], o);
                    if (b2 > best[a][r] || (b2 == best[a][r] && i2 < bidx[a][r])) best[a][r] = b2, bidx[a][r] = i2;
                }
            }
            const uint64_t q = gram_query(q0, a, r);
            if (li == 0 && q < nq) {
                row_ll[q] = ll[a][r];
                if (ARGMAX) {
                    amax[q] = bidx[a][r];
                    rmax[q] = best[a][r];
                }
            }
        }
}

// Row block bx (MIX_RB rows) of R[nb][Kp], C[nb][D], row_ll[nb], group by of four column tiles (the wave takes column tile
// 4 by + wave), component tile bz, into the block's partial vector P: T[k][j] at k D + j, N_k at K D + k, L at K D + K.
// VEC: D % 4 == 0 (16-byte loads of the count rows).
template <bool VEC>
__device__ __forceinline__ void mix_expect_body(const double *__restrict__ R, uint32_t Kp, const uint32_t *__restrict__ C,
                                                uint64_t D, uint64_t nb, const double *__restrict__ row_ll, uint32_t K,
                                                uint32_t bx, uint32_t by, uint32_t bz, double *__restrict__ P) {
    const int li = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4, wave = threadIdx.x >> 6;
    const uint32_t c0 = bz * MIX_CT;
    const uint64_t j0 = ((uint64_t)by * GT_WAVES + wave) * MIX_CT;
    if (j0 >= D) return;   // (no barrier in this kernel)
    const uint64_t i0 = (uint64_t)bx * MIX_RB;
    const uint64_t i1 = i0 + MIX_RB < nb ? i0 + MIX_RB : nb;
    const bool tally = j0 == 0, tally_l = tally && c0 == 0;
    const uint64_t col = j0 + 4 * li;

    f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[a][t] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double nk[4] = {0.0, 0.0, 0.0, 0.0}, lsum = 0.0;

    for (uint64_t i = i0; i < i1; i += 4) {
        const uint64_t row = i + kk;
        const bool ok = row < i1;
        double ra[4] = {0.0, 0.0, 0.0, 0.0}, cb[4] = {0.0, 0.0, 0.0, 0.0};
        if (ok) {
            const double2 *p = (const double2 *)(R + row * Kp + c0 + 4 * li);
            const double2 r0 = p[0], r1 = p[1];
            ra[0] = r0.x, ra[1] = r0.y, ra[2] = r1.x, ra[3] = r1.y;
            if (VEC) {
                if (col < D) {
                    const uint4 c = *(const uint4 *)(C + row * D + col);
                    cb[0] = (double)c.x, cb[1] = (double)c.y, cb[2] = (double)c.z, cb[3] = (double)c.w;
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) cb[t] = col + t < D ? (double)C[row * D + col + t] : 0.0;
            }
        }
        if (tally) {
#pragma unroll
            for (int a = 0; a < 4; ++a) nk[a] += ra[a];
            if (tally_l && li == 0 && ok) lsum += row_ll[row];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[a][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[a], cb[t], acc[a][t], 0, 0, 0);
    }

#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t comp = c0 + 4 * (kk + 4 * r) + a;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (comp < K && col + t < D) P[(uint64_t)comp * D + col + t] = acc[a][t][r];
        }
    if (tally) {   // (wave-uniform) the four row slots of a step: (0 + 1) + (2 + 3)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            nk[a] += __shfl_xor(nk[a], 16);
            nk[a] += __shfl_xor(nk[a], 32);
            const uint32_t comp = c0 + 4 * li + a;
            if (kk == 0 && comp < K) P[(uint64_t)K * D + comp] = nk[a];
        }
        lsum += __shfl_xor(lsum, 16);
        lsum += __shfl_xor(lsum, 32);
        if (tally_l && (threadIdx.x & 63) == 0) P[(uint64_t)K * D + K] = lsum;
    }
}

// The tree of 4.23 over 256 consecutive partial vectors: v[i] += v[i + s] for s = 128, 64, .. 1 and v[0] is the result, i.e.
// g(i, S) = g(i, 2 S) + g(i + S, 2 S) over the indices congruent to i modulo S, g(i, 256) = v[i]; a vector past m is +0.0.
template <int S>
__device__ __forceinline__ double mix_tree(const double *__restrict__ in, uint64_t i, uint64_t m, uint64_t E) {
    if constexpr (S == 256) {
        return i < m ? in[i * E] : 0.0;
    } else {
        return mix_tree<2 * S>(in, i, m, E) + mix_tree<2 * S>(in, i + S, m, E);
    }
}

// Elements 256 ex .. 256 ex + 255 of out = the tree over the vectors in[256 vb .. 256 vb + 255] (m vectors of E doubles).  The
// sixteen subtrees g(i, 16) are taken one after another in the order the tree meets them (i = the 4-bit reversal of 0 .. 15)
// and joined as a binary counter carries: left operand = the earlier subtree, as in g(i, S) = g(i, 2 S) + g(i + S, 2 S).
__device__ __forceinline__ void mix_fold_body(const double *__restrict__ in, uint64_t m, uint64_t E, uint32_t ex, uint32_t vb,
                                              double *__restrict__ out) {
    const uint64_t e = (uint64_t)ex * 256 + threadIdx.x;
    if (e >= E) return;
    const uint64_t first = (uint64_t)vb * 256;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, result = 0.0;
#pragma clang loop unroll(disable)
    for (uint32_t n = 0; n < 16; ++n) {
        double v = mix_tree<16>(in + e, first + (__brev(n) >> 28), m, E);
        if (!(n & 1)) {
            a1 = v;
            continue;
        }
        v = a1 + v;
        if (!(n & 2)) {
            a2 = v;
            continue;
        }
        v = a2 + v;
        if (!(n & 4)) {
            a3 = v;
            continue;
        }
        v = a3 + v;
        if (!(n & 8)) {
            a4 = v;
            continue;
        }
        result = a4 + v;
    }
    out[e] = result;
}
