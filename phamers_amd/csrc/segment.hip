// segment.hip -- two-state hidden Markov decode of score tracks (gfx950): this project's own, DESIGN.md 4.22.
//
// Per record, over its windows t = 0 .. n-1: states 0 = host, 1 = phage; evidence x_t (a log-likelihood ratio in nats,
// tempered by the caller); emission e_t = (1, exp(x_t)); transition A, initial distribution pi.  Two recurrences with two
// contracts:
//
//   Viterbi, exact integers.  x_t, log A and log pi in units of 2^-PHK_SEG_QUANT_BITS nat (int64; x_t quantised here --
//   seg_quant -- the parameters by the caller).  Max-plus on integers is associative, so the scores delta_t are those of the
//   plain left-to-right recurrence whatever the tiling; the backpointers are taken FROM those scores (walk kernel), with
//   the recurrence's own tie rule (the smaller predecessor), so the path is the recurrence's too.
//
//   Forward-backward, float64 in the probability domain.  Every quantity is a sum of products of positive numbers (no
//   cancellation), rescaled by powers of two only (frexp / ldexp: exact), the exponent kept as an integer.  The emission of
//   a step is scaled by exp(-max(x_t, 0)): (1, exp(-|x|)) or (exp(-|x|), 1), so nothing overflows; the record's sum of
//   max(x_t, 0) is added back to log_odds.  A record is cut into tiles of PHK_SEG_TILE windows from its OWN start, and the
//   tile products are carried along the record in tile order by one lane: a record's result is a function of its x and the
//   parameters alone -- not of the call's other records, its place among them, or the launch.
//
// With M_t = A diag(e_t) (t >= 1) and M_0 = diag(e_0), the tile matrix F = M_first ... M_last serves both directions:
// alpha_last = alpha_before F (row vector, pi before the first tile), beta_before = F beta_last (column vector, (1, 1)
// after the last tile).
//
// Kernels (one lane per tile or per record; grids capped, grid-stride beyond -- phk_segment_grid_pass):
//   phk_seg_tile_kernel   lane per tile: F (scaled, + exponent), the max-plus tile matrix V, the tile's sum of max(x, 0)
//   phk_seg_carry_kernel  lane per record and chain: alpha entering every tile and log_odds; delta entering every tile,
//                         path_score and the last state (both left to right); beta leaving every tile (right to left)
//   phk_seg_walk_kernel   lane per tile: beta of every step into LDS (right to left), then alpha, the posterior, delta and
//                         the backpointers (left to right); the tile's path for either end state as 64 bits each, and the
//                         map end state -> state before the tile.  Posteriors leave through LDS, coalesced.
//   phk_seg_trace_kernel  lane per record: the state at every tile's end, right to left through the maps
//   phk_seg_state_kernel  thread per window: its bit of the tile's path
// and, for fitting A and pi (Baum-Welch; the tile kernel and the two sum-product chains are shared):
//   phk_seg_fb_carry_kernel  lane per record and chain: the two sum-product chains of the carry kernel alone
//   phk_seg_xi_kernel        lane per tile: beta into LDS, then alpha and every step's four pairwise posteriors, summed
//   phk_seg_fold_kernel      lane per record: its tiles' six sums in tile order
//   phk_seg_reduce_kernel    workgroup per 256 rows: one level of the fixed tree over the records
#include "phk_common.h"

#define SEG_T PHK_SEG_TILE
#define SEG_LD (SEG_T + 1)          // LDS row stride in doubles: the transposed read of the output pass hits 64 banks
#define SEG_BLOCKS_MAX 1024         // 64-lane workgroups per launch of the per-tile and per-record kernels
#define SEG_STATE_BLOCKS_MAX 4096   // 256-thread workgroups per launch of the per-window kernel
#define SEG_CLAMP 32768.0           // |x| the integer recurrence sees at most, nats
#define SEG_LN2 0.693147180559945309417232121458

static_assert(SEG_T == 64, "a tile's path and backpointers are the bits of one 64-bit word");

struct SegPar {
    double a00, a01, a10, a11, p0, p1;
    int64_t q00, q01, q10, q11, qp0, qp1;
};

struct SegTile {
    uint64_t w0;     // first window
    uint32_t len;    // windows, 1..SEG_T
    bool first;      // the record's first tile: its step 0 has no predecessor
};

__device__ __forceinline__ SegTile seg_tile(const uint64_t *__restrict__ off, const uint64_t *__restrict__ rec_tile0,
                                            const uint32_t *__restrict__ tile_rec, uint64_t g) {
    const uint32_t r = tile_rec[g];
    const uint64_t j = g - rec_tile0[r];
    SegTile t;
    t.w0 = off[r] + j * SEG_T;
    const uint64_t left = off[r + 1] - t.w0;
    t.len = (uint32_t)(left < SEG_T ? left : SEG_T);
    t.first = j == 0;
    return t;
}

// the step's emission scaled by exp(-max(x, 0)): the disfavoured state gets exp(-|x|) (0 below the format: "certain")
__device__ __forceinline__ void seg_emit(double x, double &e0, double &e1) {
    const double m = exp(-fabs(x));
    e0 = x > 0.0 ? m : 1.0;
    e1 = x > 0.0 ? 1.0 : m;
}

__device__ __forceinline__ int64_t seg_quant(double x) {
    return (int64_t)rint(fmin(fmax(x, -SEG_CLAMP), SEG_CLAMP) * (double)(1 << PHK_SEG_QUANT_BITS));
}

__device__ __forceinline__ int64_t seg_max(int64_t a, int64_t b) { return a > b ? a : b; }

// (a, b) / 2^e with e the exponent of the larger: exact; returns e
__device__ __forceinline__ int seg_scale2(double &a, double &b) {
    int e;
    (void)frexp(fmax(a, b), &e);
    a = ldexp(a, -e);
    b = ldexp(b, -e);
    return e;
}

__global__ __launch_bounds__(64) void phk_seg_tile_kernel(const double *__restrict__ x, const uint64_t *__restrict__ off,
                                                          const uint64_t *__restrict__ rec_tile0,
                                                          const uint32_t *__restrict__ tile_rec, uint64_t ntiles, SegPar P,
                                                          double *__restrict__ tF, int32_t *__restrict__ tE,
                                                          int64_t *__restrict__ tV, double *__restrict__ tS) {
    for (uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x; g < ntiles; g += (uint64_t)gridDim.x * 64) {
        const SegTile t = seg_tile(off, rec_tile0, tile_rec, g);
        double f00, f01, f10, f11, e0, e1;
        int64_t v00, v01, v10, v11;
        const double x0 = x[t.w0];
        const int64_t q0 = seg_quant(x0);
        seg_emit(x0, e0, e1);
        double sp = fmax(x0, 0.0);
        int32_t E = 0;
        if (t.first) {   // M_0 = diag(e_0); both rows of V hold the start vector (the carry enters with (0, 0))
            f00 = e0, f01 = 0.0, f10 = 0.0, f11 = e1;
            v00 = v10 = P.qp0, v01 = v11 = P.qp1 + q0;
        } else {
            f00 = P.a00 * e0, f01 = P.a01 * e1, f10 = P.a10 * e0, f11 = P.a11 * e1;
            v00 = P.q00, v01 = P.q01 + q0, v10 = P.q10, v11 = P.q11 + q0;
        }
        for (uint32_t i = 1; i < t.len; ++i) {
            const double xi = x[t.w0 + i];
            const int64_t q = seg_quant(xi);
            seg_emit(xi, e0, e1);
            sp += fmax(xi, 0.0);
            const double n00 = (f00 * P.a00 + f01 * P.a10) * e0, n01 = (f00 * P.a01 + f01 * P.a11) * e1;
            const double n10 = (f10 * P.a00 + f11 * P.a10) * e0, n11 = (f10 * P.a01 + f11 * P.a11) * e1;
            int e;
            (void)frexp(fmax(fmax(n00, n01), fmax(n10, n11)), &e);
            f00 = ldexp(n00, -e), f01 = ldexp(n01, -e), f10 = ldexp(n10, -e), f11 = ldexp(n11, -e);
            E += e;
            const int64_t m00 = seg_max(v00 + P.q00, v01 + P.q10), m01 = seg_max(v00 + P.q01, v01 + P.q11) + q;
            const int64_t m10 = seg_max(v10 + P.q00, v11 + P.q10), m11 = seg_max(v10 + P.q01, v11 + P.q11) + q;
            v00 = m00, v01 = m01, v10 = m10, v11 = m11;
        }
        tF[4 * g] = f00, tF[4 * g + 1] = f01, tF[4 * g + 2] = f10, tF[4 * g + 3] = f11;
        tV[4 * g] = v00, tV[4 * g + 1] = v01, tV[4 * g + 2] = v10, tV[4 * g + 3] = v11;
        tE[g] = E;
        tS[g] = sp;
    }
}

// The three chains of a record: one lane's loop over the record's tiles g0 .. g1 - 1 in tile order.  The loads do not depend
// on the chain's values, so the loops are unrolled for the loads of several tiles to be in flight (the arithmetic and its
// order are the plain loop's).
// forward sum-product: alpha entering every tile; returns log_odds
__device__ __forceinline__ double seg_chain_alpha(uint64_t g0, uint64_t g1, const SegPar &P, const double *__restrict__ tF,
                                                  const int32_t *__restrict__ tE, const double *__restrict__ tS,
                                                  double *__restrict__ tA) {
    double a0 = P.p0, a1 = P.p1, sp = 0.0;
    int64_t E = 0;
#pragma unroll 8
    for (uint64_t g = g0; g < g1; ++g) {
        tA[2 * g] = a0, tA[2 * g + 1] = a1;
        double n0 = a0 * tF[4 * g] + a1 * tF[4 * g + 2], n1 = a0 * tF[4 * g + 1] + a1 * tF[4 * g + 3];
        E += tE[g] + seg_scale2(n0, n1);
        a0 = n0, a1 = n1;
        sp += tS[g];
    }
    if (g1 == g0) return 0.0;   // a record without windows
    int e;
    const double m = frexp(a0 + a1, &e);
    return ((double)(E + e) * SEG_LN2 + log(m)) + sp;
}

// backward sum-product: beta leaving every tile (right to left)
__device__ __forceinline__ void seg_chain_beta(uint64_t g0, uint64_t g1, const double *__restrict__ tF,
                                               double *__restrict__ tB) {
    double b0 = 1.0, b1 = 1.0;
#pragma unroll 8
    for (uint64_t g = g1; g > g0; --g) {
        const uint64_t h = g - 1;
        tB[2 * h] = b0, tB[2 * h + 1] = b1;
        double n0 = tF[4 * h] * b0 + tF[4 * h + 1] * b1, n1 = tF[4 * h + 2] * b0 + tF[4 * h + 3] * b1;
        (void)seg_scale2(n0, n1);
        b0 = n0, b1 = n1;
    }
}

// grid: x = records (capped, grid-stride), y = chain: 0 forward sum-product (alpha entering every tile, log_odds),
// 1 forward max-plus (delta entering every tile, path_score, the last state), 2 backward sum-product (beta leaving every
// tile).
__global__ __launch_bounds__(64) void phk_seg_carry_kernel(const uint64_t *__restrict__ rec_tile0, uint64_t R, SegPar P,
                                                           const double *__restrict__ tF, const int32_t *__restrict__ tE,
                                                           const int64_t *__restrict__ tV, const double *__restrict__ tS,
                                                           double *__restrict__ tA, double *__restrict__ tB,
                                                           int64_t *__restrict__ tD, double *__restrict__ log_odds,
                                                           int64_t *__restrict__ path_score, uint8_t *__restrict__ rec_last) {
    for (uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 64) {
        const uint64_t g0 = rec_tile0[r], g1 = rec_tile0[r + 1];
        if (blockIdx.y == 0) {
            log_odds[r] = seg_chain_alpha(g0, g1, P, tF, tE, tS, tA);
        } else if (blockIdx.y == 1) {
            int64_t d0 = 0, d1 = 0;
#pragma unroll 8
            for (uint64_t g = g0; g < g1; ++g) {
                tD[2 * g] = d0, tD[2 * g + 1] = d1;
                const int64_t m0 = seg_max(d0 + tV[4 * g], d1 + tV[4 * g + 2]), m1 = seg_max(d0 + tV[4 * g + 1], d1 + tV[4 * g + 3]);
                d0 = m0, d1 = m1;
            }
            const bool one = g1 > g0 && d1 > d0;   // a tie at the final step goes to the smaller state
            path_score[r] = one ? d1 : d0;          // (0 for a record without windows)
            rec_last[r] = one ? 1 : 0;
        } else {
            seg_chain_beta(g0, g1, tF, tB);
        }
    }
}

// The fit's carry: the two sum-product chains alone (y = 0 forward, 1 backward); the max-plus chain is not run.
__global__ __launch_bounds__(64) void phk_seg_fb_carry_kernel(const uint64_t *__restrict__ rec_tile0, uint64_t R, SegPar P,
                                                              const double *__restrict__ tF, const int32_t *__restrict__ tE,
                                                              const double *__restrict__ tS, double *__restrict__ tA,
                                                              double *__restrict__ tB, double *__restrict__ log_odds) {
    for (uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 64) {
        const uint64_t g0 = rec_tile0[r], g1 = rec_tile0[r + 1];
        if (blockIdx.y == 0)
            log_odds[r] = seg_chain_alpha(g0, g1, P, tF, tE, tS, tA);
        else
            seg_chain_beta(g0, g1, tF, tB);
    }
}

// LDS: beta_t(0) and beta_t(1) of the block's 64 tiles, [step][lane] with rows of SEG_LD doubles (2 x 33 280 bytes); the
// posterior replaces beta_t(1) and the block then writes tile after tile, lane = step.
__global__ __launch_bounds__(64) void phk_seg_walk_kernel(const double *__restrict__ x, const uint64_t *__restrict__ off,
                                                          const uint64_t *__restrict__ rec_tile0,
                                                          const uint32_t *__restrict__ tile_rec, uint64_t ntiles, SegPar P,
                                                          const double *__restrict__ tA, const double *__restrict__ tB,
                                                          const int64_t *__restrict__ tD, double *__restrict__ posterior,
                                                          uint64_t *__restrict__ tPath, uint8_t *__restrict__ tMap) {
    __shared__ double sb0[SEG_T * SEG_LD], sb1[SEG_T * SEG_LD];
    __shared__ uint64_t sw0[64];
    __shared__ uint32_t slen[64];
    const int lane = threadIdx.x;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < ntiles; base += (uint64_t)gridDim.x * 64) {
        const uint64_t g = base + lane;
        SegTile t;
        t.w0 = 0, t.len = 0, t.first = false;
        if (g < ntiles) {
            t = seg_tile(off, rec_tile0, tile_rec, g);
            const int len = (int)t.len;
            double e0, e1;
            double b0 = tB[2 * g], b1 = tB[2 * g + 1];
            for (int i = len - 1; i >= 0; --i) {
                sb0[i * SEG_LD + lane] = b0;
                sb1[i * SEG_LD + lane] = b1;
                if (i > 0) {   // beta_{t-1} = A (e_t o beta_t)
                    seg_emit(x[t.w0 + i], e0, e1);
                    const double u0 = e0 * b0, u1 = e1 * b1;
                    b0 = P.a00 * u0 + P.a01 * u1;
                    b1 = P.a10 * u0 + P.a11 * u1;
                    (void)seg_scale2(b0, b1);
                }
            }
            double a0 = tA[2 * g], a1 = tA[2 * g + 1];
            int64_t d0 = tD[2 * g], d1 = tD[2 * g + 1];
            uint64_t bp0 = 0, bp1 = 0;   // bit i: the predecessor of state 0 / 1 at the tile's step i
            for (int i = 0; i < len; ++i) {
                const double xi = x[t.w0 + i];
                const int64_t q = seg_quant(xi);
                seg_emit(xi, e0, e1);
                if (i == 0 && t.first) {
                    a0 *= e0, a1 *= e1;
                    d0 = P.qp0, d1 = P.qp1 + q;
                } else {
                    const double n0 = (a0 * P.a00 + a1 * P.a10) * e0, n1 = (a0 * P.a01 + a1 * P.a11) * e1;
                    a0 = n0, a1 = n1;
                    const int64_t c00 = d0 + P.q00, c10 = d1 + P.q10, c01 = d0 + P.q01, c11 = d1 + P.q11;
                    const bool k0 = c10 > c00, k1 = c11 > c01;   // a tie goes to predecessor 0
                    d0 = k0 ? c10 : c00;
                    d1 = (k1 ? c11 : c01) + q;
                    bp0 |= (uint64_t)k0 << i;
                    bp1 |= (uint64_t)k1 << i;
                }
                (void)seg_scale2(a0, a1);
                const double p0 = a0 * sb0[i * SEG_LD + lane], p1 = a1 * sb1[i * SEG_LD + lane];
                sb1[i * SEG_LD + lane] = p1 / (p0 + p1);
            }
            uint32_t map = 0;
            for (int end = 0; end < 2; ++end) {   // the tile's path for either state at its last step
                uint32_t s = (uint32_t)end;
                uint64_t word = (uint64_t)s << (len - 1);
                for (int i = len - 1; i > 0; --i) {
                    s = (uint32_t)(((s ? bp1 : bp0) >> i) & 1);
                    word |= (uint64_t)s << (i - 1);
                }
                map |= (uint32_t)(((s ? bp1 : bp0) & 1) << end);
                tPath[2 * g + end] = word;
            }
            tMap[g] = (uint8_t)map;
        }
        sw0[lane] = t.w0;
        slen[lane] = t.len;
        __syncthreads();
        for (int l = 0; l < 64; ++l)
            if ((uint32_t)lane < slen[l]) posterior[sw0[l] + lane] = sb1[lane * SEG_LD + l];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void phk_seg_trace_kernel(const uint64_t *__restrict__ rec_tile0, uint64_t R,
                                                           const uint8_t *__restrict__ rec_last,
                                                           const uint8_t *__restrict__ tMap, uint8_t *__restrict__ tEnd) {
    for (uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 64) {
        const uint64_t g0 = rec_tile0[r];
        uint32_t s = rec_last[r];
#pragma unroll 16
        for (uint64_t g = rec_tile0[r + 1]; g > g0; --g) {
            tEnd[g - 1] = (uint8_t)s;
            s = (tMap[g - 1] >> s) & 1u;
        }
    }
}

__global__ __launch_bounds__(256) void phk_seg_state_kernel(const uint64_t *__restrict__ off,
                                                            const uint64_t *__restrict__ rec_tile0,
                                                            const uint32_t *__restrict__ tile_rec, uint64_t ntiles,
                                                            const uint64_t *__restrict__ tPath,
                                                            const uint8_t *__restrict__ tEnd, uint8_t *__restrict__ state) {
    const uint64_t total = ntiles * SEG_T;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256) {
        const uint64_t g = idx / SEG_T;
        const uint32_t i = (uint32_t)(idx % SEG_T);
        const SegTile t = seg_tile(off, rec_tile0, tile_rec, g);
        if (i < t.len) state[t.w0 + i] = (uint8_t)((tPath[2 * g + tEnd[g]] >> i) & 1);
    }
}

// ---- the E-step of the fit ---------------------------------------------------------------------------------
// Lane per tile, as the walk kernel: beta of every step into LDS [step][lane] (2 x 32 768 bytes; a lane reads its own
// column only, so no barrier and no padding), then alpha left to right.  A step t >= 1 has the four terms
// w_ij = alpha_{t-1}(i) A_ij e_t(j) beta_t(j), normalised by their own sum -- whatever powers of two alpha and beta carry
// cancel there -- and added, in step order, to the tile's xi(i -> j); the record's step 0 adds alpha_0(s) beta_0(s),
// normalised likewise, to gamma_0(s).  tX[6 g ..] = xi00, xi01, xi10, xi11, gamma_0(0), gamma_0(1) of tile g.
__global__ __launch_bounds__(64) void phk_seg_xi_kernel(const double *__restrict__ x, const uint64_t *__restrict__ off,
                                                        const uint64_t *__restrict__ rec_tile0,
                                                        const uint32_t *__restrict__ tile_rec, uint64_t ntiles, SegPar P,
                                                        const double *__restrict__ tA, const double *__restrict__ tB,
                                                        double *__restrict__ tX) {
    __shared__ double sb0[SEG_T * 64], sb1[SEG_T * 64];
    const int lane = threadIdx.x;
    for (uint64_t g = (uint64_t)blockIdx.x * 64 + lane; g < ntiles; g += (uint64_t)gridDim.x * 64) {
        const SegTile t = seg_tile(off, rec_tile0, tile_rec, g);
        const int len = (int)t.len;
        double e0, e1;
        double b0 = tB[2 * g], b1 = tB[2 * g + 1];
        for (int i = len - 1; i >= 0; --i) {
            sb0[i * 64 + lane] = b0;
            sb1[i * 64 + lane] = b1;
            if (i > 0) {   // beta_{t-1} = A (e_t o beta_t)
                seg_emit(x[t.w0 + i], e0, e1);
                const double u0 = e0 * b0, u1 = e1 * b1;
                b0 = P.a00 * u0 + P.a01 * u1;
                b1 = P.a10 * u0 + P.a11 * u1;
                (void)seg_scale2(b0, b1);
            }
        }
        double a0 = tA[2 * g], a1 = tA[2 * g + 1];   // alpha before the tile's first step (pi for the record's first)
        double x00 = 0.0, x01 = 0.0, x10 = 0.0, x11 = 0.0, g0 = 0.0, g1 = 0.0;
        for (int i = 0; i < len; ++i) {
            seg_emit(x[t.w0 + i], e0, e1);
            const double c0 = e0 * sb0[i * 64 + lane], c1 = e1 * sb1[i * 64 + lane];
            if (i == 0 && t.first) {
                const double p0 = a0 * c0, p1 = a1 * c1;
                const double inv = 1.0 / (p0 + p1);
                g0 = p0 * inv, g1 = p1 * inv;
                a0 *= e0, a1 *= e1;
            } else {
                const double w00 = (a0 * P.a00) * c0, w01 = (a0 * P.a01) * c1;
                const double w10 = (a1 * P.a10) * c0, w11 = (a1 * P.a11) * c1;
                const double inv = 1.0 / ((w00 + w01) + (w10 + w11));
                x00 += w00 * inv, x01 += w01 * inv, x10 += w10 * inv, x11 += w11 * inv;
                const double n0 = (a0 * P.a00 + a1 * P.a10) * e0, n1 = (a0 * P.a01 + a1 * P.a11) * e1;
                a0 = n0, a1 = n1;
            }
            (void)seg_scale2(a0, a1);
        }
        double *out = tX + 6 * g;
        out[0] = x00, out[1] = x01, out[2] = x10, out[3] = x11, out[4] = g0, out[5] = g1;
    }
}

// lane per record: the six sums of its tiles, in tile order (zeros for a record without windows).  As in the carry kernel
// the loads do not depend on the sums: the loop is unrolled for the loads of 16 tiles to be in flight.
__global__ __launch_bounds__(64) void phk_seg_fold_kernel(const uint64_t *__restrict__ rec_tile0, uint64_t R,
                                                          const double *__restrict__ tX, double *__restrict__ counts_rec) {
    for (uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 64) {
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 16
        for (uint64_t g = rec_tile0[r]; g < rec_tile0[r + 1]; ++g)
#pragma unroll
            for (int c = 0; c < 6; ++c) s[c] += tX[6 * g + c];
#pragma unroll
        for (int c = 0; c < 6; ++c) counts_rec[6 * r + c] = s[c];
    }
}

// One level of the reduction over records: rows 256 b .. 256 b + 255 of (in6[m][6], in1[m]) -> row b of (out6, out1).  A
// row past m counts as +0.0; within a block, seven columns side by side, v[i] += v[i + s] for s = 128, 64, .. 1.  The tree is
// fixed by the row index alone; the grid only decides which workgroup takes which block.
#define SEG_RED 256
__global__ __launch_bounds__(SEG_RED) void phk_seg_reduce_kernel(const double *__restrict__ in6, const double *__restrict__ in1,
                                                                 uint64_t m, double *__restrict__ out6,
                                                                 double *__restrict__ out1) {
    __shared__ double s[7][SEG_RED];
    const int t = threadIdx.x;
    const uint64_t blocks = (m + SEG_RED - 1) / SEG_RED;
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t i = b * SEG_RED + t;
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c][t] = i < m ? in6[6 * i + c] : 0.0;
        s[6][t] = i < m ? in1[i] : 0.0;
        __syncthreads();
        for (int stride = SEG_RED / 2; stride > 0; stride >>= 1) {
            if (t < stride) {
#pragma unroll
                for (int c = 0; c < 7; ++c) s[c][t] += s[c][t + stride];
            }
            __syncthreads();
        }
        if (t < 6) out6[6 * b + t] = s[t][0];
        if (t == 6) out1[b] = s[6][0];
        __syncthreads();
    }
}

extern "C" uint64_t phk_segment_grid_pass(void) { return (uint64_t)SEG_BLOCKS_MAX * 64; }

static inline unsigned seg_grid(uint64_t items, uint64_t per_block, uint64_t cap) {
    const uint64_t b = phk_div_up(items, per_block);
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// The device half of a call: workspace, uploads, the five launches, the four results to the host.  rec_tile0[R + 1] = the
// first tile of every record, tile_rec[nt] = the record of every tile (host arrays of the caller).
static int seg_run(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, const uint64_t *rec_tile0,
                   const uint32_t *tile_rec, uint64_t nt, const SegPar &P, double *posterior, uint8_t *state, double *log_odds,
                   int64_t *path_score) {
    PhkLayout lay;
    const uint64_t o_x = lay.take(n * 8), o_post = lay.take(n * 8), o_state = lay.take(n);
    const uint64_t o_off = lay.take((R + 1) * 8), o_rt0 = lay.take((R + 1) * 8), o_trec = lay.take(nt * 4);
    const uint64_t o_F = lay.take(nt * 32), o_V = lay.take(nt * 32), o_E = lay.take(nt * 4), o_S = lay.take(nt * 8);
    const uint64_t o_A = lay.take(nt * 16), o_B = lay.take(nt * 16), o_D = lay.take(nt * 16), o_path = lay.take(nt * 16);
    const uint64_t o_map = lay.take(nt), o_end = lay.take(nt);
    const uint64_t o_lo = lay.take(R * 8), o_ps = lay.take(R * 8), o_last = lay.take(R);
    void *ws;
    PHK_TRY(phk_ws(ctx, WS_SEG, lay.bytes, &ws));
    char *w = (char *)ws;
    double *d_x = (double *)(w + o_x), *d_post = (double *)(w + o_post);
    uint8_t *d_state = (uint8_t *)(w + o_state);
    uint64_t *d_off = (uint64_t *)(w + o_off), *d_rt0 = (uint64_t *)(w + o_rt0);
    uint32_t *d_trec = (uint32_t *)(w + o_trec);
    double *d_F = (double *)(w + o_F), *d_S = (double *)(w + o_S), *d_A = (double *)(w + o_A), *d_B = (double *)(w + o_B);
    int64_t *d_V = (int64_t *)(w + o_V), *d_D = (int64_t *)(w + o_D);
    int32_t *d_E = (int32_t *)(w + o_E);
    uint64_t *d_path = (uint64_t *)(w + o_path);
    uint8_t *d_map = (uint8_t *)(w + o_map), *d_end = (uint8_t *)(w + o_end), *d_last = (uint8_t *)(w + o_last);
    double *d_lo = (double *)(w + o_lo);
    int64_t *d_ps = (int64_t *)(w + o_ps);

    PHK_TRY(phk_copy_to_device(ctx, d_x, x, n * 8));
    PHK_TRY(phk_copy_to_device(ctx, d_off, offsets, (R + 1) * 8));
    PHK_TRY(phk_copy_to_device(ctx, d_rt0, rec_tile0, (R + 1) * 8));
    PHK_TRY(phk_copy_to_device(ctx, d_trec, tile_rec, nt * 4));
    const unsigned tile_blocks = seg_grid(nt, 64, SEG_BLOCKS_MAX), rec_blocks = seg_grid(R, 64, SEG_BLOCKS_MAX);
    PHK_LAUNCH(ctx, "phk_seg_tile_kernel", phk_seg_tile_kernel<<<dim3(tile_blocks), dim3(64), 0, ctx->stream>>>(
                                               d_x, d_off, d_rt0, d_trec, nt, P, d_F, d_E, d_V, d_S));
    PHK_LAUNCH(ctx, "phk_seg_carry_kernel", phk_seg_carry_kernel<<<dim3(rec_blocks, 3), dim3(64), 0, ctx->stream>>>(
                                                d_rt0, R, P, d_F, d_E, d_V, d_S, d_A, d_B, d_D, d_lo, d_ps, d_last));
    PHK_LAUNCH(ctx, "phk_seg_walk_kernel", phk_seg_walk_kernel<<<dim3(tile_blocks), dim3(64), 0, ctx->stream>>>(
                                               d_x, d_off, d_rt0, d_trec, nt, P, d_A, d_B, d_D, d_post, d_path, d_map));
    PHK_LAUNCH(ctx, "phk_seg_trace_kernel",
               phk_seg_trace_kernel<<<dim3(rec_blocks), dim3(64), 0, ctx->stream>>>(d_rt0, R, d_last, d_map, d_end));
    PHK_LAUNCH(ctx, "phk_seg_state_kernel",
               phk_seg_state_kernel<<<dim3(seg_grid(nt * SEG_T, 256, SEG_STATE_BLOCKS_MAX)), dim3(256), 0, ctx->stream>>>(
                   d_off, d_rt0, d_trec, nt, d_path, d_end, d_state));
    PHK_TRY(phk_copy_to_host(ctx, posterior, d_post, n * 8));
    PHK_TRY(phk_copy_to_host(ctx, state, d_state, n));
    PHK_TRY(phk_copy_to_host(ctx, log_odds, d_lo, R * 8));
    return phk_copy_to_host(ctx, path_score, d_ps, R * 8);
}

static bool seg_prob(double p) { return p > 0.0 && p < 1.0; }
static bool seg_sums_to_one(double a, double b) { return fabs((a + b) - 1.0) <= 4.0 * 0x1p-52; }

extern "C" int phk_segment_decode(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R,
                                  const double trans[4], const double init[2], const int64_t qlog_trans[4],
                                  const int64_t qlog_init[2], double *posterior, uint8_t *state, double *log_odds,
                                  int64_t *path_score) {
    PHK_ENTER(ctx, "phk_segment_decode");
    PHK_REQUIRE(trans && init && qlog_trans && qlog_init, "phk_segment_decode: NULL parameters");
    for (int i = 0; i < 4; ++i)
        PHK_REQUIRE(seg_prob(trans[i]), "phk_segment_decode: transition probability %d = %g is not in (0, 1)", i, trans[i]);
    for (int i = 0; i < 2; ++i)
        PHK_REQUIRE(seg_prob(init[i]), "phk_segment_decode: initial probability %d = %g is not in (0, 1)", i, init[i]);
    PHK_REQUIRE(seg_sums_to_one(trans[0], trans[1]) && seg_sums_to_one(trans[2], trans[3]),
                "phk_segment_decode: a row of the transition matrix does not sum to 1");
    PHK_REQUIRE(seg_sums_to_one(init[0], init[1]), "phk_segment_decode: the initial distribution does not sum to 1");
    PHK_REQUIRE(n <= (1ull << 31) && R < (1ull << 32), "phk_segment_decode: more than 2^31 windows or 2^32 records in one call");
    if (R == 0) {
        PHK_REQUIRE(n == 0, "phk_segment_decode: %llu windows and no record", (unsigned long long)n);
        return PHK_OK;
    }
    PHK_REQUIRE(offsets && log_odds && path_score, "phk_segment_decode: NULL pointer");
    PHK_REQUIRE(offsets[0] == 0 && offsets[R] == n, "phk_segment_decode: the offsets do not run from 0 to n");
    for (uint64_t r = 0; r < R; ++r)
        PHK_REQUIRE(offsets[r] <= offsets[r + 1], "phk_segment_decode: the offsets decrease at record %llu", (unsigned long long)r);
    if (n == 0) {
        for (uint64_t r = 0; r < R; ++r) log_odds[r] = 0.0, path_score[r] = 0;
        return PHK_OK;
    }
    PHK_REQUIRE(x && posterior && state, "phk_segment_decode: NULL pointer");
    if (!phk_rows_finite(x, n)) {
        phk_set_error("phk_segment_decode: the evidence holds a value that is not finite");
        return PHK_ERR_NAN;
    }
    std::vector<uint64_t> rec_tile0(R + 1);
    rec_tile0[0] = 0;
    for (uint64_t r = 0; r < R; ++r) rec_tile0[r + 1] = rec_tile0[r] + phk_div_up(offsets[r + 1] - offsets[r], SEG_T);
    const uint64_t nt = rec_tile0[R];
    std::vector<uint32_t> tile_rec(nt);
    for (uint64_t r = 0; r < R; ++r)
        for (uint64_t g = rec_tile0[r]; g < rec_tile0[r + 1]; ++g) tile_rec[g] = (uint32_t)r;

    SegPar P;
    P.a00 = trans[0], P.a01 = trans[1], P.a10 = trans[2], P.a11 = trans[3], P.p0 = init[0], P.p1 = init[1];
    P.q00 = qlog_trans[0], P.q01 = qlog_trans[1], P.q10 = qlog_trans[2], P.q11 = qlog_trans[3];
    P.qp0 = qlog_init[0], P.qp1 = qlog_init[1];
    // the copies back wait for the stream, so the uploads have read the two vectors by then; a call that fails half way
    // drains the stream before they go
    const int rc = seg_run(ctx, x, n, offsets, R, rec_tile0.data(), tile_rec.data(), nt, P, posterior, state, log_odds, path_score);
    if (rc != PHK_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// ---- the fit: expected counts (E-step) and the Baum-Welch loop ---------------------------------------------
// What a fit keeps on the device: the evidence, the offsets and the tile lists go up once (seg_fit_setup); every E-step
// (seg_fit_estep) launches tile -> carry -> xi -> fold -> reduce on them and brings back seven numbers.
struct SegFit {
    uint64_t n = 0, R = 0, nt = 0;
    double *x, *F, *S, *A, *B, *X, *lo, *crec, *red6[2], *red1[2], *tot;
    uint64_t *off, *rt0;
    uint32_t *trec;
    int64_t *V;
    int32_t *E;
};

static int seg_fit_setup(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, SegFit &W) {
    std::vector<uint64_t> rec_tile0(R + 1);
    rec_tile0[0] = 0;
    for (uint64_t r = 0; r < R; ++r) rec_tile0[r + 1] = rec_tile0[r] + phk_div_up(offsets[r + 1] - offsets[r], SEG_T);
    const uint64_t nt = rec_tile0[R];
    std::vector<uint32_t> tile_rec(nt);
    for (uint64_t r = 0; r < R; ++r)
        for (uint64_t g = rec_tile0[r]; g < rec_tile0[r + 1]; ++g) tile_rec[g] = (uint32_t)r;
    W.n = n, W.R = R, W.nt = nt;
    const uint64_t m1 = phk_div_up(R, SEG_RED), m2 = phk_div_up(m1, SEG_RED);   // rows after the first two levels
    PhkLayout lay;
    const uint64_t o_x = lay.take(n * 8), o_off = lay.take((R + 1) * 8), o_rt0 = lay.take((R + 1) * 8), o_trec = lay.take(nt * 4);
    const uint64_t o_F = lay.take(nt * 32), o_V = lay.take(nt * 32), o_E = lay.take(nt * 4), o_S = lay.take(nt * 8);
    const uint64_t o_A = lay.take(nt * 16), o_B = lay.take(nt * 16), o_X = lay.take(nt * 48);
    const uint64_t o_lo = lay.take(R * 8), o_crec = lay.take(R * 48);
    const uint64_t o_r60 = lay.take(m1 * 48), o_r10 = lay.take(m1 * 8), o_r61 = lay.take(m2 * 48), o_r11 = lay.take(m2 * 8);
    const uint64_t o_tot = lay.take(7 * 8);
    void *ws;
    PHK_TRY(phk_ws(ctx, WS_SEG, lay.bytes, &ws));
    char *w = (char *)ws;
    W.x = (double *)(w + o_x), W.off = (uint64_t *)(w + o_off), W.rt0 = (uint64_t *)(w + o_rt0), W.trec = (uint32_t *)(w + o_trec);
    W.F = (double *)(w + o_F), W.V = (int64_t *)(w + o_V), W.E = (int32_t *)(w + o_E), W.S = (double *)(w + o_S);
    W.A = (double *)(w + o_A), W.B = (double *)(w + o_B), W.X = (double *)(w + o_X);
    W.lo = (double *)(w + o_lo), W.crec = (double *)(w + o_crec), W.tot = (double *)(w + o_tot);
    W.red6[0] = (double *)(w + o_r60), W.red1[0] = (double *)(w + o_r10);
    W.red6[1] = (double *)(w + o_r61), W.red1[1] = (double *)(w + o_r11);
    PHK_TRY(phk_copy_to_device(ctx, W.x, x, n * 8));
    PHK_TRY(phk_copy_to_device(ctx, W.off, offsets, (R + 1) * 8));
    PHK_TRY(phk_copy_to_device(ctx, W.rt0, rec_tile0.data(), (R + 1) * 8));
    PHK_TRY(phk_copy_to_device(ctx, W.trec, tile_rec.data(), nt * 4));
    // the two host vectors leave scope with this call: the uploads have read them once the stream is idle
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    return PHK_OK;
}

// totals[0..5] = the sums of counts_rec over the records, totals[6] = the sum of log_odds, both by the tree of
// phk_seg_reduce_kernel applied level after level until one row is left (that row lands in W.tot).
static int seg_fit_estep(phk_ctx *ctx, const SegFit &W, const double trans[4], const double init[2], double totals[7]) {
    SegPar P;
    P.a00 = trans[0], P.a01 = trans[1], P.a10 = trans[2], P.a11 = trans[3], P.p0 = init[0], P.p1 = init[1];
    P.q00 = P.q01 = P.q10 = P.q11 = P.qp0 = P.qp1 = 0;   // the max-plus products of the tile kernel are not read here
    const unsigned tile_blocks = seg_grid(W.nt, 64, SEG_BLOCKS_MAX), rec_blocks = seg_grid(W.R, 64, SEG_BLOCKS_MAX);
    PHK_LAUNCH(ctx, "phk_seg_tile_kernel", phk_seg_tile_kernel<<<dim3(tile_blocks), dim3(64), 0, ctx->stream>>>(
                                               W.x, W.off, W.rt0, W.trec, W.nt, P, W.F, W.E, W.V, W.S));
    PHK_LAUNCH(ctx, "phk_seg_fb_carry_kernel", phk_seg_fb_carry_kernel<<<dim3(rec_blocks, 2), dim3(64), 0, ctx->stream>>>(
                                                   W.rt0, W.R, P, W.F, W.E, W.S, W.A, W.B, W.lo));
    PHK_LAUNCH(ctx, "phk_seg_xi_kernel", phk_seg_xi_kernel<<<dim3(tile_blocks), dim3(64), 0, ctx->stream>>>(
                                             W.x, W.off, W.rt0, W.trec, W.nt, P, W.A, W.B, W.X));
    PHK_LAUNCH(ctx, "phk_seg_fold_kernel",
               phk_seg_fold_kernel<<<dim3(rec_blocks), dim3(64), 0, ctx->stream>>>(W.rt0, W.R, W.X, W.crec));
    const double *in6 = W.crec, *in1 = W.lo;
    uint64_t m = W.R;
    for (int level = 0;; ++level) {
        const uint64_t blocks = phk_div_up(m, SEG_RED);
        double *out6 = blocks == 1 ? W.tot : W.red6[level & 1], *out1 = blocks == 1 ? W.tot + 6 : W.red1[level & 1];
        PHK_LAUNCH(ctx, "phk_seg_reduce_kernel",
                   phk_seg_reduce_kernel<<<dim3(seg_grid(blocks, 1, SEG_BLOCKS_MAX)), dim3(SEG_RED), 0, ctx->stream>>>(
                       in6, in1, m, out6, out1));
        if (blocks == 1) break;
        in6 = out6, in1 = out1, m = blocks;
    }
    return phk_copy_to_host(ctx, totals, W.tot, 7 * 8);
}

// the argument checks of phk_segment_decode, for the two entry points below; *empty: nothing to launch (R == 0 or n == 0)
static int seg_fit_check(const char *who, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, const double trans[4],
                         const double init[2], bool *empty) {
    for (int i = 0; i < 4; ++i)
        PHK_REQUIRE(seg_prob(trans[i]), "%s: transition probability %d = %g is not in (0, 1)", who, i, trans[i]);
    for (int i = 0; i < 2; ++i) PHK_REQUIRE(seg_prob(init[i]), "%s: initial probability %d = %g is not in (0, 1)", who, i, init[i]);
    PHK_REQUIRE(seg_sums_to_one(trans[0], trans[1]) && seg_sums_to_one(trans[2], trans[3]),
                "%s: a row of the transition matrix does not sum to 1", who);
    PHK_REQUIRE(seg_sums_to_one(init[0], init[1]), "%s: the initial distribution does not sum to 1", who);
    PHK_REQUIRE(n <= (1ull << 31) && R < (1ull << 32), "%s: more than 2^31 windows or 2^32 records in one call", who);
    *empty = true;
    if (R == 0) {
        PHK_REQUIRE(n == 0, "%s: %llu windows and no record", who, (unsigned long long)n);
        return PHK_OK;
    }
    PHK_REQUIRE(offsets, "%s: NULL pointer", who);
    PHK_REQUIRE(offsets[0] == 0 && offsets[R] == n, "%s: the offsets do not run from 0 to n", who);
    for (uint64_t r = 0; r < R; ++r)
        PHK_REQUIRE(offsets[r] <= offsets[r + 1], "%s: the offsets decrease at record %llu", who, (unsigned long long)r);
    if (n == 0) return PHK_OK;
    PHK_REQUIRE(x, "%s: NULL pointer", who);
    if (!phk_rows_finite(x, n)) {
        phk_set_error("%s: the evidence holds a value that is not finite", who);
        return PHK_ERR_NAN;
    }
    *empty = false;
    return PHK_OK;
}

static int seg_expect_run(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, const double trans[4],
                          const double init[2], double *counts_rec, double tot[7], double *log_odds) {
    SegFit W;
    PHK_TRY(seg_fit_setup(ctx, x, n, offsets, R, W));
    PHK_TRY(seg_fit_estep(ctx, W, trans, init, tot));
    if (counts_rec) PHK_TRY(phk_copy_to_host(ctx, counts_rec, W.crec, R * 48));
    if (log_odds) PHK_TRY(phk_copy_to_host(ctx, log_odds, W.lo, R * 8));
    return PHK_OK;
}

extern "C" int phk_segment_expect(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R,
                                  const double trans[4], const double init[2], double *counts_rec, double totals[6],
                                  double *log_odds, double *log_evidence) {
    PHK_ENTER(ctx, "phk_segment_expect");
    PHK_REQUIRE(trans && init && totals && log_evidence, "phk_segment_expect: NULL pointer");
    bool empty;
    PHK_TRY(seg_fit_check("phk_segment_expect", x, n, offsets, R, trans, init, &empty));
    double tot[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (empty) {
        for (uint64_t i = 0; counts_rec && i < 6 * R; ++i) counts_rec[i] = 0.0;
        for (uint64_t r = 0; log_odds && r < R; ++r) log_odds[r] = 0.0;
    } else {
        const int rc = seg_expect_run(ctx, x, n, offsets, R, trans, init, counts_rec, tot, log_odds);
        if (rc != PHK_OK) {
            (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
    }
    for (int c = 0; c < 6; ++c) totals[c] = tot[c];
    *log_evidence = tot[6];
    return PHK_OK;
}

static const double SEG_P_MIN = 1e-12, SEG_P_MAX = 1.0 - 1e-12;

static double seg_fit_clamp(double p, uint32_t *status) {
    if (p < SEG_P_MIN) *status |= PHK_SEG_FIT_CLAMPED, p = SEG_P_MIN;
    if (p > SEG_P_MAX) *status |= PHK_SEG_FIT_CLAMPED, p = SEG_P_MAX;
    return p;
}

// the M-step, in place on par = {a, b, p_start}; every operation is one IEEE addition or division
static void seg_fit_mstep(const double tot[7], const double prior[4], int start_mode, double par[3], uint32_t *status) {
    const double n00 = tot[0] + prior[0], n01 = tot[1] + prior[1], n10 = tot[2] + prior[2], n11 = tot[3] + prior[3];
    if (n00 + n01 > 0.0)
        par[0] = seg_fit_clamp(n01 / (n00 + n01), status);
    else
        *status |= PHK_SEG_FIT_NO_TRANSITIONS;
    if (n10 + n11 > 0.0)
        par[1] = seg_fit_clamp(n10 / (n10 + n11), status);
    else
        *status |= PHK_SEG_FIT_NO_TRANSITIONS;
    if (start_mode == PHK_SEG_START_FREE) {
        if (tot[4] + tot[5] > 0.0) par[2] = seg_fit_clamp(tot[5] / (tot[4] + tot[5]), status);
    } else if (start_mode == PHK_SEG_START_STATIONARY) {
        par[2] = seg_fit_clamp(par[0] / (par[0] + par[1]), status);
    }
}

static int seg_fit_run(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R, bool empty, int start_mode,
                       const double prior[4], uint32_t max_iter, double tol, double par[3], double *trace, uint32_t *n_iter,
                       uint32_t *status) {
    SegFit W;
    if (!empty) PHK_TRY(seg_fit_setup(ctx, x, n, offsets, R, W));
    uint32_t i = 0;
    for (;;) {
        double *row = trace + (uint64_t)i * PHK_SEG_TRACE_COLS;
        const double trans[4] = {1.0 - par[0], par[0], par[1], 1.0 - par[1]}, init[2] = {1.0 - par[2], par[2]};
        row[0] = par[0], row[1] = par[1], row[2] = par[2];
        for (int c = 0; c < 7; ++c) row[3 + c] = 0.0;
        if (!empty) PHK_TRY(seg_fit_estep(ctx, W, trans, init, row + 3));
        if (i > 0 && row[9] - row[9 - PHK_SEG_TRACE_COLS] <= tol * fmax(1.0, fabs(row[9]))) {
            *status |= PHK_SEG_FIT_CONVERGED;
            break;
        }
        if (i == max_iter) break;
        seg_fit_mstep(row + 3, prior, start_mode, par, status);
        ++i;
    }
    // a generalised step (the stationary start) may have lowered the evidence: the iterate before it is the result
    if (i > 0 && trace[(uint64_t)i * PHK_SEG_TRACE_COLS + 9] < trace[(uint64_t)(i - 1) * PHK_SEG_TRACE_COLS + 9]) --i;
    *n_iter = i;
    for (int c = 0; c < 3; ++c) par[c] = trace[(uint64_t)i * PHK_SEG_TRACE_COLS + c];
    return PHK_OK;
}

extern "C" int phk_segment_fit(phk_ctx *ctx, const double *x, uint64_t n, const uint64_t *offsets, uint64_t R,
                               const double start[3], int start_mode, const double prior_counts[4], uint32_t max_iter, double tol,
                               double *trace, uint32_t *n_iter, uint32_t *status, double fitted[3]) {
    PHK_ENTER(ctx, "phk_segment_fit");
    PHK_REQUIRE(start && prior_counts && trace && n_iter && status && fitted, "phk_segment_fit: NULL pointer");
    PHK_REQUIRE(start_mode == PHK_SEG_START_FIXED || start_mode == PHK_SEG_START_FREE || start_mode == PHK_SEG_START_STATIONARY,
                "phk_segment_fit: start mode %d", start_mode);
    for (int c = 0; c < 4; ++c)
        PHK_REQUIRE(prior_counts[c] >= 0.0 && prior_counts[c] - prior_counts[c] == 0.0,
                    "phk_segment_fit: prior count %d = %g is not finite and >= 0", c, prior_counts[c]);
    PHK_REQUIRE(tol >= 0.0 && tol - tol == 0.0, "phk_segment_fit: tol = %g is not finite and >= 0", tol);
    PHK_REQUIRE(max_iter <= PHK_SEG_FIT_MAX_ITER, "phk_segment_fit: max_iter = %u exceeds %u", max_iter, PHK_SEG_FIT_MAX_ITER);
    double par[3] = {start[0], start[1], start[2]};
    if (start_mode == PHK_SEG_START_STATIONARY) par[2] = par[0] / (par[0] + par[1]);
    const double trans[4] = {1.0 - par[0], par[0], par[1], 1.0 - par[1]}, init[2] = {1.0 - par[2], par[2]};
    bool empty;
    PHK_TRY(seg_fit_check("phk_segment_fit", x, n, offsets, R, trans, init, &empty));
    *status = 0;
    const int rc = seg_fit_run(ctx, x, n, offsets, R, empty, start_mode, prior_counts, max_iter, tol, par, trace, n_iter, status);
    if (rc != PHK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    for (int c = 0; c < 3; ++c) fitted[c] = par[c];
    return PHK_OK;
}
