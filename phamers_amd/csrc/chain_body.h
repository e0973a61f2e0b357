// chain_body.h -- the per-record recurrences and the emission epilogue of the S-state chain, shared by the
// kernels of chain.hip that hold one set of parameters for every record and by its grouped kernels (4.28), which load a
// record's parameters from its group: one statement of the arithmetic, so that a group of a grouped call and a chain made
// from that group's records alone give the same bits.  A body is run by the SP lanes that carry one record (lane j = state
// j, `live` = j < S); the parameters come in registers: arow[i] = A[j][i], acol[i] = A[i][j], pj = pi[j] (zeros past S).
#pragma once
#include "mixture_body.h"

#define CH_CLAMP 32768.0
#define CH_LN2 0.693147180559945309417232121458

// the sum of v over the group's lanes in state order; every lane gets the same bits
template <int SP>
__device__ __forceinline__ double chain_sum(double v) {
    double s = __shfl(v, 0, SP);
#pragma unroll
    for (int i = 1; i < SP; ++i) s += __shfl(v, i, SP);
    return s;
}

// v / 2^e with e the exponent of the group's largest v: exact; returns e
template <int SP>
__device__ __forceinline__ int chain_scale2(double &v) {
    double m = v;
#pragma unroll
    for (int o = 1; o < SP; o <<= 1) m = fmax(m, __shfl_xor(m, o, SP));
    int e;
    (void)frexp(m, &e);
    v = ldexp(v, -e);
    return e;
}

__device__ __forceinline__ int64_t chain_quant(double d) { return (int64_t)rint(fmax(d, -CH_CLAMP) * 65536.0); }

// The wave's gram_tile accumulators of the queries q0 .. (rows 0 .. S - 1 of row tile 0 are the states): E = acc * temper
// and the row maximum M, for the queries below nq.
__device__ __forceinline__ void chain_emit_epilogue(const f64x4 acc[GT_QT][GT_RT], uint64_t q0, uint64_t nq, uint32_t S,
                                                    double temper, double *__restrict__ E, double *__restrict__ M) {
    const int li = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < GT_QT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double e = acc[a][0][r] * temper;
            double m = (uint32_t)li < S ? e : -__builtin_inf();
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) m = fmax(m, __shfl_xor(m, o));
            const uint64_t q = gram_query(q0, a, r);
            if (q < nq) {
                if ((uint32_t)li < S) E[q * S + li] = e;
                if (li == 0) M[q] = m;
            }
        }
}

// B[w][j] = beta_w(j) up to a power of two over the record's windows w0 .. w1 - 1 (w1 > w0): beta of the last step is 1,
// beta_{t-1}(i) = sum_j A_ij e_t(j) beta_t(j).
template <int SP>
__device__ __forceinline__ void chain_backward_record(const double *__restrict__ E, const double *__restrict__ M, uint64_t w0,
                                                      uint64_t w1, uint32_t S, uint32_t j, bool live, const double (&arow)[SP],
                                                      double *__restrict__ B) {
    double b = live ? 1.0 : 0.0;
    uint64_t w = w1 - 1;
    double x = live ? E[w * S + j] - M[w] : 0.0;
    for (;;) {
        if (live) B[w * S + j] = b;
        if (w == w0) break;
        const double e = live ? exp(x) : 0.0;
        --w;
        x = live ? E[w * S + j] - M[w] : 0.0;   // the next step's load, issued ahead of this step's chain
        const double u = e * b;
        double nb = 0.0;
#pragma unroll
        for (int i = 0; i < SP; ++i) nb += arow[i] * __shfl(u, i, SP);
        (void)chain_scale2<SP>(nb);
        b = nb;
    }
}

// G[w][j] = gamma_w(j) over the record's windows w0 .. w1 - 1; out = the record's vector xi[S][S], gamma_0[S], log evidence
// (zeros for a record without windows).
template <int SP>
__device__ __forceinline__ void chain_forward_record(const double *__restrict__ E, const double *__restrict__ M, uint64_t w0,
                                                     uint64_t w1, uint32_t S, uint32_t j, bool live, const double (&acol)[SP],
                                                     double pj, const double *__restrict__ B, double *__restrict__ G,
                                                     double *__restrict__ out) {
    double xi[SP];
#pragma unroll
    for (int i = 0; i < SP; ++i) xi[i] = 0.0;
    double g0 = 0.0, le = 0.0;
    if (w1 > w0) {
        double mw = M[w0];
        double x = live ? E[w0 * S + j] - mw : 0.0, bw = live ? B[w0 * S + j] : 0.0;
        double e = live ? exp(x) : 0.0;
        double sm = mw;
        int64_t ex = 0;
        {
            const double p = pj * (e * bw);
            g0 = p / chain_sum<SP>(p);
            if (live) G[w0 * S + j] = g0;
        }
        double a = pj * e;
        ex += chain_scale2<SP>(a);
        uint64_t w = w0 + 1;
        if (w < w1) {
            mw = M[w];
            x = live ? E[w * S + j] - mw : 0.0, bw = live ? B[w * S + j] : 0.0;
        }
        while (w < w1) {
            e = live ? exp(x) : 0.0;
            const double c = e * bw;
            sm += mw;
            const uint64_t wn = w + 1;
            if (wn < w1) {   // the next step's loads, issued ahead of this step's chain
                mw = M[wn];
                x = live ? E[wn * S + j] - mw : 0.0, bw = live ? B[wn * S + j] : 0.0;
            }
            double wv[SP], g = 0.0, col = 0.0;
#pragma unroll
            for (int i = 0; i < SP; ++i) {
                const double pr = __shfl(a, i, SP) * acol[i];
                g += pr;
                wv[i] = pr * c;
                col += wv[i];
            }
            const double inv = 1.0 / chain_sum<SP>(col);
#pragma unroll
            for (int i = 0; i < SP; ++i) xi[i] += wv[i] * inv;
            if (live) G[w * S + j] = col * inv;
            a = g * e;
            ex += chain_scale2<SP>(a);
            w = wn;
        }
        int e2;
        const double m = frexp(chain_sum<SP>(a), &e2);
        le = ((double)(ex + e2) * CH_LN2 + log(m)) + sm;
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < SP; ++i)
            if ((uint32_t)i < S) out[(uint32_t)i * S + j] = xi[i];
        out[S * S + j] = g0;
        if (j == 0) out[S * S + S] = le;
    }
}

// Max-plus on int64 over the record's windows w0 .. w1 - 1 (w1 > w0) with qcol[i] = qlog A[i][j], qp = qlog pi[j]:
// BP[8 w + j] = the predecessor of state j at step w (w > w0); score[r] and last[r] from lane 0.
template <int SP>
__device__ __forceinline__ void chain_viterbi_record(const double *__restrict__ E, const double *__restrict__ M, uint64_t w0,
                                                     uint64_t w1, uint32_t S, uint32_t j, bool live, const long long (&qcol)[SP],
                                                     long long qp, uint8_t *__restrict__ BP, int64_t *__restrict__ score,
                                                     uint8_t *__restrict__ last, uint64_t r) {
    long long d = qp + (live ? (long long)chain_quant(E[w0 * S + j] - M[w0]) : 0ll);
    uint64_t w = w0 + 1;
    double x = (live && w < w1) ? E[w * S + j] - M[w] : 0.0;
    while (w < w1) {
        const long long q = (long long)chain_quant(x);
        const uint64_t wn = w + 1;
        x = (live && wn < w1) ? E[wn * S + j] - M[wn] : 0.0;
        long long best = __shfl(d, 0, SP) + qcol[0];
        uint32_t k = 0;
#pragma unroll
        for (int i = 1; i < SP; ++i) {
            const long long c = __shfl(d, i, SP) + qcol[i];
            if ((uint32_t)i < S && c > best) best = c, k = (uint32_t)i;   // a tie stays with the smaller predecessor
        }
        d = best + q;
        BP[8 * w + j] = (uint8_t)k;
        w = wn;
    }
    long long best = __shfl(d, 0, SP);
    uint32_t k = 0;
#pragma unroll
    for (int i = 1; i < SP; ++i) {
        const long long c = __shfl(d, i, SP);
        if ((uint32_t)i < S && c > best) best = c, k = (uint32_t)i;
    }
    if (j == 0) score[r] = (int64_t)best, last[r] = (uint8_t)k;
}
