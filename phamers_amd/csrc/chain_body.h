// chain_body.h -- the recurrences and the emission epilogue of the S-state chain, each stated once for the
// three routes of chain.hip: the per-record kernels, which hold one set of parameters for every record; the walk kernels of
// the tile scan (4.27), which run a recurrence over a tile from the vector that enters it; the grouped kernels (4.28), which
// load a record's parameters from its group.  One statement of the arithmetic, so that a group of a grouped call and a
// chain made from that group's records alone give the same bits, and a tile's steps are the per-record route's steps.
//   chain_backward_span   beta = A (e o beta) with its rescale over windows [a, b) from beta of step b - 1
//   chain_forward_first   a record's first step from pi; chain_forward_span: the alpha / xi / gamma step over windows [w, b)
//   chain_maxplus_step    best predecessor and its index, a tie to the smaller; chain_maxplus_first, chain_maxplus_span
//   chain_*_record        a whole record: the span started from 1 (backward), from the first step (forward, Viterbi)
// A body is run by the SP lanes that carry one record or tile (lane j = state j, `live` = j < S); the parameters come in
// registers: arow[i] = A[j][i], acol[i] = A[i][j], pj = pi[j] (zeros past S).
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

// ---- backward: beta_{t-1}(i) = sum_j A_ij e_t(j) beta_t(j) ----------------------------------------------------------------
// Right to left over the windows [a, b) (b > a) from bv = beta of step b - 1: B[w][j] = beta_w(j) up to a power of two for
// every w of the span, rescaled step by step (exact); returns beta of step a.
template <int SP>
__device__ __forceinline__ double chain_backward_span(const double *__restrict__ E, const double *__restrict__ M, uint64_t a,
                                                      uint64_t b, uint32_t S, uint32_t j, bool live, const double (&arow)[SP],
                                                      double bv, double *__restrict__ B) {
    uint64_t w = b - 1;
    double x = live ? E[w * S + j] - M[w] : 0.0;
    for (;;) {
        if (live) B[w * S + j] = bv;
        if (w == a) break;
        const double e = live ? exp(x) : 0.0;
        --w;
        x = live ? E[w * S + j] - M[w] : 0.0;   // the next step's load, issued ahead of this step's chain
        const double u = e * bv;
        double nb = 0.0;
#pragma unroll
        for (int i = 0; i < SP; ++i) nb += arow[i] * __shfl(u, i, SP);
        (void)chain_scale2<SP>(nb);
        bv = nb;
    }
    return bv;
}

// B[w][j] over the record's windows w0 .. w1 - 1 (w1 > w0): beta of the last step is 1.
template <int SP>
__device__ __forceinline__ void chain_backward_record(const double *__restrict__ E, const double *__restrict__ M, uint64_t w0,
                                                      uint64_t w1, uint32_t S, uint32_t j, bool live, const double (&arow)[SP],
                                                      double *__restrict__ B) {
    (void)chain_backward_span<SP>(E, M, w0, w1, S, j, live, arow, live ? 1.0 : 0.0, B);
}

// ---- forward: alpha_t(j) = sum_i alpha_{t-1}(i) A_ij e_t(j), with xi and gamma of the step ----------------------------------
// what a step reads of window w: the row maximum, the relative emission of state j, beta_w(j)
__device__ __forceinline__ void chain_forward_load(const double *__restrict__ E, const double *__restrict__ M,
                                                   const double *__restrict__ B, uint64_t w, uint32_t S, uint32_t j, bool live,
                                                   double &mw, double &x, double &bw) {
    mw = M[w];
    x = live ? E[w * S + j] - mw : 0.0, bw = live ? B[w * S + j] : 0.0;
}

// A record's first step, from pi: g0 = gamma_0(j) = pi_j e_0(j) beta_0(j) normalised, a = alpha_0(j) = pi_j e_0(j), which the
// caller rescales (chain_scale2) once g0 is stored.
template <int SP>
__device__ __forceinline__ void chain_forward_first(double pj, double x, double bw, bool live, double &g0, double &a) {
    const double e = live ? exp(x) : 0.0;
    const double p = pj * (e * bw);
    g0 = p / chain_sum<SP>(p);
    a = pj * e;
}

// Left to right over the windows [w, b) from a = alpha entering w, with mw, x, bw loaded for w (chain_forward_load; unread
// if w == b): G[w][j] = gamma_w(j); the steps' normalised terms are added to xi[i] = xi(i, j), the exponents of the
// rescalings to ex, the row maxima to sm; returns alpha of step b - 1.
template <int SP>
__device__ __forceinline__ double chain_forward_span(const double *__restrict__ E, const double *__restrict__ M,
                                                     const double *__restrict__ B, uint64_t w, uint64_t b, uint32_t S, uint32_t j,
                                                     bool live, const double (&acol)[SP], double a, double mw, double x, double bw,
                                                     double *__restrict__ G, double (&xi)[SP], int64_t &ex, double &sm) {
    while (w < b) {
        const double e = live ? exp(x) : 0.0;
        const double c = e * bw;
        sm += mw;
        const uint64_t wn = w + 1;
        if (wn < b) chain_forward_load(E, M, B, wn, S, j, live, mw, x, bw);   // issued ahead of this step's chain
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
    return a;
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
        double mw, x, bw, a;
        chain_forward_load(E, M, B, w0, S, j, live, mw, x, bw);
        double sm = mw;
        chain_forward_first<SP>(pj, x, bw, live, g0, a);
        if (live) G[w0 * S + j] = g0;
        int64_t ex = chain_scale2<SP>(a);
        if (w0 + 1 < w1) chain_forward_load(E, M, B, w0 + 1, S, j, live, mw, x, bw);
        a = chain_forward_span<SP>(E, M, B, w0 + 1, w1, S, j, live, acol, a, mw, x, bw, G, xi, ex, sm);
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

// ---- max-plus on int64: delta_t(j) = max_i (delta_{t-1}(i) + qlog A_ij) + q_t(j) ------------------------------------------
// max_i (d of the group's lane i + qcol[i]) and k = the i that reaches it; a tie stays with the smaller i
template <int SP>
__device__ __forceinline__ long long chain_maxplus_step(long long d, const long long (&qcol)[SP], uint32_t S, uint32_t &k) {
    long long best = __shfl(d, 0, SP) + qcol[0];
    k = 0;
#pragma unroll
    for (int i = 1; i < SP; ++i) {
        const long long c = __shfl(d, i, SP) + qcol[i];
        if ((uint32_t)i < S && c > best) best = c, k = (uint32_t)i;
    }
    return best;
}

// delta of a record's first step w, from qp = qlog pi[j]
__device__ __forceinline__ long long chain_maxplus_first(const double *__restrict__ E, const double *__restrict__ M, uint64_t w,
                                                         uint32_t S, uint32_t j, bool live, long long qp) {
    return qp + (live ? (long long)chain_quant(E[w * S + j] - M[w]) : 0ll);
}

// Left to right over the windows [w, b) from d = delta entering w, with qcol[i] = qlog A[i][j]: BP[8 w + j] = the predecessor
// k of state j at step w, handed to each(k) as well; returns delta of step b - 1.
template <int SP, typename F>
__device__ __forceinline__ long long chain_maxplus_span(const double *__restrict__ E, const double *__restrict__ M, uint64_t w,
                                                        uint64_t b, uint32_t S, uint32_t j, bool live,
                                                        const long long (&qcol)[SP], long long d, uint8_t *__restrict__ BP,
                                                        F &&each) {
    double x = (live && w < b) ? E[w * S + j] - M[w] : 0.0;
    while (w < b) {
        const long long q = (long long)chain_quant(x);
        const uint64_t wn = w + 1;
        x = (live && wn < b) ? E[wn * S + j] - M[wn] : 0.0;   // the next step's load, issued ahead of this step's chain
        uint32_t k;
        d = chain_maxplus_step<SP>(d, qcol, S, k) + q;
        BP[8 * w + j] = (uint8_t)k;
        each(k);
        w = wn;
    }
    return d;
}

// Over the record's windows w0 .. w1 - 1 (w1 > w0) with qp = qlog pi[j]: BP for every step past the first; score[r] and
// last[r] (a tie to the smaller state) from lane 0.
template <int SP>
__device__ __forceinline__ void chain_viterbi_record(const double *__restrict__ E, const double *__restrict__ M, uint64_t w0,
                                                     uint64_t w1, uint32_t S, uint32_t j, bool live, const long long (&qcol)[SP],
                                                     long long qp, uint8_t *__restrict__ BP, int64_t *__restrict__ score,
                                                     uint8_t *__restrict__ last, uint64_t r) {
    const long long d = chain_maxplus_span<SP>(E, M, w0 + 1, w1, S, j, live, qcol, chain_maxplus_first(E, M, w0, S, j, live, qp),
                                               BP, [](uint32_t) {});
    const long long none[SP] = {};   // the step with no transition term: the best last state, a tie to the smaller
    uint32_t k;
    const long long best = chain_maxplus_step<SP>(d, none, S, k);
    if (j == 0) score[r] = (int64_t)best, last[r] = (uint8_t)k;
}
