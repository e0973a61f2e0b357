// chain.hip -- S-state hidden Markov chain over the count rows of windows (gfx950): this project's own, DESIGN.md 4.26.
//
// Records r have windows t = offsets[r] .. offsets[r + 1] - 1 with uint32 count rows c_t[D]; S states (2 .. PHK_CHAIN_MAX_STATES)
// with log profiles log theta_s[D] (host logarithms), transition A[S][S], start pi[S]:
//     E[t][s] = temper * sum_j c_t[j] log theta_s[j]        (gram_tile on the fp64 matrix pipe, one multiply afterwards)
//     d[t][s] = E[t][s] - max_s' E[t][s']  <= 0             (the relative emission; a window without k-mers has d = 0)
// Every result of a record is a function of its own rows and the parameters: not of the call's other records, its place
// among them, batch_rows, the entry point, the launch or the run.
//
// A record is carried by a GROUP of SP lanes (SP = S padded to 2, 4 or 8; 64 / SP records per wave), lane j = state j; a padded
// state has A = 0, pi = 0 and emission 0, which adds exact zeros.  Cross-lane traffic is __shfl within the group; sums over
// the states run in state order 0 .. SP - 1 in every lane alike.  No LDS, no barrier.
//   phk_chain_emit_kernel      E and the row maximum M from the count rows (the shape of phk_mix_resp_kernel's first half)
//   phk_chain_rowmax_kernel    M of emissions that came from the host (phk_chain_create_from_emissions)
//   phk_chain_backward_kernel  beta_t of every step, right to left, rescaled by powers of two (exact), into B[n][S]
//   phk_chain_forward_kernel   alpha left to right (rescaled likewise, the exponent kept as an integer); in step order: the
//                              step's S^2 terms w_ij = alpha_{t-1}(i) A_ij e_t(j) beta_t(j) normalised by their own sum, added
//                              to xi; gamma_t(j) = the column sum over that sum (step 0: pi_j e_0(j) beta_0(j) normalised);
//                              the record's vector (xi, gamma_0, log evidence) into V[R][S^2 + S + 1]
//   phk_chain_viterbi_kernel   max-plus on int64 over q[t][s] = rint(max(d, -2^15) 2^16), ties to the smallest predecessor; the
//                              backpointers of a step as the bytes of one 64-bit word; path_score and the last state (a tie to
//                              the smallest state)
//   phk_chain_trace_kernel     lane per record: the path, right to left through the words
//   phk_chain_spread_kernel    gamma [rows][S] -> [rows][64] (zeros past S): the R operand of mix_expect_body
//   phk_chain_expect_kernel    T = gamma^T C and N_s: mix_expect_body (mixture_body.h), blocks of MIX_RB rows anchored at the
//                              global row index
//   phk_chain_fold_kernel      mix_fold_body: the fixed 256-row tree, over the row blocks' partial vectors and over the records'
//                              vectors alike
// The records of at least scan_from windows (phk_chain_set_scan; 0: none) are passed over by the four per-record kernels and
// take the tile scan, the phk_chain_scan_* kernels further down.
// The recurrences and the emission epilogue are the bodies of chain_body.h, each stated once: the per-record kernels run a
// span body over a whole record, the walk kernels of the tile scan run the same bodies over a tile from the vector that
// enters it, and the phk_chain_group_* kernels further down run them with the parameters of the record's group
// (phk_chain_set_groups).
// The integer sums: |q| <= 2^31 and |qlog| <= 2^31 (checked), so a path over n <= 2^30 windows stays inside 2^62.
// The float sums stay away from 0 / 0 as long as the ratio of two entries of a row or column of A stays inside the format
// (entries of 1e-12 are tested): the largest entry of a rescaled vector is in [1/2, 1) and the state of the largest emission
// has e = 1, so every normalising sum is at least min(A) / 2 times a positive normal number.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

#include "chain_body.h"

#define CH_BLOCKS_MAX 1024      // 64-lane workgroups per launch of the per-record kernels
#define CH_KP MIX_CT            // row stride of the spread gamma
#define CH_QMAX (1ll << 31)
#define CH_NMAX (1ull << 30)

static_assert(PHK_CHAIN_MAX_STATES == 8, "a step's backpointers are the bytes of one 64-bit word");

template <bool FULL>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_chain_emit_kernel(const uint32_t *__restrict__ C, uint64_t nq,
                                                                        const double *__restrict__ L, uint32_t S, uint64_t D,
                                                                        double temper, double *__restrict__ E,
                                                                        double *__restrict__ M) {
    const int wave = threadIdx.x >> 6;
    const uint64_t q0 = (uint64_t)blockIdx.x * GT_QB + (uint64_t)wave * (GT_QT * 16);
    f64x4 acc[GT_QT][GT_RT];
    gram_tile<FULL, GT_QT, uint32_t>(C, nq, q0, L, S, 0, D, acc);   // S <= 8: the states are rows 0 .. S - 1 of row tile 0
    chain_emit_epilogue(acc, q0, nq, S, temper, E, M);
}

__global__ __launch_bounds__(256) void phk_chain_rowmax_kernel(const double *__restrict__ E, uint64_t n, uint32_t S,
                                                               double *__restrict__ M) {
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (uint64_t)gridDim.x * 256) {
        double m = E[t * S];
        for (uint32_t s = 1; s < S; ++s) m = fmax(m, E[t * S + s]);
        M[t] = m;
    }
}

// a record of `len` windows takes the tile scan (the per-record kernels pass over it); scan_from == 0: no record does
__device__ __forceinline__ bool chain_scanned(uint64_t len, uint64_t scan_from) { return scan_from != 0 && len >= scan_from; }

// par = A[S][S] then pi[S].  B[w][j] = beta_w(j) up to a power of two: beta of the record's last step is 1,
// beta_{t-1}(i) = sum_j A_ij e_t(j) beta_t(j).
template <int SP>
__global__ __launch_bounds__(64) void phk_chain_backward_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                                const uint64_t *__restrict__ off, uint64_t R, uint32_t S,
                                                                const double *__restrict__ par, double *__restrict__ B,
                                                                uint64_t scan_from) {
    const uint32_t j = threadIdx.x % SP;
    const bool live = j < S;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / SP);
    double arow[SP];
#pragma unroll
    for (int i = 0; i < SP; ++i) arow[i] = (live && (uint32_t)i < S) ? par[j * S + i] : 0.0;
    for (uint64_t r = (uint64_t)blockIdx.x * (64 / SP) + threadIdx.x / SP; r < R; r += groups) {
        const uint64_t w0 = off[r], w1 = off[r + 1];
        if (w1 == w0 || chain_scanned(w1 - w0, scan_from)) continue;
        chain_backward_record<SP>(E, M, w0, w1, S, j, live, arow, B);
    }
}

// G[w][j] = gamma_w(j); V[r] = xi[S][S], gamma_0[S], log evidence.
template <int SP>
__global__ __launch_bounds__(64) void phk_chain_forward_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                               const uint64_t *__restrict__ off, uint64_t R, uint32_t S,
                                                               const double *__restrict__ par, const double *__restrict__ B,
                                                               double *__restrict__ G, double *__restrict__ V,
                                                               uint64_t scan_from) {
    const uint32_t j = threadIdx.x % SP;
    const bool live = j < S;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / SP);
    const uint64_t Ev = (uint64_t)S * S + S + 1;
    double acol[SP];
#pragma unroll
    for (int i = 0; i < SP; ++i) acol[i] = (live && (uint32_t)i < S) ? par[(uint32_t)i * S + j] : 0.0;
    const double pj = live ? par[S * S + j] : 0.0;
    for (uint64_t r = (uint64_t)blockIdx.x * (64 / SP) + threadIdx.x / SP; r < R; r += groups) {
        const uint64_t w0 = off[r], w1 = off[r + 1];
        if (chain_scanned(w1 - w0, scan_from)) continue;
        chain_forward_record<SP>(E, M, w0, w1, S, j, live, acol, pj, B, G, V + r * Ev);
    }
}

// qpar = qlog A[S][S] then qlog pi[S].  BP[8 w + j] = the predecessor of state j at step w (w > the record's first).
template <int SP>
__global__ __launch_bounds__(64) void phk_chain_viterbi_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                               const uint64_t *__restrict__ off, uint64_t R, uint32_t S,
                                                               const int64_t *__restrict__ qpar, uint8_t *__restrict__ BP,
                                                               int64_t *__restrict__ score, uint8_t *__restrict__ last,
                                                               uint64_t scan_from) {
    const uint32_t j = threadIdx.x % SP;
    const bool live = j < S;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / SP);
    long long qcol[SP];
#pragma unroll
    for (int i = 0; i < SP; ++i) qcol[i] = (live && (uint32_t)i < S) ? (long long)qpar[(uint32_t)i * S + j] : 0ll;
    const long long qp = live ? (long long)qpar[S * S + j] : 0ll;
    for (uint64_t r = (uint64_t)blockIdx.x * (64 / SP) + threadIdx.x / SP; r < R; r += groups) {
        const uint64_t w0 = off[r], w1 = off[r + 1];
        if (chain_scanned(w1 - w0, scan_from)) continue;
        if (w1 == w0) {
            if (j == 0) score[r] = 0, last[r] = 0;
            continue;
        }
        chain_viterbi_record<SP>(E, M, w0, w1, S, j, live, qcol, qp, BP, score, last, r);
    }
}

__global__ __launch_bounds__(64) void phk_chain_trace_kernel(const uint64_t *__restrict__ off, uint64_t R,
                                                             const uint8_t *__restrict__ last, const uint64_t *__restrict__ BP,
                                                             uint8_t *__restrict__ state, uint64_t scan_from) {
    for (uint64_t r = (uint64_t)blockIdx.x * 64 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 64) {
        const uint64_t w0 = off[r];
        if (chain_scanned(off[r + 1] - w0, scan_from)) continue;
        uint32_t s = last[r];
#pragma unroll 8
        for (uint64_t w = off[r + 1]; w > w0; --w) {
            state[w - 1] = (uint8_t)s;
            s = (uint32_t)(BP[w - 1] >> (8 * s)) & 0xffu;   // (the word of the record's first step is not followed)
        }
    }
}

__global__ __launch_bounds__(256) void phk_chain_spread_kernel(const double *__restrict__ G, uint64_t nb, uint32_t S,
                                                               double *__restrict__ Rx) {
    const uint64_t total = nb * CH_KP;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t c = (uint32_t)(i % CH_KP);
        Rx[i] = c < S ? G[(i / CH_KP) * S + c] : 0.0;
    }
}

// grid: x = row block of the batch, y = group of four column tiles; see phk_mix_expect_kernel
template <bool VEC>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_chain_expect_kernel(const double *__restrict__ Rx,
                                                                          const uint32_t *__restrict__ C, uint64_t D, uint64_t nb,
                                                                          const double *__restrict__ M, uint32_t S, uint64_t Em,
                                                                          double *__restrict__ part) {
    mix_expect_body<VEC>(Rx, CH_KP, C, D, nb, M, S, blockIdx.x, blockIdx.y, 0, part + (uint64_t)blockIdx.x * Em);
}

__global__ __launch_bounds__(256) void phk_chain_fold_kernel(const double *__restrict__ in, uint64_t m, uint64_t Ev,
                                                             double *__restrict__ out) {
    mix_fold_body(in, m, Ev, blockIdx.x, blockIdx.y, out + (uint64_t)blockIdx.y * Ev);
}

// ---- grouped chains -------------------------------------------------------------------------------------
// The records are cut into groups g = 0 .. G - 1 of consecutive records, each with its own log profiles, A, pi: gpar =
// [G][S^2 + S] (A then pi), gqpar likewise, glogp = [G][S][D].  rg[r] = the group of record r, or CH_NO_GROUP for a record
// the kernels pass over (its group is inactive or holds no window).  The matrix-pipe kernels and the fold find their work
// in descriptor tables built per phk_chain_set_grouped for the groups at work and read at blockIdx.x (uniform addresses);
// the per-record kernels load a record's parameters from its group one record ahead of the record they work on
// (chain_group_walk: the one loop of the three).
//   phk_chain_group_emit_kernel      gram_tile + chain_emit_epilogue for the workgroup's (group, row tile of that group)
//   phk_chain_group_backward_kernel  chain_backward_record with the record's group's A
//   phk_chain_group_forward_kernel   chain_forward_record
//   phk_chain_group_viterbi_kernel   chain_viterbi_record
//   phk_chain_group_expect_kernel    mix_expect_body for the workgroup's (group, block of MIX_RB rows from the group's first
//                                    window, column group)
//   phk_chain_group_fold_kernel      mix_fold_body for the workgroup's (vectors of one group, 256 elements), a launch per level
#define CH_NO_GROUP 0xffffffffu

struct ChainGroup {        // one per group
    uint64_t w0, n;        // its first window and its windows
};
struct ChainGroupTile {    // emit: tile = row tile of the group; expect: tile = row block of the group, y = column group
    uint32_t group, tile, y, pad;
    uint64_t part;         // expect: the block's partial vector among all the call's
};
struct ChainGroupFold {    // one workgroup of a fold level: elements 256 ex .. of the tree over vectors 256 vb .. of in
    const double *in;
    double *out;           // the output vector of vb
    uint64_t m, E;
    uint32_t ex, vb;
};

template <bool FULL>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_chain_group_emit_kernel(const uint32_t *__restrict__ C,
                                                                              const ChainGroup *__restrict__ grp,
                                                                              const ChainGroupTile *__restrict__ tiles,
                                                                              const double *__restrict__ L, uint32_t S, uint64_t D,
                                                                              double temper, double *__restrict__ E,
                                                                              double *__restrict__ M) {
    const ChainGroupTile t = tiles[blockIdx.x];
    const ChainGroup g = grp[t.group];
    const int wave = threadIdx.x >> 6;
    const uint64_t q0 = (uint64_t)t.tile * GT_QB + (uint64_t)wave * (GT_QT * 16);
    f64x4 acc[GT_QT][GT_RT];
    gram_tile<FULL, GT_QT, uint32_t>(C + g.w0 * D, g.n, q0, L + (uint64_t)t.group * S * D, S, 0, D, acc);
    chain_emit_epilogue(acc, q0, g.n, S, temper, E + g.w0 * S, M + g.w0);
}

// What a record body takes of its group's parameters in lane j: a[i] = A[j][i] (COL false: backward), or a[i] = A[i][j] and
// p = pi[j] (COL true: forward on doubles, Viterbi on the quantised logarithms); zeros past S and for CH_NO_GROUP.
template <int SP, typename T, bool COL>
struct ChainGroupPar {
    T a[SP], p;
    __device__ __forceinline__ void load(const T *__restrict__ par, uint32_t g, uint32_t S, uint32_t j, bool live) {
        const T *q = par + (uint64_t)(g == CH_NO_GROUP ? 0 : g) * (S * S + S);
        const bool ok = live && g != CH_NO_GROUP;
#pragma unroll
        for (int i = 0; i < SP; ++i) a[i] = (ok && (uint32_t)i < S) ? q[COL ? (uint32_t)i * S + j : j * S + (uint32_t)i] : (T)0;
        if constexpr (COL) p = ok ? q[S * S + j] : (T)0;   // (a row goes without the pi entry)
    }
};

// The records of the lane group in turn: record(r, j, live, par) for every record r of a group at work, par = its group's
// parameters, loaded one record ahead of the record at work.
template <int SP, typename T, bool COL, typename F>
__device__ __forceinline__ void chain_group_walk(const uint32_t *__restrict__ rg, uint64_t R, const T *__restrict__ gpar,
                                                 uint32_t S, F &&record) {
    const uint32_t j = threadIdx.x % SP;
    const bool live = j < S;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / SP);
    uint64_t r = (uint64_t)blockIdx.x * (64 / SP) + threadIdx.x / SP;
    uint32_t g = r < R ? rg[r] : CH_NO_GROUP;
    ChainGroupPar<SP, T, COL> par, next;
    par.load(gpar, g, S, j, live);
    for (; r < R; r += groups) {
        const uint64_t rn = r + groups;
        const uint32_t gn = rn < R ? rg[rn] : CH_NO_GROUP;   // the next record's parameters, issued ahead of this record's chain
        next.load(gpar, gn, S, j, live);
        if (g != CH_NO_GROUP) record(r, j, live, par);
        g = gn, par = next;
    }
}

template <int SP>
__global__ __launch_bounds__(64) void phk_chain_group_backward_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                                      const uint64_t *__restrict__ off, uint64_t R, uint32_t S,
                                                                      const uint32_t *__restrict__ rg,
                                                                      const double *__restrict__ gpar, double *__restrict__ B) {
    chain_group_walk<SP, double, false>(rg, R, gpar, S, [&](uint64_t r, uint32_t j, bool live, const auto &par) {
        const uint64_t w0 = off[r], w1 = off[r + 1];
        if (w1 != w0) chain_backward_record<SP>(E, M, w0, w1, S, j, live, par.a, B);
    });
}

template <int SP>
__global__ __launch_bounds__(64) void phk_chain_group_forward_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                                     const uint64_t *__restrict__ off, uint64_t R, uint32_t S,
                                                                     const uint32_t *__restrict__ rg,
                                                                     const double *__restrict__ gpar,
                                                                     const double *__restrict__ B, double *__restrict__ G,
                                                                     double *__restrict__ V) {
    const uint64_t Ev = (uint64_t)S * S + S + 1;
    chain_group_walk<SP, double, true>(rg, R, gpar, S, [&](uint64_t r, uint32_t j, bool live, const auto &par) {
        chain_forward_record<SP>(E, M, off[r], off[r + 1], S, j, live, par.a, par.p, B, G, V + r * Ev);
    });
}

template <int SP>
__global__ __launch_bounds__(64) void phk_chain_group_viterbi_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                                     const uint64_t *__restrict__ off, uint64_t R, uint32_t S,
                                                                     const uint32_t *__restrict__ rg,
                                                                     const int64_t *__restrict__ gqpar, uint8_t *__restrict__ BP,
                                                                     int64_t *__restrict__ score, uint8_t *__restrict__ last) {
    chain_group_walk<SP, long long, true>(rg, R, (const long long *)gqpar, S,
                                          [&](uint64_t r, uint32_t j, bool live, const auto &par) {
        const uint64_t w0 = off[r], w1 = off[r + 1];
        if (w1 == w0) {
            if (j == 0) score[r] = 0, last[r] = 0;
        } else {
            chain_viterbi_record<SP>(E, M, w0, w1, S, j, live, par.a, par.p, BP, score, last, r);
        }
    });
}

// Rx holds the spread gamma of the windows wa .. of the batch; a group's rows start at window w0 (before wa for a group cut
// over several batches: the body reads the block's rows only, which the batch holds)
template <bool VEC>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_chain_group_expect_kernel(const double *__restrict__ Rx, uint64_t wa,
                                                                                const uint32_t *__restrict__ C, uint64_t D,
                                                                                const ChainGroup *__restrict__ grp,
                                                                                const ChainGroupTile *__restrict__ tiles,
                                                                                const double *__restrict__ M, uint32_t S,
                                                                                uint64_t Em, double *__restrict__ part) {
    const ChainGroupTile t = tiles[blockIdx.x];
    const ChainGroup g = grp[t.group];
    const double *R0 = Rx + ((int64_t)g.w0 - (int64_t)wa) * (int64_t)CH_KP;
    mix_expect_body<VEC>(R0, CH_KP, C + g.w0 * D, D, g.n, M + g.w0, S, t.tile, t.y, 0, part + t.part * Em);
}

__global__ __launch_bounds__(256) void phk_chain_group_fold_kernel(const ChainGroupFold *__restrict__ folds) {
    const ChainGroupFold f = folds[blockIdx.x];
    mix_fold_body(f.in, f.m, f.E, f.ex, f.vb, f.out);
}

extern "C" uint64_t phk_chain_grid_pass(void) { return (uint64_t)CH_BLOCKS_MAX * 32; }

// ---- the tile scan ----------------------------------------------------------------------------------------
// A record of at least scan_from windows is cut into tiles of PHK_CHAIN_TILE windows from its own start.  The scanned records
// are s = 0 .. ns - 1 (record sr[s], tiles st[s] .. st[s + 1] - 1); tile t belongs to scanned record ti[t].
//   phk_chain_scan_tile_kernel   a group of SP x SP lanes per tile, lane (i, j) = entry [i][j]: F = the ordered product of the
//                                tile's A diag(e_t) with the exponent of its power-of-two rescaling, the max-plus product Vq on
//                                int64, the tile's sum of M.  A record's first tile starts from
//                                pi: every row is that vector.
//   phk_chain_scan_carry_kernel  a group of SP x SP lanes per scanned record, over its tiles in tile order; blockIdx.y is the
//                                role: alpha entering every tile and the log evidence (left to right), beta leaving every tile
//                                (right to left), delta entering every tile, path_score and the last state (left to right).
//                                The tiles' matrices are loaded CH_PF tiles ahead of the chain.
//   phk_chain_scan_walk_kernel   a group of SP lanes per tile: chain_backward_span and chain_forward_span, the bodies of the
//                                per-record kernels, inside the tile from the vectors that enter it; gamma, the tile's xi,
//                                gamma_0 from the first
//   phk_chain_scan_path_kernel   likewise chain_maxplus_span: the backpointer words (the tile's first step too) and the
//                                tile's map from end state to the state before the tile
//   phk_chain_scan_fold_kernel   xi of a record = its tiles' xi added in tile order, into V[r]
//   phk_chain_scan_ends_kernel   lane per scanned record: the state at every tile's end, right to left through the maps
//   phk_chain_scan_fill_kernel   lane per tile: the tile's states from its end state and its words
#define CH_SCAN_PASS 4096ull    // tiles per launch of the per-tile kernels
#define CH_PF 8                 // tiles the carry loads ahead

static_assert(PHK_CHAIN_TILE == 64, "DESIGN.md 4.27 states the step count for 64");

// tile t: its record, whether it is the record's first, its windows [a, b)
__device__ __forceinline__ void chain_scan_tile(const uint32_t *__restrict__ ti, const uint64_t *__restrict__ sr,
                                                const uint64_t *__restrict__ st, const uint64_t *__restrict__ off, uint64_t t,
                                                uint64_t &r, bool &first, uint64_t &a, uint64_t &b) {
    const uint32_t s = ti[t];
    r = sr[s];
    const uint64_t t0 = st[s], w1 = off[r + 1];
    first = t == t0;
    a = off[r] + (t - t0) * PHK_CHAIN_TILE;
    b = a + PHK_CHAIN_TILE < w1 ? a + PHK_CHAIN_TILE : w1;
}

// v / 2^e with e the exponent of the largest v over the lanes l ^ o, o = LO, 2 LO, .. < HI: exact; returns e
template <int LO, int HI>
__device__ __forceinline__ int chain_scale2x(double &v) {
    double m = v;
#pragma unroll
    for (int o = LO; o < HI; o <<= 1) m = fmax(m, __shfl_xor(m, o, HI));
    int e;
    (void)frexp(m, &e);
    v = ldexp(v, -e);
    return e;
}

template <int SP>
__global__ __launch_bounds__(64) void phk_chain_scan_tile_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                                 const uint64_t *__restrict__ off, const uint32_t *__restrict__ ti,
                                                                 const uint64_t *__restrict__ sr, const uint64_t *__restrict__ st,
                                                                 uint64_t nt, uint32_t S, const double *__restrict__ par,
                                                                 const int64_t *__restrict__ qpar, double *__restrict__ F,
                                                                 int32_t *__restrict__ FE, int64_t *__restrict__ Vq,
                                                                 double *__restrict__ SM) {
    constexpr int G = SP * SP;
    const uint32_t g = threadIdx.x % G, i = g / SP, j = g % SP;
    const bool lj = j < S, live = lj && i < S;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / G);
    double acol[SP];
    long long qcol[SP];
#pragma unroll
    for (int k = 0; k < SP; ++k) {
        acol[k] = (lj && (uint32_t)k < S) ? par[(uint32_t)k * S + j] : 0.0;
        qcol[k] = (lj && (uint32_t)k < S) ? (long long)qpar[(uint32_t)k * S + j] : 0ll;
    }
    const double aij = live ? par[i * S + j] : 0.0, pj = live ? par[S * S + j] : 0.0;
    const long long qij = live ? (long long)qpar[i * S + j] : 0ll, qpj = live ? (long long)qpar[S * S + j] : 0ll;
    for (uint64_t t = (uint64_t)blockIdx.x * (64 / G) + threadIdx.x / G; t < nt; t += groups) {
        uint64_t r, a, b;
        bool first;
        chain_scan_tile(ti, sr, st, off, t, r, first, a, b);
        double mw = M[a];
        double x = lj ? E[a * S + j] - mw : 0.0;
        double f = (first ? pj : aij) * (lj ? exp(x) : 0.0);
        long long v = (first ? qpj : qij) + (lj ? (long long)chain_quant(x) : 0ll);
        int fe = chain_scale2x<1, G>(f);
        double sm = mw;
        uint64_t w = a + 1;
        if (w < b) {
            mw = M[w];
            x = lj ? E[w * S + j] - mw : 0.0;
        }
        while (w < b) {
            const double e = lj ? exp(x) : 0.0;
            const long long q = lj ? (long long)chain_quant(x) : 0ll;
            sm += mw;
            const uint64_t wn = w + 1;
            if (wn < b) {   // the next step's loads, issued ahead of this step's chain
                mw = M[wn];
                x = lj ? E[wn * S + j] - mw : 0.0;
            }
            double gs = 0.0;
#pragma unroll
            for (int k = 0; k < SP; ++k) gs += __shfl(f, k, SP) * acol[k];
            f = gs * e;
            fe += chain_scale2x<1, G>(f);
            // row i of the max-plus product: chain_maxplus_step without the predecessor's index, kept here in its own words
            // because the call costs this kernel registers (96 -> 100 VGPRs at SP = 4)
            long long best = __shfl(v, 0, SP) + qcol[0];
#pragma unroll
            for (int k = 1; k < SP; ++k) {
                const long long c = __shfl(v, k, SP) + qcol[k];
                if ((uint32_t)k < S && c > best) best = c;
            }
            v = best + q;
            w = wn;
        }
        F[t * G + g] = f;
        Vq[t * G + g] = live ? (int64_t)v : 0;
        if (g == 0) FE[t] = fe, SM[t] = sm;
    }
}

// roles: 0 alpha and the evidence, 1 beta, 2 delta, path_score and the last state.  AI[t][i] = alpha entering tile t (t not the
// record's first), BO[t][j] = beta of tile t's last step, DI[t][i] = delta entering tile t; V[r]'s last entry = log evidence.
template <int SP>
__global__ __launch_bounds__(64) void phk_chain_scan_carry_kernel(const double *__restrict__ F, const int32_t *__restrict__ FE,
                                                                  const int64_t *__restrict__ Vq, const double *__restrict__ SM,
                                                                  const uint64_t *__restrict__ sr, const uint64_t *__restrict__ st,
                                                                  uint64_t ns, uint32_t S, uint32_t role0, double *__restrict__ AI,
                                                                  double *__restrict__ BO, int64_t *__restrict__ DI,
                                                                  double *__restrict__ V, int64_t *__restrict__ score,
                                                                  uint8_t *__restrict__ last) {
    constexpr int G = SP * SP;
    const uint32_t g = threadIdx.x % G, i = g / SP, j = g % SP;
    const uint32_t role = role0 + blockIdx.y;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / G), Ev = (uint64_t)S * S + S + 1;
    for (uint64_t s = (uint64_t)blockIdx.x * (64 / G) + threadIdx.x / G; s < ns; s += groups) {
        const uint64_t t0 = st[s], t1 = st[s + 1], r = sr[s];
        if (role == 0) {
            // lane (i, j) holds alpha(i) in ai and alpha(j) in ar; the first tile's row 0 is the vector from pi
            double ai = F[t0 * G + i], ar = F[t0 * G + j], sm = SM[t0];
            int64_t ex = FE[t0];
            double fb[CH_PF], sb[CH_PF];
            int eb[CH_PF];
#pragma unroll
            for (int p = 0; p < CH_PF; ++p) {
                const uint64_t t = t0 + 1 + p;
                const bool ok = t < t1;
                fb[p] = ok ? F[t * G + g] : 0.0, eb[p] = ok ? FE[t] : 0, sb[p] = ok ? SM[t] : 0.0;
            }
            for (uint64_t base = t0 + 1; base < t1; base += CH_PF) {
#pragma unroll
                for (int p = 0; p < CH_PF; ++p) {
                    const uint64_t t = base + p, tn = t + CH_PF;
                    if (t >= t1) break;
                    const double f = fb[p], smt = sb[p];
                    const int fe = eb[p];
                    if (tn < t1) fb[p] = F[tn * G + g], eb[p] = FE[tn], sb[p] = SM[tn];
                    if (j == 0) AI[t * SP + i] = ai;
                    const double pr = ai * f;
                    double sum = __shfl(pr, j, G);
#pragma unroll
                    for (int k = 1; k < SP; ++k) sum += __shfl(pr, k * SP + j, G);   // over the start states in state order
                    ex += fe + chain_scale2x<1, SP>(sum);
                    ar = sum;
                    ai = __shfl(sum, i, G);
                    sm += smt;
                }
            }
            int e2;
            const double m = frexp(chain_sum<SP>(ar), &e2);
            if (g == 0) V[r * Ev + S * S + S] = ((double)(ex + e2) * CH_LN2 + log(m)) + sm;
        } else if (role == 1) {
            // lane (i, j) holds beta(j); tiles t1 - 1 down to t0, c counts them
            const uint64_t K = t1 - t0;
            double bj = j < S ? 1.0 : 0.0;
            double fb[CH_PF];
#pragma unroll
            for (int p = 0; p < CH_PF; ++p) fb[p] = (uint64_t)p + 1 < K ? F[(t1 - 1 - p) * G + g] : 0.0;
            for (uint64_t base = 0; base < K; base += CH_PF) {
#pragma unroll
                for (int p = 0; p < CH_PF; ++p) {
                    const uint64_t c = base + p, cn = c + CH_PF;
                    if (c >= K) break;
                    const uint64_t t = t1 - 1 - c;
                    const double f = fb[p];
                    if (cn + 1 < K) fb[p] = F[(t1 - 1 - cn) * G + g];
                    if (i == 0) BO[t * SP + j] = bj;
                    if (c + 1 == K) break;
                    double sum = chain_sum<SP>(f * bj);   // beta'(i), over the end states in state order
                    (void)chain_scale2x<SP, G>(sum);
                    bj = __shfl(sum, j * SP, G);
                }
            }
        } else {
            long long di = Vq[t0 * G + i], dr = Vq[t0 * G + j];
            long long vb[CH_PF];
#pragma unroll
            for (int p = 0; p < CH_PF; ++p) vb[p] = t0 + 1 + p < t1 ? (long long)Vq[(t0 + 1 + p) * G + g] : 0ll;
            for (uint64_t base = t0 + 1; base < t1; base += CH_PF) {
#pragma unroll
                for (int p = 0; p < CH_PF; ++p) {
                    const uint64_t t = base + p, tn = t + CH_PF;
                    if (t >= t1) break;
                    const long long v = vb[p];
                    if (tn < t1) vb[p] = (long long)Vq[tn * G + g];
                    if (j == 0) DI[t * SP + i] = (int64_t)di;
                    const long long c = di + v;
                    long long best = __shfl(c, j, G);
#pragma unroll
                    for (int k = 1; k < SP; ++k) {
                        const long long o = __shfl(c, k * SP + j, G);
                        if ((uint32_t)k < S && o > best) best = o;
                    }
                    dr = best;
                    di = __shfl(best, i, G);
                }
            }
            long long best = __shfl(dr, 0, SP);
            uint32_t k = 0;
#pragma unroll
            for (int q = 1; q < SP; ++q) {
                const long long c = __shfl(dr, q, SP);
                if ((uint32_t)q < S && c > best) best = c, k = (uint32_t)q;   // a tie stays with the smaller state
            }
            if (g == 0) score[r] = (int64_t)best, last[r] = (uint8_t)k;
        }
    }
}

// XI[t][i][j] = the tile's xi (SP x SP, zeros past S); gamma_0 goes into V[r] from the record's first tile.
template <int SP>
__global__ __launch_bounds__(64) void phk_chain_scan_walk_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                                 const uint64_t *__restrict__ off, const uint32_t *__restrict__ ti,
                                                                 const uint64_t *__restrict__ sr, const uint64_t *__restrict__ st,
                                                                 uint64_t nt, uint32_t S, const double *__restrict__ par,
                                                                 const double *__restrict__ AI, const double *__restrict__ BO,
                                                                 double *B, double *__restrict__ Gm, double *__restrict__ XI,
                                                                 double *__restrict__ V) {
    const uint32_t j = threadIdx.x % SP;
    const bool live = j < S;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / SP), Ev = (uint64_t)S * S + S + 1;
    double arow[SP], acol[SP];
#pragma unroll
    for (int i = 0; i < SP; ++i) {
        arow[i] = (live && (uint32_t)i < S) ? par[j * S + i] : 0.0;
        acol[i] = (live && (uint32_t)i < S) ? par[(uint32_t)i * S + j] : 0.0;
    }
    const double pj = live ? par[S * S + j] : 0.0;
    for (uint64_t t = (uint64_t)blockIdx.x * (64 / SP) + threadIdx.x / SP; t < nt; t += groups) {
        uint64_t r, a, b;
        bool first;
        chain_scan_tile(ti, sr, st, off, t, r, first, a, b);
        // beta of the tile's steps, right to left from the vector of its last step; bw = beta of its first step
        double bw = chain_backward_span<SP>(E, M, a, b, S, j, live, arow, live ? BO[t * SP + j] : 0.0, B);
        // alpha, gamma and xi left to right from the vector that enters the tile (the exponents and the sum of M are the
        // carry's: what the span adds up here goes unused)
        double xi[SP];
#pragma unroll
        for (int i = 0; i < SP; ++i) xi[i] = 0.0;
        double mw = M[a], x = live ? E[a * S + j] - mw : 0.0, al, sm = 0.0;
        int64_t ex = 0;
        uint64_t w = a;
        if (first) {
            double g0;
            chain_forward_first<SP>(pj, x, bw, live, g0, al);
            if (live) Gm[a * S + j] = g0, V[r * Ev + S * S + j] = g0;
            (void)chain_scale2<SP>(al);
            w = a + 1;
            if (w < b) chain_forward_load(E, M, B, w, S, j, live, mw, x, bw);
        } else {
            al = live ? AI[t * SP + j] : 0.0;
        }
        (void)chain_forward_span<SP>(E, M, B, w, b, S, j, live, acol, al, mw, x, bw, Gm, xi, ex, sm);
#pragma unroll
        for (int i = 0; i < SP; ++i) XI[t * (SP * SP) + (uint32_t)i * SP + j] = xi[i];
    }
}

// MP[8 t + j] = the state before tile t on the best path that ends the tile in state j.
template <int SP>
__global__ __launch_bounds__(64) void phk_chain_scan_path_kernel(const double *__restrict__ E, const double *__restrict__ M,
                                                                 const uint64_t *__restrict__ off, const uint32_t *__restrict__ ti,
                                                                 const uint64_t *__restrict__ sr, const uint64_t *__restrict__ st,
                                                                 uint64_t nt, uint32_t S, const int64_t *__restrict__ qpar,
                                                                 const int64_t *__restrict__ DI, uint8_t *__restrict__ BP,
                                                                 uint8_t *__restrict__ MP) {
    const uint32_t j = threadIdx.x % SP;
    const bool live = j < S;
    const uint64_t groups = (uint64_t)gridDim.x * (64 / SP);
    long long qcol[SP];
#pragma unroll
    for (int i = 0; i < SP; ++i) qcol[i] = (live && (uint32_t)i < S) ? (long long)qpar[(uint32_t)i * S + j] : 0ll;
    const long long qp = live ? (long long)qpar[S * S + j] : 0ll;
    for (uint64_t t = (uint64_t)blockIdx.x * (64 / SP) + threadIdx.x / SP; t < nt; t += groups) {
        uint64_t r, a, b;
        bool first;
        chain_scan_tile(ti, sr, st, off, t, r, first, a, b);
        long long d;
        uint64_t w = a;
        if (first) {
            d = chain_maxplus_first(E, M, a, S, j, live, qp);
            w = a + 1;
        } else {
            d = live ? (long long)DI[t * SP + j] : 0ll;
        }
        uint32_t org = j;   // the state before the tile on the best path to state j of the step reached
        (void)chain_maxplus_span<SP>(E, M, w, b, S, j, live, qcol, d, BP, [&](uint32_t k) { org = __shfl(org, k, SP); });
        MP[8 * t + j] = (uint8_t)org;
    }
}

__global__ __launch_bounds__(256) void phk_chain_scan_fold_kernel(const double *__restrict__ XI, const uint64_t *__restrict__ sr,
                                                                  const uint64_t *__restrict__ st, uint64_t ns, uint32_t S,
                                                                  uint32_t SP, double *__restrict__ V) {
    const uint64_t SS = (uint64_t)S * S, Ev = SS + S + 1, G = (uint64_t)SP * SP;
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < ns * SS; x += (uint64_t)gridDim.x * 256) {
        const uint64_t s = x / SS, q = x % SS;
        const double *p = XI + st[s] * G + (q / S) * SP + q % S;
        const uint64_t K = st[s + 1] - st[s];
        double acc = 0.0;
#pragma unroll 16
        for (uint64_t k = 0; k < K; ++k) acc += p[k * G];
        V[sr[s] * Ev + q] = acc;
    }
}

__global__ __launch_bounds__(64) void phk_chain_scan_ends_kernel(const uint64_t *__restrict__ sr, const uint64_t *__restrict__ st,
                                                                 uint64_t ns, const uint8_t *__restrict__ last,
                                                                 const uint64_t *__restrict__ MP, uint8_t *__restrict__ END) {
    for (uint64_t s = (uint64_t)blockIdx.x * 64 + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * 64) {
        const uint64_t t0 = st[s];
        uint32_t x = last[sr[s]];
#pragma unroll 8
        for (uint64_t t = st[s + 1]; t > t0; --t) {
            END[t - 1] = (uint8_t)x;
            x = (uint32_t)(MP[t - 1] >> (8 * x)) & 0xffu;   // (the map of the record's first tile is not followed)
        }
    }
}

__global__ __launch_bounds__(64) void phk_chain_scan_fill_kernel(const uint64_t *__restrict__ off, const uint32_t *__restrict__ ti,
                                                                 const uint64_t *__restrict__ sr, const uint64_t *__restrict__ st,
                                                                 uint64_t nt, const uint8_t *__restrict__ END,
                                                                 const uint64_t *__restrict__ BP, uint8_t *__restrict__ state) {
    for (uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x; t < nt; t += (uint64_t)gridDim.x * 64) {
        uint64_t r, a, b;
        bool first;
        chain_scan_tile(ti, sr, st, off, t, r, first, a, b);
        uint32_t s = END[t];
#pragma unroll 8
        for (uint64_t w = b; w > a; --w) {
            state[w - 1] = (uint8_t)s;
            s = (uint32_t)(BP[w - 1] >> (8 * s)) & 0xffu;
        }
    }
}

extern "C" uint64_t phk_chain_tile(void) { return PHK_CHAIN_TILE; }
extern "C" uint64_t phk_chain_scan_grid_pass(void) { return CH_SCAN_PASS; }

// ---- the resident chain ------------------------------------------------------------------------------------------------
// the tile scan (phk_chain_set_scan) and its buffers
struct ChainScan {
    uint64_t from = 0, ns = 0, nt = 0;     // the threshold at work (0 = every record on the per-record route), scanned
                                           // records, tiles
    uint64_t asked = 0;                    // the threshold as the caller gave it (grouped mode refuses any but 0)
    PhkDevMem ti, sr, st, F, FE, Vq, SM, AI, BO, DI, XI, MP, END;
};

// grouped mode (phk_chain_set_groups) and its buffers
struct ChainGroups {
    uint64_t G = 0;                        // groups of consecutive records; 0 = one set of parameters for every record
    std::vector<uint64_t> off;             // [G + 1] over the records
    std::vector<uint8_t> work;             // per group: at work in the calls after the last phk_chain_set_grouped
    bool tables = false;                   // the descriptor tables below are those of work
    struct Batch { uint64_t wa, nb, d0, d1; };                    // windows wa .. wa + nb - 1, expect descriptors d0 .. d1 - 1
    std::vector<Batch> batches;
    std::vector<std::pair<uint64_t, uint64_t>> levels_v, levels_t;   // fold descriptors [first, last) level by level
    uint64_t ntiles = 0;
    PhkDevMem rg, spans, par, qpar, logp, part, resT, resV, fold, tiles, etiles, folds;
};

struct phk_chain {
    uint64_t n = 0, R = 0, D = 0, B = 0;   // B: rows per batch of the emission and expectation passes
    uint32_t S = 0;
    bool from_counts = false, ready = false;
    const uint32_t *counts = nullptr;      // the batch's rows, or own_counts
    PhkDevMem own_counts, off, E, M, Bt, G, BP, state, par, qpar, logp, V, last, score, Rx, part, fold[2];
    std::vector<uint64_t> h_off;           // the offsets on the host: the tile and group tables are built from them
    ChainScan scan;
    ChainGroups grp;
};

// a member that owns its buffers, as new: what it held is freed (the caller drains the stream if it may be in use)
template <typename T>
static void chain_renew(T &x) {
    x.~T();
    new (&x) T();
}

static unsigned chain_grid(uint64_t items, uint64_t per_block, uint64_t cap) {
    const uint64_t b = phk_div_up(items, per_block);
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

static int chain_check_shape(const char *who, uint64_t n, const uint64_t *offsets, uint64_t R, uint32_t S) {
    PHK_REQUIRE(S >= 2 && S <= PHK_CHAIN_MAX_STATES, "%s: %u states (2 to %d)", who, S, PHK_CHAIN_MAX_STATES);
    PHK_REQUIRE(n <= CH_NMAX && R < (1ull << 32), "%s: more than 2^30 windows or 2^32 records", who);
    if (R == 0) {
        PHK_REQUIRE(n == 0, "%s: %llu windows and no record", who, (unsigned long long)n);
        return PHK_OK;
    }
    PHK_REQUIRE(offsets, "%s: NULL offsets", who);
    PHK_REQUIRE(offsets[0] == 0 && offsets[R] == n, "%s: the offsets do not run from 0 to n", who);
    for (uint64_t r = 0; r < R; ++r)
        PHK_REQUIRE(offsets[r] <= offsets[r + 1], "%s: the offsets decrease at record %llu", who, (unsigned long long)r);
    return PHK_OK;
}

static int chain_alloc(phk_ctx *ctx, const char *who, phk_chain *c, const uint64_t *offsets, uint64_t batch_rows) {
    const uint64_t n = c->n, R = c->R, S = c->S, D = c->D, Ev = S * S + S + 1, Em = S * D + S + 1;
    uint64_t B = (512ull << 20) / (CH_KP * sizeof(double));
    B = B / MIX_RB * MIX_RB;
    if (batch_rows) B = phk_div_up(batch_rows, MIX_RB) * MIX_RB;
    c->B = B;
    const uint64_t Brows = B > n ? n : B, nblocks = phk_div_up(n, MIX_RB);
    const uint64_t fold_v = phk_div_up(R, 256) * Ev, fold_t = c->from_counts ? phk_div_up(nblocks, 256) * Em : 0;
    PHK_TRY(c->off.alloc(who, "offsets", (R + 1) * 8));
    PHK_TRY(c->E.alloc(who, "emissions", n * S * 8));
    PHK_TRY(c->M.alloc(who, "row maxima", n * 8));
    PHK_TRY(c->Bt.alloc(who, "backward vectors", n * S * 8));
    PHK_TRY(c->G.alloc(who, "posteriors", n * S * 8));
    PHK_TRY(c->BP.alloc(who, "backpointers", n * 8));
    PHK_TRY(c->state.alloc(who, "states", n));
    PHK_TRY(c->par.alloc(who, "parameters", (S * S + S) * 8));
    PHK_TRY(c->qpar.alloc(who, "parameters", (S * S + S) * 8));
    PHK_TRY(c->V.alloc(who, "record vectors", R * Ev * 8));
    PHK_TRY(c->last.alloc(who, "last states", R));
    PHK_TRY(c->score.alloc(who, "path scores", R * 8));
    PHK_TRY(c->fold[0].alloc(who, "fold vectors", std::max(fold_v, fold_t) * 8));
    PHK_TRY(c->fold[1].alloc(who, "fold vectors", std::max(fold_v, fold_t) * 8));
    if (c->from_counts) {
        PHK_TRY(c->logp.alloc(who, "log profiles", S * D * 8));
        PHK_TRY(c->Rx.alloc(who, "spread posteriors", Brows * CH_KP * 8));
        PHK_TRY(c->part.alloc(who, "partial vectors", nblocks * Em * 8));
    }
    if (R) PHK_TRY(phk_copy_to_device(ctx, c->off.ptr, offsets, (R + 1) * 8));
    if (R) c->h_off.assign(offsets, offsets + R + 1);
    return PHK_OK;
}

static int chain_finish_create(phk_ctx *ctx, phk_chain *c, int rc, phk_chain **out) {
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        phk_set_error("phk_chain_create: the uploads failed");
        rc = PHK_ERR_HIP;
    }
    if (rc != PHK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        delete c;
        return rc;
    }
    *out = c;
    return PHK_OK;
}

extern "C" int phk_chain_create(phk_ctx *ctx, const uint32_t *counts, uint64_t n, uint64_t D, const uint64_t *offsets, uint64_t R,
                                uint32_t S, uint64_t batch_rows, phk_chain **out) {
    PHK_ENTER(ctx, "phk_chain_create");
    PHK_REQUIRE(out, "phk_chain_create: NULL out");
    *out = nullptr;
    PHK_TRY(chain_check_shape("phk_chain_create", n, offsets, R, S));
    PHK_REQUIRE(D > 0 && D < (1ull << 32), "phk_chain_create: %llu columns", (unsigned long long)D);
    PHK_REQUIRE(n == 0 || counts, "phk_chain_create: NULL counts");
    phk_chain *c = new phk_chain();
    c->n = n, c->R = R, c->D = D, c->S = S, c->from_counts = true;
    int rc = c->own_counts.alloc("phk_chain_create", "count rows", n * D * 4);
    if (rc == PHK_OK && n) rc = phk_copy_to_device(ctx, c->own_counts.ptr, counts, n * D * 4);
    c->counts = c->own_counts.as<uint32_t>();
    if (rc == PHK_OK) rc = chain_alloc(ctx, "phk_chain_create", c, offsets, batch_rows);
    return chain_finish_create(ctx, c, rc, out);
}

extern "C" int phk_batch_chain_create(phk_ctx *ctx, const phk_batch *b, const uint64_t *offsets, uint64_t R, uint32_t S,
                                      uint64_t batch_rows, phk_chain **out) {
    PHK_ENTER(ctx, "phk_batch_chain_create");
    PHK_REQUIRE(out, "phk_batch_chain_create: NULL out");
    *out = nullptr;
    PHK_REQUIRE(b, "phk_batch_chain_create: NULL batch");
    PHK_TRY(chain_check_shape("phk_batch_chain_create", b->n, offsets, R, S));
    PHK_REQUIRE(b->D > 0, "phk_batch_chain_create: a batch without columns");
    phk_chain *c = new phk_chain();
    c->n = b->n, c->R = R, c->D = b->D, c->S = S, c->from_counts = true;
    c->counts = b->d_counts;   // read where they lie: the batch outlives the chain
    return chain_finish_create(ctx, c, chain_alloc(ctx, "phk_batch_chain_create", c, offsets, batch_rows), out);
}

extern "C" int phk_chain_create_from_emissions(phk_ctx *ctx, const double *E, uint64_t n, const uint64_t *offsets, uint64_t R,
                                               uint32_t S, phk_chain **out) {
    PHK_ENTER(ctx, "phk_chain_create_from_emissions");
    PHK_REQUIRE(out, "phk_chain_create_from_emissions: NULL out");
    *out = nullptr;
    PHK_TRY(chain_check_shape("phk_chain_create_from_emissions", n, offsets, R, S));
    PHK_REQUIRE(n == 0 || E, "phk_chain_create_from_emissions: NULL emissions");
    if (n && !phk_rows_finite(E, n * S)) {
        phk_set_error("phk_chain_create_from_emissions: an emission is not finite");
        return PHK_ERR_NAN;
    }
    phk_chain *c = new phk_chain();
    c->n = n, c->R = R, c->D = 0, c->S = S, c->from_counts = false;
    int rc = chain_alloc(ctx, "phk_chain_create_from_emissions", c, offsets, 0);
    if (rc == PHK_OK && n) rc = phk_copy_to_device(ctx, c->E.ptr, E, n * S * 8);
    if (rc == PHK_OK && n) {
        rc = [&]() -> int {
            PHK_LAUNCH(ctx, "phk_chain_rowmax_kernel",
                       phk_chain_rowmax_kernel<<<dim3(chain_grid(n, 256, 4096)), dim3(256), 0, ctx->stream>>>(
                           c->E.as<double>(), n, S, c->M.as<double>()));
            return PHK_OK;
        }();
    }
    return chain_finish_create(ctx, c, rc, out);
}

extern "C" int phk_chain_destroy(phk_ctx *ctx, phk_chain *c) {
    if (!c) return PHK_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete c;
    return PHK_OK;
}

static int chain_scan_alloc(phk_ctx *ctx, ChainScan &s, uint32_t S, const std::vector<uint32_t> &ti,
                            const std::vector<uint64_t> &sr, const std::vector<uint64_t> &st) {
    const char *who = "phk_chain_set_scan";
    const uint64_t nt = ti.size(), ns = sr.size(), SP = S <= 2 ? 2 : (S <= 4 ? 4 : 8), G = SP * SP;
    PHK_TRY(s.ti.alloc(who, "tile table", nt * 4));
    PHK_TRY(s.sr.alloc(who, "tile table", ns * 8));
    PHK_TRY(s.st.alloc(who, "tile table", (ns + 1) * 8));
    PHK_TRY(s.F.alloc(who, "tile matrices", nt * G * 8));
    PHK_TRY(s.FE.alloc(who, "tile exponents", nt * 4));
    PHK_TRY(s.Vq.alloc(who, "tile matrices", nt * G * 8));
    PHK_TRY(s.SM.alloc(who, "tile sums", nt * 8));
    PHK_TRY(s.AI.alloc(who, "entering vectors", nt * SP * 8));
    PHK_TRY(s.BO.alloc(who, "entering vectors", nt * SP * 8));
    PHK_TRY(s.DI.alloc(who, "entering vectors", nt * SP * 8));
    PHK_TRY(s.XI.alloc(who, "tile vectors", nt * G * 8));
    PHK_TRY(s.MP.alloc(who, "tile maps", nt * 8));
    PHK_TRY(s.END.alloc(who, "tile end states", nt));
    PHK_TRY(phk_copy_to_device(ctx, s.ti.ptr, ti.data(), nt * 4));
    PHK_TRY(phk_copy_to_device(ctx, s.sr.ptr, sr.data(), ns * 8));
    PHK_TRY(phk_copy_to_device(ctx, s.st.ptr, st.data(), (ns + 1) * 8));
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // the tables leave scope
    return PHK_OK;
}

extern "C" int phk_chain_set_scan(phk_ctx *ctx, phk_chain *c, uint64_t scan_from) {
    PHK_ENTER(ctx, "phk_chain_set_scan");
    PHK_REQUIRE(c, "phk_chain_set_scan: NULL chain");
    PHK_REQUIRE(!(c->grp.G && scan_from), "phk_chain_set_scan: a grouped chain does not take the tile scan");
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // the buffers of an earlier threshold may be in use
    chain_renew(c->scan);
    c->scan.asked = scan_from;
    if (scan_from == 0 || c->n == 0) return PHK_OK;
    std::vector<uint32_t> ti;
    std::vector<uint64_t> sr, st;
    for (uint64_t r = 0; r < c->R; ++r) {
        const uint64_t len = c->h_off[r + 1] - c->h_off[r];
        if (len < scan_from) continue;   // (scan_from >= 1: a record without windows is never scanned)
        st.push_back(ti.size());
        ti.insert(ti.end(), phk_div_up(len, PHK_CHAIN_TILE), (uint32_t)sr.size());
        sr.push_back(r);
    }
    if (sr.empty()) return PHK_OK;
    st.push_back(ti.size());
    const int rc = chain_scan_alloc(ctx, c->scan, c->S, ti, sr, st);
    if (rc != PHK_OK) {
        chain_renew(c->scan);
        return rc;
    }
    c->scan.from = scan_from, c->scan.ns = sr.size(), c->scan.nt = ti.size();
    return PHK_OK;
}

#define CHAIN_BY_SP(S, CALL)  \
    do {                      \
        if ((S) <= 2) {       \
            CALL(2);          \
        } else if ((S) <= 4) {\
            CALL(4);          \
        } else {              \
            CALL(8);          \
        }                     \
    } while (0)

// the two variants of a loader: FULL (gram_tile: the columns fill whole chunks) or VEC (mix_expect_body: rows of whole float4)
#define CHAIN_BY_FLAG(FLAG, CALL) \
    do {                          \
        if (FLAG) {               \
            CALL(true);           \
        } else {                  \
            CALL(false);          \
        }                         \
    } while (0)

static int chain_emit(phk_ctx *ctx, phk_chain *c, double temper) {
    const uint64_t n = c->n, D = c->D;
    for (uint64_t s = 0; s < n; s += c->B) {
        const uint64_t nb = n - s < c->B ? n - s : c->B;
        const dim3 grid((unsigned)phk_div_up(nb, GT_QB)), blk(GT_WAVES * 64);
        double *E = c->E.as<double>() + s * c->S, *M = c->M.as<double>() + s;
#define CH_EMIT(FULL)                                                                                                         \
        PHK_LAUNCH(ctx, "phk_chain_emit_kernel", phk_chain_emit_kernel<FULL><<<grid, blk, 0, ctx->stream>>>(                  \
                                                     c->counts + s * D, nb, c->logp.as<double>(), c->S, D, temper, E, M))
        CHAIN_BY_FLAG(D % GT_KC == 0, CH_EMIT);
#undef CH_EMIT
    }
    return PHK_OK;
}

// A in (0, 1), pi in (0, 1), every row of A and pi summing to 1 within 4 ulp of 1, the quantised logarithms in [-2^31, 0];
// a message names the group (between the entry point's name and its text) unless group < 0
static int chain_check_params(const char *who, long long group, uint32_t S, const double *trans, const double *init,
                              const int64_t *qlog_trans, const int64_t *qlog_init) {
    char prefix[40] = "";
    auto where = [&]() -> const char * {   // written only for a message: the check runs per group and call
        if (group >= 0) snprintf(prefix, sizeof prefix, "group %lld: ", group);
        return prefix;
    };
    for (uint32_t i = 0; i < S * S; ++i)
        PHK_REQUIRE(trans[i] > 0.0 && trans[i] < 1.0, "%s: %stransition probability %u = %g is not in (0, 1)", who, where(), i,
                    trans[i]);
    for (uint32_t i = 0; i < S; ++i)
        PHK_REQUIRE(init[i] > 0.0 && init[i] < 1.0, "%s: %sinitial probability %u = %g is not in (0, 1)", who, where(), i, init[i]);
    for (uint32_t i = 0; i <= S; ++i) {
        const double *row = i < S ? trans + i * S : init;
        double sum = 0.0;
        for (uint32_t j = 0; j < S; ++j) sum += row[j];
        PHK_REQUIRE(fabs(sum - 1.0) <= 4.0 * 0x1p-52, "%s: %srow %u of the transition matrix (row %u: the initial distribution) "
                                                      "does not sum to 1", who, where(), i, S);
    }
    for (uint32_t i = 0; i < S * S + S; ++i) {
        const int64_t q = i < S * S ? qlog_trans[i] : qlog_init[i - S * S];
        PHK_REQUIRE(q <= 0 && q >= -CH_QMAX, "%s: %squantised logarithm %u = %lld is not in [-2^31, 0]", who, where(), i,
                    (long long)q);
    }
    return PHK_OK;
}

extern "C" int phk_chain_set(phk_ctx *ctx, phk_chain *c, const double *log_profiles, uint64_t D, const double *trans,
                             const double *init, const int64_t *qlog_trans, const int64_t *qlog_init, double temper) {
    PHK_ENTER(ctx, "phk_chain_set");
    PHK_REQUIRE(c, "phk_chain_set: NULL chain");
    PHK_REQUIRE(!c->grp.G, "phk_chain_set: a grouped chain takes its parameters from phk_chain_set_grouped");
    PHK_REQUIRE(trans && init && qlog_trans && qlog_init, "phk_chain_set: NULL parameters");
    const uint32_t S = c->S;
    PHK_TRY(chain_check_params("phk_chain_set", -1, S, trans, init, qlog_trans, qlog_init));
    PHK_REQUIRE(temper > 0.0 && temper - temper == 0.0, "phk_chain_set: temper = %g is not finite and > 0", temper);
    if (c->from_counts) {
        PHK_REQUIRE(log_profiles, "phk_chain_set: NULL log profiles");
        PHK_REQUIRE(D == c->D, "phk_chain_set: the profiles have %llu columns, the count rows %llu", (unsigned long long)D,
                    (unsigned long long)c->D);
        if (!phk_rows_finite(log_profiles, (uint64_t)S * D)) {
            phk_set_error("phk_chain_set: the log profiles hold a value that is not finite (a zero profile entry?)");
            return PHK_ERR_NAN;
        }
    } else {
        PHK_REQUIRE(!log_profiles, "phk_chain_set: a chain made from emissions takes no profiles");
    }
    c->ready = false;
    double par[PHK_CHAIN_MAX_STATES * PHK_CHAIN_MAX_STATES + PHK_CHAIN_MAX_STATES];
    int64_t qpar[PHK_CHAIN_MAX_STATES * PHK_CHAIN_MAX_STATES + PHK_CHAIN_MAX_STATES];
    std::copy(trans, trans + S * S, par), std::copy(init, init + S, par + S * S);
    std::copy(qlog_trans, qlog_trans + S * S, qpar), std::copy(qlog_init, qlog_init + S, qpar + S * S);
    int rc = phk_copy_to_device(ctx, c->par.ptr, par, (S * S + S) * 8);
    if (rc == PHK_OK) rc = phk_copy_to_device(ctx, c->qpar.ptr, qpar, (S * S + S) * 8);
    if (rc == PHK_OK && c->from_counts) rc = phk_copy_to_device(ctx, c->logp.ptr, log_profiles, (uint64_t)S * D * 8);
    if (rc == PHK_OK && c->from_counts && c->n) rc = chain_emit(ctx, c, temper);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PHK_OK) {   // par and qpar leave scope
        phk_set_error("phk_chain_set: the stream failed");
        rc = PHK_ERR_HIP;
    }
    c->ready = rc == PHK_OK;
    return rc;
}

static int chain_group_forward_backward(phk_ctx *ctx, const phk_chain *c);
static int chain_group_viterbi(phk_ctx *ctx, const phk_chain *c);
template <typename T>
static void chain_group_zero(const phk_chain *c, T *x, uint64_t per, T *y);

extern "C" int phk_chain_emissions(phk_ctx *ctx, const phk_chain *c, double *E) {
    PHK_ENTER(ctx, "phk_chain_emissions");
    PHK_REQUIRE(c && c->ready, "phk_chain_emissions: no chain, or phk_chain_set has not succeeded on it");
    if (c->n == 0) return PHK_OK;
    PHK_REQUIRE(E, "phk_chain_emissions: NULL pointer");
    PHK_TRY(phk_copy_to_host(ctx, E, c->E.ptr, c->n * c->S * 8));
    if (c->grp.G) chain_group_zero<double>(c, E, c->S, nullptr);   // a group that is not at work has no emissions
    return PHK_OK;
}

// the scanned records' tiles: F, Vq and the sums of M
static int chain_scan_tiles(phk_ctx *ctx, const phk_chain *c) {
    const ChainScan &s = c->scan;
#define CH_TILES(SP)                                                                                                          \
    PHK_LAUNCH(ctx, "phk_chain_scan_tile_kernel",                                                                             \
               phk_chain_scan_tile_kernel<SP>                                                                                 \
               <<<dim3(chain_grid(s.nt, 64 / (SP * SP), CH_SCAN_PASS / (64 / (SP * SP)))), dim3(64), 0, ctx->stream>>>(       \
                   c->E.as<double>(), c->M.as<double>(), c->off.as<uint64_t>(), s.ti.as<uint32_t>(), s.sr.as<uint64_t>(),     \
                   s.st.as<uint64_t>(), s.nt, c->S, c->par.as<double>(), c->qpar.as<int64_t>(), s.F.as<double>(),             \
                   s.FE.as<int32_t>(), s.Vq.as<int64_t>(), s.SM.as<double>()))
    CHAIN_BY_SP(c->S, CH_TILES);
#undef CH_TILES
    return PHK_OK;
}

// the carry over the scanned records' tiles: `roles` roles from `role0` on (0 alpha, 1 beta, 2 delta)
static int chain_scan_carry(phk_ctx *ctx, const phk_chain *c, uint32_t role0, uint32_t roles) {
    const ChainScan &s = c->scan;
#define CH_CARRY(SP)                                                                                                          \
    PHK_LAUNCH(ctx, "phk_chain_scan_carry_kernel",                                                                            \
               phk_chain_scan_carry_kernel<SP>                                                                                \
               <<<dim3(chain_grid(s.ns, 64 / (SP * SP), CH_BLOCKS_MAX), roles), dim3(64), 0, ctx->stream>>>(                  \
                   s.F.as<double>(), s.FE.as<int32_t>(), s.Vq.as<int64_t>(), s.SM.as<double>(), s.sr.as<uint64_t>(),          \
                   s.st.as<uint64_t>(), s.ns, c->S, role0, s.AI.as<double>(), s.BO.as<double>(), s.DI.as<int64_t>(),          \
                   c->V.as<double>(), c->score.as<int64_t>(), c->last.as<uint8_t>()))
    CHAIN_BY_SP(c->S, CH_CARRY);
#undef CH_CARRY
    return PHK_OK;
}

// forward-backward of the scanned records (after chain_scan_tiles): B, G and V as the per-record kernels leave them
static int chain_scan_forward_backward(phk_ctx *ctx, const phk_chain *c) {
    const ChainScan &s = c->scan;
    PHK_TRY(chain_scan_carry(ctx, c, 0, 2));
#define CH_WALK(SP)                                                                                                           \
    PHK_LAUNCH(ctx, "phk_chain_scan_walk_kernel",                                                                             \
               phk_chain_scan_walk_kernel<SP>                                                                                 \
               <<<dim3(chain_grid(s.nt, 64 / SP, CH_SCAN_PASS / (64 / SP))), dim3(64), 0, ctx->stream>>>(                     \
                   c->E.as<double>(), c->M.as<double>(), c->off.as<uint64_t>(), s.ti.as<uint32_t>(), s.sr.as<uint64_t>(),     \
                   s.st.as<uint64_t>(), s.nt, c->S, c->par.as<double>(), s.AI.as<double>(), s.BO.as<double>(),                \
                   c->Bt.as<double>(), c->G.as<double>(), s.XI.as<double>(), c->V.as<double>()));                             \
    PHK_LAUNCH(ctx, "phk_chain_scan_fold_kernel",                                                                             \
               phk_chain_scan_fold_kernel<<<dim3(chain_grid(s.ns * c->S * c->S, 256, 4096)), dim3(256), 0, ctx->stream>>>(    \
                   s.XI.as<double>(), s.sr.as<uint64_t>(), s.st.as<uint64_t>(), s.ns, c->S, SP, c->V.as<double>()))
    CHAIN_BY_SP(c->S, CH_WALK);
#undef CH_WALK
    return PHK_OK;
}

// the max-plus half of the scanned records (after chain_scan_tiles): BP, state, score and last as the per-record kernels
// leave them
static int chain_scan_path(phk_ctx *ctx, const phk_chain *c) {
    const ChainScan &s = c->scan;
    PHK_TRY(chain_scan_carry(ctx, c, 2, 1));
#define CH_PATH(SP)                                                                                                           \
    PHK_LAUNCH(ctx, "phk_chain_scan_path_kernel",                                                                             \
               phk_chain_scan_path_kernel<SP>                                                                                 \
               <<<dim3(chain_grid(s.nt, 64 / SP, CH_SCAN_PASS / (64 / SP))), dim3(64), 0, ctx->stream>>>(                     \
                   c->E.as<double>(), c->M.as<double>(), c->off.as<uint64_t>(), s.ti.as<uint32_t>(), s.sr.as<uint64_t>(),     \
                   s.st.as<uint64_t>(), s.nt, c->S, c->qpar.as<int64_t>(), s.DI.as<int64_t>(), c->BP.as<uint8_t>(),           \
                   s.MP.as<uint8_t>()))
    CHAIN_BY_SP(c->S, CH_PATH);
#undef CH_PATH
    PHK_LAUNCH(ctx, "phk_chain_scan_ends_kernel",
               phk_chain_scan_ends_kernel<<<dim3(chain_grid(s.ns, 64, CH_BLOCKS_MAX)), dim3(64), 0, ctx->stream>>>(
                   s.sr.as<uint64_t>(), s.st.as<uint64_t>(), s.ns, c->last.as<uint8_t>(), s.MP.as<uint64_t>(),
                   s.END.as<uint8_t>()));
    PHK_LAUNCH(ctx, "phk_chain_scan_fill_kernel",
               phk_chain_scan_fill_kernel<<<dim3(chain_grid(s.nt, 64, CH_SCAN_PASS / 64)), dim3(64), 0, ctx->stream>>>(
                   c->off.as<uint64_t>(), s.ti.as<uint32_t>(), s.sr.as<uint64_t>(), s.st.as<uint64_t>(), s.nt,
                   s.END.as<uint8_t>(), c->BP.as<uint64_t>(), c->state.as<uint8_t>()));
    return PHK_OK;
}

// backward then forward over every record: B, G and the records' vectors V
static int chain_forward_backward(phk_ctx *ctx, const phk_chain *c) {
    const double *E = c->E.as<double>(), *M = c->M.as<double>(), *par = c->par.as<double>();
    const uint64_t *off = c->off.as<uint64_t>(), sf = c->scan.from;
    if (sf) PHK_TRY(chain_scan_forward_backward(ctx, c));
#define CH_FB(SP)                                                                                                             \
    {                                                                                                                         \
        const dim3 grid(chain_grid(c->R, 64 / SP, CH_BLOCKS_MAX));                                                            \
        PHK_LAUNCH(ctx, "phk_chain_backward_kernel", phk_chain_backward_kernel<SP><<<grid, dim3(64), 0, ctx->stream>>>(       \
                                                         E, M, off, c->R, c->S, par, c->Bt.as<double>(), sf));                \
        PHK_LAUNCH(ctx, "phk_chain_forward_kernel",                                                                           \
                   phk_chain_forward_kernel<SP><<<grid, dim3(64), 0, ctx->stream>>>(E, M, off, c->R, c->S, par,               \
                                                                                    c->Bt.as<double>(), c->G.as<double>(),    \
                                                                                    c->V.as<double>(), sf));                  \
    }
    CHAIN_BY_SP(c->S, CH_FB);
#undef CH_FB
    return PHK_OK;
}

// the fixed tree over m vectors of Ev doubles, level after level; *out = the one vector left (in a fold buffer)
static int chain_fold(phk_ctx *ctx, const phk_chain *c, const double *in, uint64_t m, uint64_t Ev, const double **out) {
    for (int level = 0;; ++level) {
        const uint64_t blocks = phk_div_up(m, 256);
        double *dst = c->fold[level & 1].as<double>();
        PHK_LAUNCH(ctx, "phk_chain_fold_kernel",
                   phk_chain_fold_kernel<<<dim3((unsigned)phk_div_up(Ev, 256), (unsigned)blocks), dim3(256), 0, ctx->stream>>>(
                       in, m, Ev, dst));
        in = dst, m = blocks;
        if (blocks == 1) break;
    }
    *out = in;
    return PHK_OK;
}

// out[r] = the log evidence of record r: the last entry of its vector V[r]
static int chain_record_evidence(phk_ctx *ctx, const phk_chain *c, double *out) {
    const uint64_t R = c->R, Ev = (uint64_t)c->S * c->S + c->S + 1;
    std::vector<double> rec(R * Ev);
    PHK_TRY(phk_copy_to_host(ctx, rec.data(), c->V.ptr, R * Ev * 8));
    for (uint64_t r = 0; r < R; ++r) out[r] = rec[r * Ev + Ev - 1];
    return PHK_OK;
}

static int chain_expect_run(phk_ctx *ctx, const phk_chain *c, double *T, double *Ns, double *xi, double *gamma0,
                            double *log_evidence, double *log_evidence_rec) {
    const uint64_t S = c->S, D = c->D, R = c->R, n = c->n, Ev = S * S + S + 1, Em = S * D + S + 1;
    if (c->scan.from) PHK_TRY(chain_scan_tiles(ctx, c));
    PHK_TRY(chain_forward_backward(ctx, c));
    const double *tot;
    PHK_TRY(chain_fold(ctx, c, c->V.as<double>(), R, Ev, &tot));
    std::vector<double> v(Ev);
    PHK_TRY(phk_copy_to_host(ctx, v.data(), tot, Ev * 8));
    std::copy(v.begin(), v.begin() + S * S, xi);
    std::copy(v.begin() + S * S, v.begin() + S * S + S, gamma0);
    *log_evidence = v[S * S + S];
    if (log_evidence_rec) PHK_TRY(chain_record_evidence(ctx, c, log_evidence_rec));
    if (!T) return PHK_OK;
    for (uint64_t s = 0; s < n; s += c->B) {
        const uint64_t nb = n - s < c->B ? n - s : c->B;
        PHK_LAUNCH(ctx, "phk_chain_spread_kernel",
                   phk_chain_spread_kernel<<<dim3(chain_grid(nb * CH_KP, 256, 4096)), dim3(256), 0, ctx->stream>>>(
                       c->G.as<double>() + s * S, nb, (uint32_t)S, c->Rx.as<double>()));
        const dim3 grid((unsigned)phk_div_up(nb, MIX_RB), (unsigned)phk_div_up(D, GT_WAVES * MIX_CT)), blk(GT_WAVES * 64);
        double *part = c->part.as<double>() + (s / MIX_RB) * Em;
#define CH_EXPECT(VEC)                                                                                                        \
        PHK_LAUNCH(ctx, "phk_chain_expect_kernel", phk_chain_expect_kernel<VEC><<<grid, blk, 0, ctx->stream>>>(               \
                                                       c->Rx.as<double>(), c->counts + s * D, D, nb, c->M.as<double>() + s,   \
                                                       (uint32_t)S, Em, part))
        CHAIN_BY_FLAG(D % 4 == 0, CH_EXPECT);
#undef CH_EXPECT
    }
    PHK_TRY(chain_fold(ctx, c, c->part.as<double>(), phk_div_up(n, MIX_RB), Em, &tot));
    std::vector<double> t(Em);
    PHK_TRY(phk_copy_to_host(ctx, t.data(), tot, Em * 8));
    std::copy(t.begin(), t.begin() + S * D, T);
    std::copy(t.begin() + S * D, t.begin() + S * D + S, Ns);
    return PHK_OK;
}

extern "C" int phk_chain_expect(phk_ctx *ctx, const phk_chain *c, double *T, double *Ns, double *xi, double *gamma0,
                                double *log_evidence, double *log_evidence_rec) {
    PHK_ENTER(ctx, "phk_chain_expect");
    PHK_REQUIRE(c && c->ready, "phk_chain_expect: no chain, or phk_chain_set has not succeeded on it");
    PHK_REQUIRE(!c->grp.G, "phk_chain_expect: a grouped chain gives its expectations through phk_chain_expect_grouped");
    PHK_REQUIRE(xi && gamma0 && log_evidence, "phk_chain_expect: NULL pointer");
    PHK_REQUIRE(!T == !Ns, "phk_chain_expect: T and Ns go together");
    PHK_REQUIRE(!T || c->from_counts, "phk_chain_expect: a chain made from emissions has no T");
    const uint64_t S = c->S;
    if (c->n == 0) {
        std::fill(xi, xi + S * S, 0.0), std::fill(gamma0, gamma0 + S, 0.0);
        *log_evidence = 0.0;
        if (T) std::fill(T, T + S * c->D, 0.0), std::fill(Ns, Ns + S, 0.0);
        for (uint64_t r = 0; log_evidence_rec && r < c->R; ++r) log_evidence_rec[r] = 0.0;
        return PHK_OK;
    }
    const int rc = chain_expect_run(ctx, c, T, Ns, xi, gamma0, log_evidence, log_evidence_rec);
    if (rc != PHK_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

static int chain_decode_run(phk_ctx *ctx, const phk_chain *c, uint8_t *state, double *posterior, double *log_evidence_rec,
                            int64_t *path_score) {
    const uint64_t S = c->S, R = c->R, n = c->n;
    const uint64_t *off = c->off.as<uint64_t>(), sf = c->scan.from;
    if (c->grp.G) {   // every record with its group's parameters; the trace needs none
        if (posterior || log_evidence_rec) PHK_TRY(chain_group_forward_backward(ctx, c));
        PHK_TRY(chain_group_viterbi(ctx, c));
    } else {
        if (sf) PHK_TRY(chain_scan_tiles(ctx, c));
        if (posterior || log_evidence_rec) PHK_TRY(chain_forward_backward(ctx, c));
        if (sf) PHK_TRY(chain_scan_path(ctx, c));
#define CH_VIT(SP)                                                                                                        \
        PHK_LAUNCH(ctx, "phk_chain_viterbi_kernel",                                                                           \
                   phk_chain_viterbi_kernel<SP><<<dim3(chain_grid(R, 64 / SP, CH_BLOCKS_MAX)), dim3(64), 0, ctx->stream>>>(   \
                       c->E.as<double>(), c->M.as<double>(), off, R, c->S, c->qpar.as<int64_t>(), c->BP.as<uint8_t>(),        \
                       c->score.as<int64_t>(), c->last.as<uint8_t>(), sf))
        CHAIN_BY_SP(c->S, CH_VIT);
#undef CH_VIT
    }
    PHK_LAUNCH(ctx, "phk_chain_trace_kernel",
               phk_chain_trace_kernel<<<dim3(chain_grid(R, 64, CH_BLOCKS_MAX)), dim3(64), 0, ctx->stream>>>(
                   off, R, c->last.as<uint8_t>(), c->BP.as<uint64_t>(), c->state.as<uint8_t>(), sf));
    PHK_TRY(phk_copy_to_host(ctx, state, c->state.ptr, n));
    if (path_score) PHK_TRY(phk_copy_to_host(ctx, path_score, c->score.ptr, R * 8));
    if (posterior) PHK_TRY(phk_copy_to_host(ctx, posterior, c->G.ptr, n * S * 8));
    if (log_evidence_rec) PHK_TRY(chain_record_evidence(ctx, c, log_evidence_rec));
    if (c->grp.G) {   // zeros for the groups that are not at work
        chain_group_zero<uint8_t>(c, state, 1, nullptr);
        if (posterior) chain_group_zero<double>(c, posterior, S, nullptr);
        if (log_evidence_rec) chain_group_zero<double>(c, nullptr, 0, log_evidence_rec);
        if (path_score) chain_group_zero<int64_t>(c, nullptr, 0, path_score);
    }
    return PHK_OK;
}

extern "C" int phk_chain_decode(phk_ctx *ctx, const phk_chain *c, uint8_t *state, double *posterior, double *log_evidence_rec,
                                int64_t *path_score) {
    PHK_ENTER(ctx, "phk_chain_decode");
    PHK_REQUIRE(c && c->ready, "phk_chain_decode: no chain, or phk_chain_set has not succeeded on it");
    if (c->n == 0) {
        for (uint64_t r = 0; r < c->R; ++r) {
            if (log_evidence_rec) log_evidence_rec[r] = 0.0;
            if (path_score) path_score[r] = 0;
        }
        return PHK_OK;
    }
    PHK_REQUIRE(state, "phk_chain_decode: NULL state");
    const int rc = chain_decode_run(ctx, c, state, posterior, log_evidence_rec, path_score);
    if (rc != PHK_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// ---- grouped chains: the host half ----------------------------------------------------------------------
// the windows [w0, w1) of group g
static inline void chain_group_span(const phk_chain *c, uint64_t g, uint64_t &w0, uint64_t &w1) {
    const uint64_t r0 = c->grp.off[g], r1 = c->grp.off[g + 1];
    w0 = c->R ? c->h_off[r0] : 0, w1 = c->R ? c->h_off[r1] : 0;
}

extern "C" int phk_chain_set_groups(phk_ctx *ctx, phk_chain *c, const uint64_t *group_offsets, uint64_t G) {
    const char *who = "phk_chain_set_groups";
    PHK_ENTER(ctx, "phk_chain_set_groups");
    PHK_REQUIRE(c, "%s: NULL chain", who);
    if (G == 0) {
        PHK_REQUIRE(!group_offsets, "%s: offsets and no group", who);
        if (!c->grp.G) return PHK_OK;
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        chain_renew(c->grp);
        c->ready = false;   // (the parameters of the calls that follow come from phk_chain_set)
        return PHK_OK;
    }
    PHK_REQUIRE(c->from_counts, "%s: a chain made from emissions has no groups", who);
    PHK_REQUIRE(c->scan.asked == 0, "%s: the tile scan is on (phk_chain_set_scan): grouped chains do not take it", who);
    PHK_REQUIRE(group_offsets, "%s: NULL offsets", who);
    PHK_REQUIRE(G < CH_NO_GROUP, "%s: 2^32 - 1 groups or more", who);
    PHK_REQUIRE(group_offsets[0] == 0 && group_offsets[G] == c->R, "%s: the group offsets do not run from 0 to the %llu records",
                who, (unsigned long long)c->R);
    for (uint64_t g = 0; g < G; ++g)
        PHK_REQUIRE(group_offsets[g] <= group_offsets[g + 1], "%s: the group offsets decrease at group %llu", who,
                    (unsigned long long)g);
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // the buffers of earlier groups may be in use
    chain_renew(c->grp);
    c->ready = false;
    c->grp.off.assign(group_offsets, group_offsets + G + 1);
    c->grp.G = G;
    const uint64_t S = c->S, D = c->D, PS = S * S + S, Ev = PS + 1, Em = S * D + S + 1;
    // every group at work at once: its blocks' partial vectors, and two fold buffers per tree that has a second level
    std::vector<ChainGroup> grp(G);
    uint64_t blocks = 0, fold = 0;
    for (uint64_t g = 0; g < G; ++g) {
        uint64_t w0, w1;
        chain_group_span(c, g, w0, w1);
        grp[g] = ChainGroup{w0, w1 - w0};
        const uint64_t nb = phk_div_up(w1 - w0, MIX_RB), nr = c->grp.off[g + 1] - c->grp.off[g];
        blocks += nb;
        if (nb > 256) fold += 2 * phk_div_up(nb, 256) * Em;
        if (nr > 256) fold += 2 * phk_div_up(nr, 256) * Ev;
    }
    auto body = [&]() -> int {
        PHK_TRY(c->grp.rg.alloc(who, "record groups", c->R * 4));
        PHK_TRY(c->grp.spans.alloc(who, "groups", G * sizeof(ChainGroup)));
        PHK_TRY(c->grp.par.alloc(who, "parameters", G * PS * 8));
        PHK_TRY(c->grp.qpar.alloc(who, "parameters", G * PS * 8));
        PHK_TRY(c->grp.logp.alloc(who, "log profiles", G * S * D * 8));
        PHK_TRY(c->grp.part.alloc(who, "partial vectors", blocks * Em * 8));
        PHK_TRY(c->grp.resT.alloc(who, "group vectors", G * Em * 8));
        PHK_TRY(c->grp.resV.alloc(who, "group vectors", G * Ev * 8));
        PHK_TRY(c->grp.fold.alloc(who, "fold vectors", fold * 8));
        PHK_TRY(phk_copy_to_device(ctx, c->grp.spans.ptr, grp.data(), G * sizeof(ChainGroup)));
        if (c->R) PHK_HIP(hipMemsetAsync(c->last.ptr, 0, c->R, ctx->stream));   // the trace reads it for every record
        PHK_HIP(hipStreamSynchronize(ctx->stream));   // grp leaves scope
        return PHK_OK;
    };
    const int rc = body();
    if (rc != PHK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        chain_renew(c->grp);
    }
    return rc;
}

// The tables of the groups at work (c->grp.work): the records' groups, the emission tiles, the expectation blocks in batches
// of at most c->B consecutive windows, the fold levels of the records' vectors and of the blocks' partial vectors.
static int chain_group_tables(phk_ctx *ctx, phk_chain *c) {
    const char *who = "phk_chain_set_grouped";
    const uint64_t G = c->grp.G, S = c->S, D = c->D, Ev = S * S + S + 1, Em = S * D + S + 1;
    const uint64_t ygroups = phk_div_up(D, GT_WAVES * MIX_CT), cap = c->B > c->n ? c->n : c->B;
    std::vector<uint32_t> rg(c->R, CH_NO_GROUP);
    std::vector<ChainGroupTile> tiles, etiles;
    std::vector<ChainGroupFold> folds;
    c->grp.batches.clear(), c->grp.levels_v.clear(), c->grp.levels_t.clear();
    struct Live { const double *in; double *res, *f[2]; uint64_t m; };
    std::vector<Live> live_v, live_t;
    uint64_t part_at = 0, fold_at = 0;
    double *part = c->grp.part.as<double>(), *fold = c->grp.fold.as<double>();
    for (uint64_t g = 0; g < G; ++g) {
        if (!c->grp.work[g]) continue;
        uint64_t w0, w1;
        chain_group_span(c, g, w0, w1);
        const uint64_t r0 = c->grp.off[g], r1 = c->grp.off[g + 1], n = w1 - w0, nb = phk_div_up(n, MIX_RB);
        std::fill(rg.begin() + r0, rg.begin() + r1, (uint32_t)g);
        for (uint64_t t = 0; t < phk_div_up(n, GT_QB); ++t) tiles.push_back(ChainGroupTile{(uint32_t)g, (uint32_t)t, 0, 0, 0});
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t a = w0 + b * MIX_RB, e = a + MIX_RB < w1 ? a + MIX_RB : w1;
            if (c->grp.batches.empty() || e - c->grp.batches.back().wa > cap)
                c->grp.batches.push_back(ChainGroups::Batch{a, 0, etiles.size(), etiles.size()});
            for (uint64_t y = 0; y < ygroups; ++y)
                etiles.push_back(ChainGroupTile{(uint32_t)g, (uint32_t)b, (uint32_t)y, 0, part_at + b});
            c->grp.batches.back().nb = e - c->grp.batches.back().wa, c->grp.batches.back().d1 = etiles.size();
        }
        Live t{part + part_at * Em, c->grp.resT.as<double>() + g * Em, {nullptr, nullptr}, nb};
        if (nb > 256) t.f[0] = fold + fold_at, t.f[1] = t.f[0] + phk_div_up(nb, 256) * Em, fold_at += 2 * phk_div_up(nb, 256) * Em;
        live_t.push_back(t);
        Live v{c->V.as<double>() + r0 * Ev, c->grp.resV.as<double>() + g * Ev, {nullptr, nullptr}, r1 - r0};
        if (v.m > 256) v.f[0] = fold + fold_at, v.f[1] = v.f[0] + phk_div_up(v.m, 256) * Ev, fold_at += 2 * phk_div_up(v.m, 256) * Ev;
        live_v.push_back(v);
        part_at += nb;
    }
    // a group's level reads m vectors and writes ceil(m / 256); the last one is the group's result
    auto levels = [&](std::vector<Live> &live, uint64_t E, std::vector<std::pair<uint64_t, uint64_t>> &out) {
        for (int level = 0; !live.empty(); ++level) {
            const uint64_t first = folds.size();
            std::vector<Live> next;
            for (Live &v : live) {
                const uint64_t blocks = phk_div_up(v.m, 256);
                double *o = blocks == 1 ? v.res : v.f[level & 1];
                for (uint64_t vb = 0; vb < blocks; ++vb)
                    for (uint64_t ex = 0; ex < phk_div_up(E, 256); ++ex)
                        folds.push_back(ChainGroupFold{v.in, o + vb * E, v.m, E, (uint32_t)ex, (uint32_t)vb});
                if (blocks > 1) v.in = o, v.m = blocks, next.push_back(v);
            }
            out.push_back({first, folds.size()});
            live.swap(next);
        }
    };
    levels(live_v, Ev, c->grp.levels_v);
    levels(live_t, Em, c->grp.levels_t);
    PHK_REQUIRE(tiles.size() < (1ull << 31) && etiles.size() < (1ull << 31) && folds.size() < (1ull << 31),
                "%s: more than 2^31 workgroups in one launch", who);
    c->grp.ntiles = tiles.size();
    if (c->grp.tiles.bytes < tiles.size() * sizeof(ChainGroupTile))
        PHK_TRY(c->grp.tiles.alloc(who, "descriptors", tiles.size() * sizeof(ChainGroupTile)));
    if (c->grp.etiles.bytes < etiles.size() * sizeof(ChainGroupTile))
        PHK_TRY(c->grp.etiles.alloc(who, "descriptors", etiles.size() * sizeof(ChainGroupTile)));
    if (c->grp.folds.bytes < folds.size() * sizeof(ChainGroupFold))
        PHK_TRY(c->grp.folds.alloc(who, "descriptors", folds.size() * sizeof(ChainGroupFold)));
    if (c->R) PHK_TRY(phk_copy_to_device(ctx, c->grp.rg.ptr, rg.data(), c->R * 4));
    if (!tiles.empty()) PHK_TRY(phk_copy_to_device(ctx, c->grp.tiles.ptr, tiles.data(), tiles.size() * sizeof(ChainGroupTile)));
    if (!etiles.empty()) PHK_TRY(phk_copy_to_device(ctx, c->grp.etiles.ptr, etiles.data(), etiles.size() * sizeof(ChainGroupTile)));
    if (!folds.empty()) PHK_TRY(phk_copy_to_device(ctx, c->grp.folds.ptr, folds.data(), folds.size() * sizeof(ChainGroupFold)));
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // the tables leave scope
    return PHK_OK;
}

extern "C" int phk_chain_set_grouped(phk_ctx *ctx, phk_chain *c, const double *log_profiles, uint64_t D, const double *trans,
                                     const double *init, const int64_t *qlog_trans, const int64_t *qlog_init, double temper,
                                     const uint8_t *active) {
    const char *who = "phk_chain_set_grouped";
    PHK_ENTER(ctx, "phk_chain_set_grouped");
    PHK_REQUIRE(c, "%s: NULL chain", who);
    PHK_REQUIRE(c->grp.G, "%s: the chain has no groups (phk_chain_set_groups)", who);
    PHK_REQUIRE(log_profiles && trans && init && qlog_trans && qlog_init, "%s: NULL parameters", who);
    PHK_REQUIRE(D == c->D, "%s: the profiles have %llu columns, the count rows %llu", who, (unsigned long long)D,
                (unsigned long long)c->D);
    PHK_REQUIRE(temper > 0.0 && temper - temper == 0.0, "%s: temper = %g is not finite and > 0", who, temper);
    const uint64_t G = c->grp.G, S = c->S, SS = S * S, PS = SS + S;
    for (uint64_t g = 0; g < G; ++g) {
        if (active && !active[g]) continue;
        PHK_TRY(chain_check_params(who, (long long)g, c->S, trans + g * SS, init + g * S, qlog_trans + g * SS,
                                   qlog_init + g * S));
    }
    for (uint64_t g = 0; g < G; ++g) {
        if (active && !active[g]) continue;
        if (!phk_rows_finite(log_profiles + g * S * D, S * D)) {
            phk_set_error("%s: group %llu: the log profiles hold a value that is not finite (a zero profile entry?)", who,
                          (unsigned long long)g);
            return PHK_ERR_NAN;
        }
    }
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    c->ready = false;
    // the groups at work: active and with a window; their parameters packed as the kernels read them (the others' stay
    // unread: zeros go up in their place)
    std::vector<uint8_t> work(G);
    std::vector<double> par(G * PS, 0.0), logp;
    std::vector<int64_t> qpar(G * PS, 0);
    bool all = true;
    for (uint64_t g = 0; g < G; ++g) {
        uint64_t w0, w1;
        chain_group_span(c, g, w0, w1);
        work[g] = (!active || active[g]) && w1 > w0;
        all = all && work[g];
        if (!work[g]) continue;
        std::copy(trans + g * SS, trans + (g + 1) * SS, par.begin() + g * PS);
        std::copy(init + g * S, init + (g + 1) * S, par.begin() + g * PS + SS);
        std::copy(qlog_trans + g * SS, qlog_trans + (g + 1) * SS, qpar.begin() + g * PS);
        std::copy(qlog_init + g * S, qlog_init + (g + 1) * S, qpar.begin() + g * PS + SS);
    }
    const double *lp = log_profiles;
    if (!all) {
        logp.assign(G * S * D, 0.0);
        for (uint64_t g = 0; g < G; ++g)
            if (work[g]) std::copy(log_profiles + g * S * D, log_profiles + (g + 1) * S * D, logp.begin() + g * S * D);
        lp = logp.data();
    }
    auto body = [&]() -> int {
        if (!c->grp.tables || work != c->grp.work) {
            c->grp.tables = false;
            c->grp.work = work;
            PHK_TRY(chain_group_tables(ctx, c));
            c->grp.tables = true;
        }
        PHK_TRY(phk_copy_to_device(ctx, c->grp.par.ptr, par.data(), G * PS * 8));
        PHK_TRY(phk_copy_to_device(ctx, c->grp.qpar.ptr, qpar.data(), G * PS * 8));
        PHK_TRY(phk_copy_to_device(ctx, c->grp.logp.ptr, lp, G * S * D * 8));
        if (c->grp.ntiles) {
            const dim3 grid((unsigned)c->grp.ntiles), blk(GT_WAVES * 64);
#define CH_GEMIT(FULL)                                                                                                        \
            PHK_LAUNCH(ctx, "phk_chain_group_emit_kernel",                                                                    \
                       phk_chain_group_emit_kernel<FULL><<<grid, blk, 0, ctx->stream>>>(                                      \
                           c->counts, c->grp.spans.as<ChainGroup>(), c->grp.tiles.as<ChainGroupTile>(),                       \
                           c->grp.logp.as<double>(), c->S, D, temper, c->E.as<double>(), c->M.as<double>()))
            CHAIN_BY_FLAG(D % GT_KC == 0, CH_GEMIT);
#undef CH_GEMIT
        }
        return PHK_OK;
    };
    int rc = body();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PHK_OK) {   // the packed parameters leave scope
        phk_set_error("%s: the stream failed", who);
        rc = PHK_ERR_HIP;
    }
    c->ready = rc == PHK_OK;
    return rc;
}

// backward then forward over the records of the groups at work
static int chain_group_forward_backward(phk_ctx *ctx, const phk_chain *c) {
    const double *E = c->E.as<double>(), *M = c->M.as<double>(), *par = c->grp.par.as<double>();
    const uint64_t *off = c->off.as<uint64_t>();
    const uint32_t *rg = c->grp.rg.as<uint32_t>();
#define CH_GFB(SP)                                                                                                            \
    {                                                                                                                         \
        const dim3 grid(chain_grid(c->R, 64 / SP, CH_BLOCKS_MAX));                                                            \
        PHK_LAUNCH(ctx, "phk_chain_group_backward_kernel", phk_chain_group_backward_kernel<SP><<<grid, dim3(64), 0, ctx->stream>>>( \
                                                               E, M, off, c->R, c->S, rg, par, c->Bt.as<double>()));          \
        PHK_LAUNCH(ctx, "phk_chain_group_forward_kernel",                                                                     \
                   phk_chain_group_forward_kernel<SP><<<grid, dim3(64), 0, ctx->stream>>>(                                    \
                       E, M, off, c->R, c->S, rg, par, c->Bt.as<double>(), c->G.as<double>(), c->V.as<double>()));            \
    }
    CHAIN_BY_SP(c->S, CH_GFB);
#undef CH_GFB
    return PHK_OK;
}

static int chain_group_viterbi(phk_ctx *ctx, const phk_chain *c) {
#define CH_GVIT(SP)                                                                                                           \
    PHK_LAUNCH(ctx, "phk_chain_group_viterbi_kernel",                                                                         \
               phk_chain_group_viterbi_kernel<SP><<<dim3(chain_grid(c->R, 64 / SP, CH_BLOCKS_MAX)), dim3(64), 0, ctx->stream>>>( \
                   c->E.as<double>(), c->M.as<double>(), c->off.as<uint64_t>(), c->R, c->S, c->grp.rg.as<uint32_t>(),         \
                   c->grp.qpar.as<int64_t>(), c->BP.as<uint8_t>(), c->score.as<int64_t>(), c->last.as<uint8_t>()))
    CHAIN_BY_SP(c->S, CH_GVIT);
#undef CH_GVIT
    return PHK_OK;
}

static int chain_group_fold(phk_ctx *ctx, const phk_chain *c, const std::vector<std::pair<uint64_t, uint64_t>> &levels) {
    for (const auto &lv : levels) {
        if (lv.second == lv.first) continue;
        PHK_LAUNCH(ctx, "phk_chain_group_fold_kernel",
                   phk_chain_group_fold_kernel<<<dim3((unsigned)(lv.second - lv.first)), dim3(256), 0, ctx->stream>>>(
                       c->grp.folds.as<ChainGroupFold>() + lv.first));
    }
    return PHK_OK;
}

// zeros over the windows (x: per window, `per` elements each) or records (per == 0: y, one element each) of the groups
// that are not at work
template <typename T>
static void chain_group_zero(const phk_chain *c, T *x, uint64_t per, T *y) {
    for (uint64_t g = 0; g < c->grp.G; ++g) {
        if (c->grp.work[g]) continue;
        uint64_t w0, w1;
        chain_group_span(c, g, w0, w1);
        if (x) std::fill(x + w0 * per, x + w1 * per, (T)0);
        if (y) std::fill(y + c->grp.off[g], y + c->grp.off[g + 1], (T)0);
    }
}

static int chain_group_expect_run(phk_ctx *ctx, const phk_chain *c, double *T, double *Ns, double *xi, double *gamma0,
                                  double *log_evidence, double *log_evidence_rec) {
    const uint64_t S = c->S, D = c->D, G = c->grp.G, SS = S * S, Ev = SS + S + 1, Em = S * D + S + 1;
    PHK_TRY(chain_group_forward_backward(ctx, c));
    PHK_TRY(chain_group_fold(ctx, c, c->grp.levels_v));
    for (const ChainGroups::Batch &b : c->grp.batches) {
        PHK_LAUNCH(ctx, "phk_chain_spread_kernel",
                   phk_chain_spread_kernel<<<dim3(chain_grid(b.nb * CH_KP, 256, 4096)), dim3(256), 0, ctx->stream>>>(
                       c->G.as<double>() + b.wa * S, b.nb, (uint32_t)S, c->Rx.as<double>()));
        const dim3 grid((unsigned)(b.d1 - b.d0)), blk(GT_WAVES * 64);
        const ChainGroupTile *tiles = c->grp.etiles.as<ChainGroupTile>() + b.d0;
#define CH_GEXPECT(VEC)                                                                                                       \
        PHK_LAUNCH(ctx, "phk_chain_group_expect_kernel",                                                                      \
                   phk_chain_group_expect_kernel<VEC><<<grid, blk, 0, ctx->stream>>>(                                         \
                       c->Rx.as<double>(), b.wa, c->counts, D, c->grp.spans.as<ChainGroup>(), tiles, c->M.as<double>(),       \
                       (uint32_t)S, Em, c->grp.part.as<double>()))
        CHAIN_BY_FLAG(D % 4 == 0, CH_GEXPECT);
#undef CH_GEXPECT
    }
    PHK_TRY(chain_group_fold(ctx, c, c->grp.levels_t));
    std::vector<double> v(G * Ev), t(G * Em);
    PHK_TRY(phk_copy_to_host(ctx, v.data(), c->grp.resV.ptr, G * Ev * 8));
    PHK_TRY(phk_copy_to_host(ctx, t.data(), c->grp.resT.ptr, G * Em * 8));
    for (uint64_t g = 0; g < G; ++g) {
        if (!c->grp.work[g]) {
            std::fill(xi + g * SS, xi + (g + 1) * SS, 0.0), std::fill(gamma0 + g * S, gamma0 + (g + 1) * S, 0.0);
            std::fill(T + g * S * D, T + (g + 1) * S * D, 0.0), std::fill(Ns + g * S, Ns + (g + 1) * S, 0.0);
            log_evidence[g] = 0.0;
            continue;
        }
        const double *pv = v.data() + g * Ev, *pt = t.data() + g * Em;
        std::copy(pv, pv + SS, xi + g * SS), std::copy(pv + SS, pv + SS + S, gamma0 + g * S);
        log_evidence[g] = pv[SS + S];
        std::copy(pt, pt + S * D, T + g * S * D), std::copy(pt + S * D, pt + S * D + S, Ns + g * S);
    }
    if (log_evidence_rec) {
        PHK_TRY(chain_record_evidence(ctx, c, log_evidence_rec));
        chain_group_zero<double>(c, nullptr, 0, log_evidence_rec);
    }
    return PHK_OK;
}

extern "C" int phk_chain_expect_grouped(phk_ctx *ctx, const phk_chain *c, double *T, double *Ns, double *xi, double *gamma0,
                                        double *log_evidence, double *log_evidence_rec) {
    const char *who = "phk_chain_expect_grouped";
    PHK_ENTER(ctx, "phk_chain_expect_grouped");
    PHK_REQUIRE(c, "%s: NULL chain", who);
    PHK_REQUIRE(c->grp.G, "%s: the chain has no groups (phk_chain_set_groups)", who);
    PHK_REQUIRE(c->ready, "%s: phk_chain_set_grouped has not succeeded on the chain", who);
    PHK_REQUIRE(T && Ns && xi && gamma0 && log_evidence, "%s: NULL pointer", who);
    const int rc = chain_group_expect_run(ctx, c, T, Ns, xi, gamma0, log_evidence, log_evidence_rec);
    if (rc != PHK_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}
