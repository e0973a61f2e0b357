// combo_grid.hip -- the cross-validated k_neighbors x k_clusters grid of the knn, kmeans and combo scoring methods
// (phamers_amd/combo_grid.py): every row of X = vstack(positive, negative) scored by the model of the fold
// that holds it out, for every value of both lists, from rows that go up once.  gfx950.
//
// Resident (phk_combo_grid_create): X[M][D], a fold id and a class per row, the row lists of the 2 F train sets (class c less
// fold f, in row order) and of the F held-out sets, and the centroid bank.
//   phk_combo_grid_fit   : one k-means problem per (train set, k) on kmeans_batch.h's batched core, its rows read through
//                          KbFoldRows (the set's rows of X less the set's column mean, NumPy's, given by the caller); the
//                          problems of a chunk share their row count, so the chunks are cut by train-set size.  A problem's
//                          centroids -- the member rows of X as given, summed in row order per (cluster, column), divided by
//                          the count: NumPy's mean(axis=0) -- go into the bank at the caller's offset;
//   phk_combo_grid_score : the neighbour pass (pair_tile.h's tiles of all rows against all rows, a pair of one fold at +inf,
//                          written to device memory in blocks of `rows_per_pass` query rows; per query one wave then takes
//                          the first max(k_neighbors) columns in order of (chain value, row index) and keeps their classes as
//                          one 64-bit word, rank r at bit r), the centroid pass (per fold its held-out rows against the fold's
//                          bank; one tile never straddles two (class, value) segments, so its 64 columns fold to one integer
//                          atomic min of the chain's bit pattern per row), and the epilogue: the vote of every k_neighbors
//                          from a popcount of the word's low k bits, and phk_centroid_metric_kernel's expression per value.
// Bank layout: fold f owns rows [f Cb, (f + 1) Cb), Cb = 2 sum(k); inside, the positive class's segments for the values in
// the caller's order, then the negative class's.  Everything is float64 and order-deterministic (the only atomics are integer
// counts and minima), so a cell does not depend on the other values, on `chunk` or on `rows_per_pass`.
#include "kmeans_batch.h"
#include "pair_tile.h"

#include <numeric>

#define CG_DEFAULT_CHUNK 64
#define CG_PASS_BYTES (256ull << 20)   // the default block of the pair matrix
#define CG_MAX_ROWS (1ull << 22)       // column tiles of one launch row stay within CL_MAX_BLOCKS

struct phk_combo_grid {
    uint64_t M = 0, D = 0;
    uint32_t folds = 0;
    PhkDevMem x, fold, cls;              // X[M][D] (double), a fold id (uint32_t) and a class (uint8_t) per row
    PhkDevMem idx;                       // int32_t: the train lists of set 0 .. 2 F - 1 (set = slot * F + fold; slot 0 = positive), then
    PhkDevMem held;                      // the held-out lists of fold 0 .. F - 1: held_off[f] .. held_off[f + 1] in idx (uint64_t here)
    std::vector<uint64_t> set_off;       // [2 F + 1] into idx
    std::vector<uint64_t> held_off;      // [F + 1] into idx
    PhkDevMem bank;                      // double [bank_rows][D]
    uint64_t bank_rows = 0;
    PhkDevMem ws;                        // the k-means chunks' workspace
    PhkDevMem ps;                        // the scoring passes' workspace
};

struct CgTile {               // a column tile of the centroid pass: columns [begin, end) of a fold's bank, all of segment seg
    uint32_t begin, end, seg, pad;
};

// ---- fold k-means: the centroids --------------------------------------------------------------------------------------
// One workgroup per (cluster, problem): bank row boff[b] + c = the mean of the member rows of X as given, summed in row
// order per column and divided by the count (np.mean(train[labels == c], axis=0) for D >= 2).  A cluster without members
// sets the problem's flag.
__global__ __launch_bounds__(256) void cg_centroid_kernel(KbView v, const double *__restrict__ X, const int32_t *__restrict__ idx,
                                                          const uint64_t *__restrict__ ioff, const uint64_t *__restrict__ boff,
                                                          double *__restrict__ bank, uint32_t *__restrict__ empty) {
    const uint32_t c = blockIdx.x, b = blockIdx.y;
    if (c >= v.st[b].k) return;
    const uint32_t *labels = v.labels + (uint64_t)b * v.n;
    const int32_t *list = idx + ioff[b];
    double *out = bank + (boff[b] + c) * v.D;
    uint32_t cnt = 0;
    for (uint64_t d = threadIdx.x; d < v.D; d += 256) {
        double s = 0.0;
        uint32_t m = 0;
        for (uint64_t i = 0; i < v.n; ++i)
            if (labels[i] == c) { s += X[(uint64_t)list[i] * v.D + d]; ++m; }
        out[d] = m ? s / (double)m : 0.0;
        cnt = m;
    }
    if (threadIdx.x == 0 && cnt == 0) atomicOr(&empty[b], 1u);
}

// ---- the neighbour pass -------------------------------------------------------------------------------------------------
// out[i - q0][j] = the CL_SQDIFF chain of rows i and j of X, +inf when both are held out by the same fold (the row itself
// included).  grid (column tiles, query tiles of the launch); q0 = the launch's first query row, a multiple of CL_T.
__global__ __launch_bounds__(CL_THREADS) void cg_pair_kernel(const double *__restrict__ X, uint64_t M, uint64_t D,
                                                             const uint32_t *__restrict__ fold, uint64_t q0,
                                                             double *__restrict__ out) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t qbase = q0 + (uint64_t)blockIdx.y * CL_T, cbase = (uint64_t)blockIdx.x * CL_T;
    double s[4][4];
    cl_tile({X, nullptr, M, qbase}, {X, nullptr, M, cbase}, D, Qs, Cs, s);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t i = qbase + ty + 16 * r;
        if (i >= M) continue;
        const uint32_t fi = fold[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t j = cbase + tx + 16 * c;
            if (j < M) out[(i - q0) * M + j] = fold[j] == fi ? __builtin_inf() : s[r][c];
        }
    }
}

// One wave per query of the block: phk_knn_vote_kernel's selection -- the next column in order of (value, index), kmax
// times -- with the class of the r-th neighbour kept at bit r of the query's word.
__global__ __launch_bounds__(256) void cg_select_kernel(const double *__restrict__ dist, uint64_t nq, uint64_t M,
                                                        const uint8_t *__restrict__ cls, int kmax, uint64_t *__restrict__ words) {
    const int lane = threadIdx.x & 63;
    const uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (q >= nq) return;
    const double *row = dist + q * M;
    double last_d = -1.0;
    uint64_t last_i = 0, word = 0;
    bool first = true;
    for (int r = 0; r < kmax; ++r) {
        double bd = __builtin_inf();
        uint64_t bi = ~0ull;
        for (uint64_t j = lane; j < M; j += 64) {
            const double d = row[j];
            const bool after = first || d > last_d || (d == last_d && j > last_i);
            if (after && (d < bd || (d == bd && j < bi))) {
                bd = d;
                bi = j;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const double od = __shfl_xor(bd, s);
            const uint64_t oi = __shfl_xor(bi, s);
            if (od < bd || (od == bd && oi < bi)) {
                bd = od;
                bi = oi;
            }
        }
        last_d = bd;
        last_i = bi;
        first = false;
        if (bi < M && cls[bi]) word |= 1ull << r;
    }
    if (lane == 0) words[q] = word;
}

// ---- the centroid pass --------------------------------------------------------------------------------------------------
// grid (query tiles of the launch, column tiles, folds).  Fold f's held-out rows against column tile t of its bank; the tile's
// minimum per query row goes to minb[row][seg] as an integer minimum of the bit pattern (the chains are non-negative doubles).
__global__ __launch_bounds__(CL_THREADS) void cg_centroid_pass_kernel(const double *__restrict__ X, uint64_t D,
                                                                      const int32_t *__restrict__ idx,
                                                                      const uint64_t *__restrict__ held_off,
                                                                      const double *__restrict__ bank, uint64_t Cb,
                                                                      const CgTile *__restrict__ tiles, uint32_t nseg, uint64_t xtile0,
                                                                      unsigned long long *__restrict__ minb) {
    __shared__ double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    const uint32_t f = blockIdx.z;
    const uint64_t h0 = held_off[f], cnt = held_off[f + 1] - h0;
    const uint64_t qbase = (xtile0 + blockIdx.x) * CL_T;
    if (qbase >= cnt) return;
    const CgTile t = tiles[blockIdx.y];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int32_t *held = idx + h0;
    double s[4][4];
    cl_tile({X, held, cnt, qbase}, {bank + (uint64_t)f * Cb * D, nullptr, t.end, t.begin}, D, Qs, Cs, s);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double m = __builtin_inf();
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (t.begin + tx + 16 * c < t.end) m = s[r][c] < m ? s[r][c] : m;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const double other = __shfl_xor(m, o);
            m = other < m ? other : m;
        }
        const uint64_t q = qbase + ty + 16 * r;
        if (tx == 0 && q < cnt)
            atomicMin(&minb[(uint64_t)held[q] * nseg + t.seg], (unsigned long long)__double_as_longlong(m));
    }
}

__global__ __launch_bounds__(256) void cg_fill_kernel(unsigned long long *__restrict__ p, uint64_t n, unsigned long long v) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- the epilogue -------------------------------------------------------------------------------------------------------
// One thread per row: knn[i][row] = phk_knn_vote_kernel's vote among the first kn[i] neighbours, km[j][row] =
// phk_centroid_metric_kernel's metric of the smallest chains to the positive (segment j) and negative (segment Ku + j)
// centroids of value j.
__global__ __launch_bounds__(256) void cg_epilogue_kernel(const uint64_t *__restrict__ words, const unsigned long long *__restrict__ minb,
                                                          uint64_t M, uint32_t Kn, const uint32_t *__restrict__ kn, uint32_t Ku,
                                                          double *__restrict__ knn, double *__restrict__ km) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= M) return;
    if (Kn) {
        const uint64_t word = words[q];
        for (uint32_t i = 0; i < Kn; ++i) {
            const int k = (int)kn[i];
            const int votes = __popcll(k >= 64 ? word : word & ((1ull << k) - 1ull));
            knn[(uint64_t)i * M + q] = (2 * votes > k) ? 1.0 : -1.0;
        }
    }
    for (uint32_t j = 0; j < Ku; ++j) {
        const double bp = __longlong_as_double((long long)minb[q * 2 * Ku + j]);
        const double bn = __longlong_as_double((long long)minb[q * 2 * Ku + Ku + j]);
        const double ep = sqrt(bp), en = sqrt(bn);
        km[(uint64_t)j * M + q] = tanh((en - ep) / (ep + en));
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
extern "C" int phk_combo_grid_create(phk_ctx *ctx, const double *X, uint64_t M, uint64_t D, const uint32_t *fold_of,
                                     const uint8_t *is_positive, uint32_t folds, phk_combo_grid **out) {
    PHK_ENTER(ctx, "phk_combo_grid_create");
    PHK_REQUIRE(X && fold_of && is_positive && out, "phk_combo_grid_create: NULL pointer");
    PHK_REQUIRE(M >= 1 && D >= 1 && M <= CG_MAX_ROWS, "phk_combo_grid_create: bad shape (%llu x %llu; at most %llu rows)",
                (unsigned long long)M, (unsigned long long)D, (unsigned long long)CG_MAX_ROWS);
    PHK_REQUIRE(folds >= 2 && folds <= 65535, "phk_combo_grid_create: folds must be 2..65535 (got %u)", folds);
    for (uint64_t i = 0; i < M; ++i)
        PHK_REQUIRE(fold_of[i] < folds, "phk_combo_grid_create: fold %u of row %llu is not below folds = %u", fold_of[i],
                    (unsigned long long)i, folds);
    if (!phk_rows_finite(X, M * D)) {
        phk_set_error("phk_combo_grid_create: the rows contain NaN or infinity");
        return PHK_ERR_NAN;
    }
    const uint32_t F = folds;
    phk_combo_grid *g = new phk_combo_grid;
    g->M = M;
    g->D = D;
    g->folds = F;
    // the lists: set (slot, f) = the rows of the slot's class outside fold f, in row order; then fold f's rows, in row order
    std::vector<int32_t> idx;
    idx.reserve((uint64_t)F * M);
    g->set_off.assign(2 * (uint64_t)F + 1, 0);
    g->held_off.assign((uint64_t)F + 1, 0);
    for (uint32_t slot = 0; slot < 2; ++slot)
        for (uint32_t f = 0; f < F; ++f) {
            for (uint64_t i = 0; i < M; ++i)
                if ((is_positive[i] != 0) == (slot == 0) && fold_of[i] != f) idx.push_back((int32_t)i);
            g->set_off[(uint64_t)slot * F + f + 1] = idx.size();
        }
    g->held_off[0] = idx.size();
    for (uint32_t f = 0; f < F; ++f) {
        for (uint64_t i = 0; i < M; ++i)
            if (fold_of[i] == f) idx.push_back((int32_t)i);
        g->held_off[f + 1] = idx.size();
    }
    int rc = PHK_OK;
    auto put = [&](PhkDevMem &m, const char *what, const void *src, uint64_t bytes) {
        if (rc == PHK_OK) rc = m.alloc("phk_combo_grid_create", what, bytes);
        if (rc == PHK_OK) rc = phk_copy_to_device(ctx, m.ptr, src, bytes);
    };
    put(g->x, "rows", X, M * D * 8);
    put(g->fold, "fold ids", fold_of, M * 4);
    put(g->cls, "classes", is_positive, M);
    put(g->idx, "row lists", idx.data(), idx.size() * 4);
    put(g->held, "row lists", g->held_off.data(), ((uint64_t)F + 1) * 8);
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PHK_ERR_HIP;
    if (rc != PHK_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return PHK_OK;
}

extern "C" int phk_combo_grid_destroy(phk_ctx *ctx, phk_combo_grid *g) {
    PHK_ENTER(ctx, "phk_combo_grid_destroy");
    if (!g) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    delete g;
    return PHK_OK;
}

extern "C" int phk_combo_grid_fit(phk_ctx *ctx, phk_combo_grid *g, uint64_t S, const uint32_t *set, const uint32_t *ks,
                                  const uint32_t *first_seed, const double *draws, const uint64_t *draw_off, const double *set_mean,
                                  const double *set_tol, int max_iter, uint32_t chunk, uint64_t bank_rows, const uint64_t *bank_off,
                                  uint32_t *status, int32_t *n_iter, double *min_gap, double *seed_margin) {
    PHK_ENTER(ctx, "phk_combo_grid_fit");
    PHK_REQUIRE(g, "phk_combo_grid_fit: NULL grid");
    const uint64_t D = g->D, nsets = 2 * (uint64_t)g->folds;
    PHK_TRY(kb_check_call("phk_combo_grid_fit", max_iter, chunk));
    PHK_REQUIRE(bank_rows >= 1 && bank_rows < (1ull << 31), "phk_combo_grid_fit: bad bank_rows");
    PHK_REQUIRE(S == 0 || (set && ks && first_seed && draw_off && set_mean && set_tol && bank_off && status && n_iter && min_gap &&
                           seed_margin),
                "phk_combo_grid_fit: NULL pointer");
    auto size_of = [&](uint64_t s) { return g->set_off[set[s] + 1] - g->set_off[set[s]]; };
    uint64_t n_max = 0;
    for (uint64_t s = 0; s < S; ++s) {
        PHK_REQUIRE(set[s] < nsets, "phk_combo_grid_fit: problem %llu names train set %u of %llu", (unsigned long long)s, set[s],
                    (unsigned long long)nsets);
        PHK_TRY(kb_check_problem("phk_combo_grid_fit", s, ks[s], size_of(s), first_seed[s], draws));
        PHK_REQUIRE(bank_off[s] + ks[s] <= bank_rows, "phk_combo_grid_fit: the centroids of problem %llu do not fit the bank",
                    (unsigned long long)s);
        PHK_REQUIRE(set_tol[set[s]] >= 0.0, "phk_combo_grid_fit: bad tolerance of train set %u", set[s]);
        n_max = std::max(n_max, size_of(s));
    }
    if (g->bank_rows != bank_rows) {
        PHK_HIP(hipStreamSynchronize(ctx->stream));
        g->bank_rows = 0;
        PHK_TRY(g->bank.alloc("phk_combo_grid_fit", "centroids", bank_rows * D * 8));
        g->bank_rows = bank_rows;
        PHK_HIP(hipMemsetAsync(g->bank.ptr, 0, bank_rows * D * 8, ctx->stream));
    }
    if (S == 0) return PHK_OK;
    // chunks: the problems in order of their train set's size (stable), cut where the size changes and after Sc problems
    const uint64_t Sc = std::min<uint64_t>(S, chunk ? chunk : CG_DEFAULT_CHUNK);
    std::vector<uint64_t> order(S);
    std::iota(order.begin(), order.end(), 0ull);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return size_of(a) < size_of(b); });
    std::vector<uint64_t> cut(1, 0);
    for (uint64_t p = 1; p <= S; ++p)
        if (p == S || p - cut.back() == Sc || size_of(order[p]) != size_of(order[cut.back()])) cut.push_back(p);
    // the chunk's workspace: the core's regions for the largest train set, then what KbFoldRows and the centroids read
    PhkLayout ws;
    const KbSpace core(ws, kb_extent(ks, order.data(), cut, n_max, D));
    const uint64_t o_mean = ws.take(nsets * D * 8), o_ioff = ws.take(Sc * 8), o_moff = ws.take(Sc * 8), o_boff = ws.take(Sc * 8),
                   o_empty = ws.take(Sc * 4);
    PHK_TRY(g->ws.grow(ctx, "phk_combo_grid_fit", ws.bytes, Sc));
    char *w = g->ws.as<char>();
    uint32_t *d_act, *d_empty = (uint32_t *)(w + o_empty);
    KbView v = core.bind(w, &d_act);
    const double *d_x = g->x.as<double>();
    const int32_t *d_idx = g->idx.as<int32_t>();
    const KbFoldRows rows = {d_x, d_idx, (const uint64_t *)(w + o_ioff), (const double *)(w + o_mean), (const uint64_t *)(w + o_moff)};
    const KbNames names = {"cg_seed_dist_kernel", "cg_seed_choose_kernel", "cg_assign_kernel", "cg_update_kernel", "cg_stop_kernel"};
    PHK_HIP(hipMemcpyAsync(w + o_mean, set_mean, nsets * D * 8, hipMemcpyHostToDevice, ctx->stream));

    KbChunk ch;
    std::vector<uint64_t> ioff(Sc), moff(Sc), boff(Sc);
    std::vector<uint32_t> empty(Sc);
    for (uint64_t c = 0; c + 1 < cut.size(); ++c) {
        const uint64_t p0 = cut[c], nb = cut[c + 1] - p0;
        v.n = size_of(order[p0]);
        ch.clear();
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t s = order[p0 + b];
            PHK_TRY(ch.add(ctx, v, ks[s], first_seed[s], draws ? draws + draw_off[s] : nullptr, set_tol[set[s]]));
            ioff[b] = g->set_off[set[s]];
            moff[b] = (uint64_t)set[s] * D;
            boff[b] = bank_off[s];
        }
        PHK_HIP(hipMemcpyAsync(w + o_ioff, ioff.data(), nb * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(w + o_moff, moff.data(), nb * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(w + o_boff, boff.data(), nb * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemsetAsync(d_empty, 0, nb * 4, ctx->stream));
        PHK_TRY(ch.upload(ctx, v));
        PHK_TRY(kb_solve_chunk(ctx, v, rows, ch, max_iter, d_act, names));
        PHK_LAUNCH(ctx, "cg_centroid_kernel",
                   cg_centroid_kernel<<<dim3(ch.kmax, (unsigned)nb), dim3(256), 0, ctx->stream>>>(
                       v, d_x, d_idx, (const uint64_t *)(w + o_ioff), (const uint64_t *)(w + o_boff), g->bank.as<double>(), d_empty));
        PHK_HIP(hipMemcpyAsync(empty.data(), d_empty, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_TRY(ch.download(ctx, v));   // (the host vectors above are reused by the next chunk)
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t s = order[p0 + b];
            status[s] = (ch.met_empty(b) || empty[b]) ? PHK_COMBO_GRID_EMPTY : 0u;
            n_iter[s] = ch.n_iter(b);
            seed_margin[s] = ch.seed_margin(b);
            min_gap[s] = ch.min_gap(b);
        }
    }
    return PHK_OK;
}

extern "C" int phk_combo_grid_get_centroids(phk_ctx *ctx, phk_combo_grid *g, uint64_t row0, uint64_t rows, double *out) {
    PHK_ENTER(ctx, "phk_combo_grid_get_centroids");
    PHK_REQUIRE(g && (out || rows == 0), "phk_combo_grid_get_centroids: NULL pointer");
    PHK_REQUIRE(row0 + rows <= g->bank_rows, "phk_combo_grid_get_centroids: rows %llu..%llu are not in the bank (%llu rows)",
                (unsigned long long)row0, (unsigned long long)(row0 + rows), (unsigned long long)g->bank_rows);
    if (rows == 0) return PHK_OK;
    return phk_copy_to_host(ctx, out, g->bank.as<double>() + row0 * g->D, rows * g->D * 8);
}

extern "C" int phk_combo_grid_put_centroids(phk_ctx *ctx, phk_combo_grid *g, uint64_t row0, uint64_t rows, const double *in) {
    PHK_ENTER(ctx, "phk_combo_grid_put_centroids");
    PHK_REQUIRE(g && (in || rows == 0), "phk_combo_grid_put_centroids: NULL pointer");
    PHK_REQUIRE(row0 + rows <= g->bank_rows, "phk_combo_grid_put_centroids: rows %llu..%llu are not in the bank (%llu rows)",
                (unsigned long long)row0, (unsigned long long)(row0 + rows), (unsigned long long)g->bank_rows);
    if (rows == 0) return PHK_OK;
    PHK_TRY(phk_copy_to_device(ctx, g->bank.as<double>() + row0 * g->D, in, rows * g->D * 8));
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // (the caller's rows may go away)
    return PHK_OK;
}

extern "C" int phk_combo_grid_score(phk_ctx *ctx, phk_combo_grid *g, uint32_t Kn, const uint32_t *kn, uint32_t Ku, const uint32_t *ku,
                                    uint64_t rows_per_pass, double *knn_out, double *km_out) {
    PHK_ENTER(ctx, "phk_combo_grid_score");
    PHK_REQUIRE(g, "phk_combo_grid_score: NULL grid");
    PHK_REQUIRE(Kn || Ku, "phk_combo_grid_score: no k_neighbors and no k_clusters value");
    PHK_REQUIRE((!Kn || (kn && knn_out)) && (!Ku || (ku && km_out)), "phk_combo_grid_score: NULL pointer");
    const uint64_t M = g->M, D = g->D;
    const uint32_t F = g->folds;
    uint64_t held_max = 0;
    for (uint32_t f = 0; f < F; ++f) held_max = std::max(held_max, g->held_off[f + 1] - g->held_off[f]);
    uint32_t kmax = 0;
    for (uint32_t i = 0; i < Kn; ++i) {
        PHK_REQUIRE(kn[i] >= 1 && kn[i] <= 64 && kn[i] <= M - held_max,
                    "phk_combo_grid_score: k_neighbors=%u out of range (1..min(64, smallest train set = %llu))", kn[i],
                    (unsigned long long)(M - held_max));
        kmax = std::max(kmax, kn[i]);
    }
    uint64_t Ksum = 0;
    for (uint32_t j = 0; j < Ku; ++j) {
        PHK_REQUIRE(ku[j] >= 1, "phk_combo_grid_score: k_clusters must be >= 1");
        Ksum += ku[j];
    }
    const uint64_t Cb = 2 * Ksum;
    PHK_REQUIRE(!Ku || (g->bank.ptr && g->bank_rows == (uint64_t)F * Cb),
                "phk_combo_grid_score: the bank holds %llu rows, these values need %llu", (unsigned long long)g->bank_rows,
                (unsigned long long)((uint64_t)F * Cb));
    // query rows per launch of the two pair passes: whole tiles, the pair matrix's block within CG_PASS_BYTES by default
    const uint64_t Mt = phk_div_up(M, CL_T) * CL_T;
    uint64_t R = rows_per_pass ? phk_div_up(rows_per_pass, CL_T) * CL_T : std::max<uint64_t>(CL_T, CG_PASS_BYTES / (M * 8) / CL_T * CL_T);
    R = std::min(R, Mt);
    const uint64_t coltiles = Mt / CL_T;
    R = std::min<uint64_t>(R, std::max<uint64_t>(1, std::min<uint64_t>(65535, CL_MAX_BLOCKS / coltiles)) * CL_T);
    // the centroid pass's column tiles
    std::vector<CgTile> tiles;
    {
        uint32_t at = 0;
        for (uint32_t slot = 0; slot < 2; ++slot)
            for (uint32_t j = 0; j < Ku; ++j) {
                for (uint32_t b = 0; b < ku[j]; b += CL_T)
                    tiles.push_back({at + b, at + ku[j], slot * Ku + j, 0u});
                at += ku[j];
            }
    }
    PHK_REQUIRE(tiles.size() <= 65535 && tiles.size() * F <= CL_MAX_BLOCKS,
                "phk_combo_grid_score: %llu column tiles of centroids x %u folds do not fit one launch", (unsigned long long)tiles.size(), F);
    PhkLayout ps;
    const uint64_t o_dist = ps.take(Kn ? R * M * 8 : 0), o_word = ps.take(Kn ? M * 8 : 0), o_kn = ps.take(Kn * 4ull),
                   o_min = ps.take(M * 2 * Ku * 8), o_tile = ps.take(tiles.size() * sizeof(CgTile)), o_knn = ps.take((uint64_t)Kn * M * 8),
                   o_km = ps.take((uint64_t)Ku * M * 8);
    PHK_TRY(g->ps.grow(ctx, "phk_combo_grid_score", ps.bytes, Kn + Ku));
    char *w = g->ps.as<char>();
    double *d_dist = (double *)(w + o_dist), *d_knn = (double *)(w + o_knn), *d_km = (double *)(w + o_km);
    uint64_t *d_word = (uint64_t *)(w + o_word);
    unsigned long long *d_min = (unsigned long long *)(w + o_min);
    if (Kn) {
        PHK_HIP(hipMemcpyAsync(w + o_kn, kn, Kn * 4ull, hipMemcpyHostToDevice, ctx->stream));
        for (uint64_t q0 = 0; q0 < M; q0 += R) {
            const uint64_t nq = std::min(R, M - q0);
            PHK_LAUNCH(ctx, "cg_pair_kernel",
                       cg_pair_kernel<<<dim3((unsigned)coltiles, (unsigned)phk_div_up(nq, CL_T)), dim3(CL_THREADS), 0, ctx->stream>>>(
                           g->x.as<double>(), M, D, g->fold.as<uint32_t>(), q0, d_dist));
            PHK_LAUNCH(ctx, "cg_select_kernel",
                       cg_select_kernel<<<dim3((unsigned)phk_div_up(nq, 4)), dim3(256), 0, ctx->stream>>>(
                           d_dist, nq, M, g->cls.as<uint8_t>(), (int)kmax, d_word + q0));
        }
    }
    if (Ku) {
        const double inf = __builtin_inf();
        unsigned long long infbits;
        memcpy(&infbits, &inf, 8);
        PHK_HIP(hipMemcpyAsync(w + o_tile, tiles.data(), tiles.size() * sizeof(CgTile), hipMemcpyHostToDevice, ctx->stream));
        PHK_LAUNCH(ctx, "cg_fill_kernel",
                   cg_fill_kernel<<<dim3((unsigned)phk_div_up(M * 2 * Ku, 256)), dim3(256), 0, ctx->stream>>>(d_min, M * 2 * Ku, infbits));
        const uint64_t qtiles = phk_div_up(held_max, CL_T);
        uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(R / CL_T, CL_MAX_BLOCKS / (tiles.size() * F)));
        for (uint64_t x0 = 0; x0 < qtiles; x0 += step)
            PHK_LAUNCH(ctx, "cg_centroid_pass_kernel",
                       cg_centroid_pass_kernel<<<dim3((unsigned)std::min(step, qtiles - x0), (unsigned)tiles.size(), F), dim3(CL_THREADS), 0,
                                                 ctx->stream>>>(g->x.as<double>(), D, g->idx.as<int32_t>(), g->held.as<uint64_t>(),
                                                                g->bank.as<double>(), Cb, (const CgTile *)(w + o_tile), 2 * Ku, x0,
                                                                d_min));
    }
    PHK_LAUNCH(ctx, "cg_epilogue_kernel",
               cg_epilogue_kernel<<<dim3((unsigned)phk_div_up(M, 256)), dim3(256), 0, ctx->stream>>>(
                   d_word, d_min, M, Kn, (const uint32_t *)(w + o_kn), Ku, d_knn, d_km));
    if (Kn) PHK_TRY(phk_copy_to_host(ctx, knn_out, d_knn, (uint64_t)Kn * M * 8));
    if (Ku) PHK_TRY(phk_copy_to_host(ctx, km_out, d_km, (uint64_t)Ku * M * 8));
    return PHK_OK;
}
