// dbscan_sweep.hip -- phk_dbscan_sweep: DBSCAN for every cell c = (eps_c, min_samples_c) of a grid of up to 64 cells on one
// resident copy of the rows X[n][D] (gfx950), the study behind a choice of learning.dbscan's two parameters
// (scripts/learning.py:149-163).  Every cell decides on the same distances: s_ij = pair_tile.h's direct-difference chain is
// computed once per pass and serves all cells.
//
// The distinct thresholds t_e (cluster.hip's cl_eps_threshold of each eps: s <= t_e  <=>  sqrt(s) <= eps) are sorted
// ascending, E <= 64 of them; bin(s) = the number of thresholds that s exceeds, so s is a neighbour distance exactly in the
// cells whose threshold index is >= bin(s) -- the bit set ge[bin(s)] -- and in no cell when bin(s) = E.
//   count   : per row a histogram of bin(s) over all columns (LDS integer adds, flushed by global integer atomic adds);
//             a prefix over the bins gives the neighbour count at every threshold and so coremask[i], bit c = row i is a
//             core point of cell c.  Integers: exact and order-free.
//   union   : the tiles (I, J), I <= J, of U = the rows that are core in some cell; a pair is an edge of the cells
//             coremask[i] & coremask[j] & ge[bin(s)], joined per cell on 128 LDS slots, then each slot with its LDS root in
//             parent[c][|U|] by agent-scope atomics (phk_cl_union_kernel's scheme, per cell); compression is its own launch.
//   border  : the rows that are not core in some cell against U: an int32 atomic min of the column's root into
//             best[c][row] for the cells ~coremask[i] & coremask[j] & ge[bin(s)].  The smallest root is the smallest label.
//   labels  : per cell the roots ranked in row order, on the host.
// Each of the three pair passes takes a limit on the pair tiles of one launch.
#include "cluster_shared.h"
#include "pair_tile.h"

#include <algorithm>
#include <cmath>

#define DS_MAX_CELLS 64
#define DS_SLOTS (2 * CL_T)   // LDS union-find slots of one cell

struct phk_dbscan_rows {
    uint64_t n = 0, D = 0;
    PhkDevMem x;   // the rows, free of NaN
};

// The thresholds, the cell sets ge[0 .. E] and the tile staging every pair pass keeps in LDS.
struct DsShared {
    double Qs[CL_KC][CL_T + CL_PAD], Cs[CL_KC][CL_T + CL_PAD];
    double th[DS_MAX_CELLS];
    uint64_t ge[DS_MAX_CELLS + 1];
};

__device__ __forceinline__ void ds_load_tables(DsShared &sh, const double *__restrict__ th, const uint64_t *__restrict__ ge, uint32_t E) {
    if (threadIdx.x < E) sh.th[threadIdx.x] = th[threadIdx.x];
    if (threadIdx.x <= E) sh.ge[threadIdx.x] = ge ? ge[threadIdx.x] : 0;
}

// the number of thresholds th[0] <= ... <= th[E - 1] that s exceeds (top = the largest power of two <= E).  A NaN s (rows
// with infinities) exceeds every threshold, as it fails phk_dbscan's s <= t.
__device__ __forceinline__ uint32_t ds_bin(const double *th, uint32_t E, uint32_t top, double s) {
    uint32_t lo = 0;
    for (uint32_t step = top; step; step >>= 1)
        if (lo + step <= E && !(s <= th[lo + step - 1])) lo += step;
    return lo;
}

// Count pass.  Workgroup (query block, column group g) walks the column tiles [g T / G, (g + 1) T / G) and keeps
// hist[query][bin] in LDS (row stride E | 1 words); the non-zero words go to cnt[n][E] by integer atomic adds.  Self counts.
__global__ __launch_bounds__(CL_THREADS) void phk_ds_count_kernel(const double *__restrict__ X, uint64_t n, uint64_t D,
                                                                  const double *__restrict__ th, uint32_t E, uint32_t top,
                                                                  uint64_t qb0, uint32_t groups, uint32_t *__restrict__ cnt) {
    __shared__ DsShared sh;
    __shared__ uint32_t hist[CL_T * (DS_MAX_CELLS + 1)];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint32_t stride = E | 1u;
    const uint64_t qbase = (qb0 + blockIdx.x) * CL_T;
    const uint64_t T = (n + CL_T - 1) / CL_T;
    const uint64_t j0 = T * blockIdx.y / groups, j1 = T * (blockIdx.y + 1) / groups;
    ds_load_tables(sh, th, nullptr, E);
    for (uint32_t w = threadIdx.x; w < CL_T * stride; w += CL_THREADS) hist[w] = 0;
    __syncthreads();
    const double tmax = sh.th[E - 1];
    for (uint64_t J = j0; J < j1; ++J) {
        double s[4][4];
        cl_tile({X, nullptr, n, qbase}, {X, nullptr, n, J * CL_T}, D, sh.Qs, sh.Cs, s);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (J * CL_T + tx + 16 * c < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (s[r][c] <= tmax) atomicAdd(&hist[(ty + 16 * r) * stride + ds_bin(sh.th, E, top, s[r][c])], 1u);
            }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < CL_T * E; w += CL_THREADS) {
        const uint32_t q = w / E, b = w - q * E;
        const uint32_t v = hist[q * stride + b];
        if (v && qbase + q < n) atomicAdd(&cnt[(qbase + q) * E + b], v);
    }
}

// One thread per row: the prefix over the row's bins, visited through the cells sorted by threshold index (order[k] = the
// k-th of them, cell_e / cell_ms = a cell's threshold index and min_samples): bit c of coremask[i] = the count at cell c's
// threshold is >= its min_samples.
__global__ __launch_bounds__(256) void phk_ds_coremask_kernel(const uint32_t *__restrict__ cnt, uint64_t n, uint32_t E, uint32_t C,
                                                             const uint8_t *__restrict__ order, const uint8_t *__restrict__ cell_e,
                                                             const uint32_t *__restrict__ cell_ms, uint64_t *__restrict__ coremask) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *row = cnt + i * E;
    uint64_t m = 0;
    uint32_t cum = 0, e = 0;
    for (uint32_t k = 0; k < C; ++k) {
        const uint32_t c = order[k];
        for (const uint32_t last = cell_e[c]; e <= last; ++e) cum += row[e];
        if (cum >= cell_ms[c]) m |= 1ull << c;
    }
    coremask[i] = m;
}

// Union pass.  Tile (I, J), I <= J, of the rows U[0 .. nu) (compact order = row order).  lp[c][128]: the tile's slots of
// cell c (slot r: compact row 64 I + r, slot 64 + j: compact row 64 J + j; the diagonal tile uses slots 0..63 for both).
// Afterwards every slot that is not its own LDS root is joined to that root in parent[c][nu]: at most 127 global unions per
// cell and tile.  A row that is not core in cell c takes part in no edge of c and stays its own root there.
__global__ __launch_bounds__(CL_THREADS) void phk_ds_union_kernel(const double *__restrict__ X, uint64_t D, const double *__restrict__ th,
                                                                  const uint64_t *__restrict__ ge, uint32_t E, uint32_t top, uint32_t C,
                                                                  const int32_t *__restrict__ U, const uint64_t *__restrict__ coremask,
                                                                  uint64_t nu, uint64_t ib0, int32_t *parent) {
    __shared__ DsShared sh;
    extern __shared__ int ds_lp[];   // [C][DS_SLOTS]
    const uint64_t I = ib0 + blockIdx.y, J = blockIdx.x;
    if (I > J) return;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const bool diag = I == J;
    ds_load_tables(sh, th, ge, E);
    for (uint32_t w = threadIdx.x; w < C * DS_SLOTS; w += CL_THREADS) ds_lp[w] = w & (DS_SLOTS - 1);
    uint64_t cmq[4], cmc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t a = I * CL_T + ty + 16 * r, b = J * CL_T + tx + 16 * r;
        cmq[r] = a < nu ? coremask[U[a]] : 0;
        cmc[r] = b < nu ? coremask[U[b]] : 0;
    }
    __syncthreads();
    const double tmax = sh.th[E - 1];
    double s[4][4];
    cl_tile({X, U, nu, I * CL_T}, {X, U, nu, J * CL_T}, D, sh.Qs, sh.Cs, s);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!(s[r][c] <= tmax)) continue;
            const int qi = ty + 16 * r, cj = tx + 16 * c;
            uint64_t mask = cmq[r] & cmc[c] & sh.ge[ds_bin(sh.th, E, top, s[r][c])];
            while (mask) {
                const int cell = __builtin_ctzll(mask);
                mask &= mask - 1;
                lf_union(ds_lp + cell * DS_SLOTS, qi, diag ? cj : CL_T + cj);
            }
        }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < C * DS_SLOTS; w += CL_THREADS) {
        const uint32_t cell = w / DS_SLOTS;
        const int x = w & (DS_SLOTS - 1);
        if (diag && x >= CL_T) continue;
        const int r = lf_find(ds_lp + cell * DS_SLOTS, x);
        if (r != x) {
            const uint64_t gx = x < CL_T ? I * CL_T + x : J * CL_T + (x - CL_T);
            const uint64_t gr = r < CL_T ? I * CL_T + r : J * CL_T + (r - CL_T);
            uf_union(parent + (uint64_t)cell * nu, (int32_t)gr, (int32_t)gx);
        }
    }
}

// Path compression, a launch of its own: root[c][m] = the root of compact row m in cell c (plain loads: the union pass has
// completed).  grid (rows, cells).
__global__ __launch_bounds__(256) void phk_ds_compress_kernel(const int32_t *__restrict__ parent, uint64_t nu, int32_t *__restrict__ root) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nu) return;
    const int32_t *p = parent + (uint64_t)blockIdx.y * nu;
    int32_t x = (int32_t)m;
    for (int32_t q = p[x]; q != x; q = p[x]) x = q;
    root[(uint64_t)blockIdx.y * nu + m] = x;
}

// Border pass.  Query rows B[0 .. nb) (not core in at least one cell) against U.  lb[query][C] in LDS takes the smallest root
// per cell (LDS integer min), flushed to best[c][nb] by global integer atomic min; INT32_MAX = no core neighbour (noise).
__global__ __launch_bounds__(CL_THREADS) void phk_ds_border_kernel(const double *__restrict__ X, uint64_t D, const double *__restrict__ th,
                                                                   const uint64_t *__restrict__ ge, uint32_t E, uint32_t top, uint32_t C,
                                                                   const int32_t *__restrict__ B, uint64_t nb,
                                                                   const int32_t *__restrict__ U, uint64_t nu,
                                                                   const uint64_t *__restrict__ coremask, const int32_t *__restrict__ root,
                                                                   uint64_t qb0, uint32_t groups, int32_t *__restrict__ best) {
    __shared__ DsShared sh;
    extern __shared__ int ds_lb[];   // [CL_T][C]
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t qbase = (qb0 + blockIdx.x) * CL_T;
    const uint64_t T = (nu + CL_T - 1) / CL_T;
    const uint64_t j0 = T * blockIdx.y / groups, j1 = T * (blockIdx.y + 1) / groups;
    ds_load_tables(sh, th, ge, E);
    for (uint32_t w = threadIdx.x; w < CL_T * C; w += CL_THREADS) ds_lb[w] = INT32_MAX;
    uint64_t ncq[4];   // the cells the query is NOT core in
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t q = qbase + ty + 16 * r;
        ncq[r] = q < nb ? ~coremask[B[q]] : 0;
    }
    __syncthreads();
    const double tmax = sh.th[E - 1];
    for (uint64_t J = j0; J < j1; ++J) {
        double s[4][4];
        cl_tile({X, B, nb, qbase}, {X, U, nu, J * CL_T}, D, sh.Qs, sh.Cs, s);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t m = J * CL_T + tx + 16 * c;
            if (m >= nu) continue;
            const uint64_t cm = coremask[U[m]];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!(s[r][c] <= tmax)) continue;
                uint64_t mask = ncq[r] & cm & sh.ge[ds_bin(sh.th, E, top, s[r][c])];
                while (mask) {
                    const int cell = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    atomicMin(&ds_lb[(ty + 16 * r) * C + cell], root[(uint64_t)cell * nu + m]);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < CL_T * C; w += CL_THREADS) {
        const uint32_t q = w / C, cell = w - q * C;
        const int v = ds_lb[w];
        if (v != INT32_MAX && qbase + q < nb) atomicMin(&best[(uint64_t)cell * nb + qbase + q], v);
    }
}

// p[i] = i % mod (mod > 0: the identity parent of every cell), else v
__global__ __launch_bounds__(256) void phk_ds_fill_kernel(int32_t *__restrict__ p, uint64_t count, int32_t v, uint64_t mod) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = mod ? (int32_t)(i % mod) : v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
extern "C" int phk_dbscan_sweep_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_dbscan_rows **out) {
    PHK_ENTER(ctx, "phk_dbscan_sweep_create");
    PHK_REQUIRE(out, "phk_dbscan_sweep_create: NULL pointer");
    PHK_REQUIRE(D >= 1 && n < (1ull << 31), "phk_dbscan_sweep_create: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)D);
    PHK_REQUIRE(X || n == 0, "phk_dbscan_sweep_create: NULL pointer");
    phk_dbscan_rows *h = new phk_dbscan_rows;
    h->n = n;
    h->D = D;
    if (n) {
        const uint64_t bytes = n * D * sizeof(double);
        int rc = h->x.alloc("phk_dbscan_sweep_create", "rows", bytes);
        if (rc == PHK_OK) rc = phk_copy_to_device(ctx, h->x.ptr, X, bytes);
        if (rc == PHK_OK) rc = cl_refuse_nan(ctx, "phk_dbscan_sweep_create", h->x.as<double>(), n * D);
        if (rc != PHK_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return PHK_OK;
}

extern "C" int phk_dbscan_sweep_destroy(phk_ctx *ctx, phk_dbscan_rows *rows) {
    PHK_ENTER(ctx, "phk_dbscan_sweep_destroy");
    if (!rows) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    delete rows;
    return PHK_OK;
}

extern "C" int phk_dbscan_sweep(phk_ctx *ctx, phk_dbscan_rows *rows, uint32_t C, const double *eps, const uint64_t *min_samples,
                                uint64_t tiles_per_launch, int32_t *labels, uint64_t *coremask, uint64_t *n_clusters,
                                uint32_t *launches) {
    PHK_ENTER(ctx, "phk_dbscan_sweep");
    PHK_REQUIRE(rows, "phk_dbscan_sweep: NULL rows");
    PHK_REQUIRE(C >= 1 && C <= DS_MAX_CELLS, "phk_dbscan_sweep: need 1 <= cells <= %d (got %u)", DS_MAX_CELLS, C);
    PHK_REQUIRE(eps && min_samples, "phk_dbscan_sweep: NULL pointer");
    for (uint32_t c = 0; c < C; ++c) {
        PHK_REQUIRE(eps[c] > 0.0 && eps[c] < __builtin_inf(), "phk_dbscan_sweep: eps must be finite and > 0 (cell %u: %g)", c, eps[c]);
        PHK_REQUIRE(min_samples[c] >= 1, "phk_dbscan_sweep: min_samples must be >= 1 (cell %u)", c);
    }
    const uint64_t n = rows->n, D = rows->D;
    const double *d_x = rows->x.as<double>();
    if (launches) launches[0] = launches[1] = launches[2] = 0;
    if (n == 0) {
        if (n_clusters) std::fill(n_clusters, n_clusters + C, 0ull);
        return PHK_OK;
    }
    PHK_REQUIRE(labels, "phk_dbscan_sweep: NULL pointer");
    // thresholds: the distinct ones ascending; a cell's threshold index; ge[b] = the cells whose index is >= b
    std::vector<double> tc(C), th;
    for (uint32_t c = 0; c < C; ++c) tc[c] = cl_eps_threshold(eps[c]);
    th = tc;
    std::sort(th.begin(), th.end());
    th.erase(std::unique(th.begin(), th.end()), th.end());
    const uint32_t E = (uint32_t)th.size();
    uint32_t top = 1;
    while (top * 2 <= E) top *= 2;
    std::vector<uint8_t> cell_e(C), order(C);
    std::vector<uint32_t> cell_ms(C);
    std::vector<uint64_t> ge(E + 1, 0);
    for (uint32_t c = 0; c < C; ++c) {
        cell_e[c] = (uint8_t)(std::lower_bound(th.begin(), th.end(), tc[c]) - th.begin());
        cell_ms[c] = (uint32_t)std::min<uint64_t>(min_samples[c], n + 1);   // (n + 1: more than any count)
        order[c] = (uint8_t)c;
        for (uint32_t b = 0; b <= cell_e[c]; ++b) ge[b] |= 1ull << c;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint8_t a, uint8_t b) { return cell_e[a] < cell_e[b]; });
    const uint64_t full = C == 64 ? ~0ull : (1ull << C) - 1;
    const uint64_t limit = tiles_per_launch ? std::min<uint64_t>(tiles_per_launch, CL_MAX_BLOCKS) : CL_MAX_BLOCKS;

    PhkLayout lay;
    const uint64_t o_th = lay.take(E * sizeof(double)), o_ge = lay.take((E + 1) * sizeof(uint64_t)), o_ce = lay.take(C),
                   o_or = lay.take(C), o_ms = lay.take(C * sizeof(uint32_t)), o_cnt = lay.take(n * E * sizeof(uint32_t)),
                   o_cm = lay.take(n * sizeof(uint64_t)), o_u = lay.take(n * sizeof(int32_t)), o_b = lay.take(n * sizeof(int32_t)),
                   o_par = lay.take(n * C * sizeof(int32_t)), o_root = lay.take(n * C * sizeof(int32_t)),
                   o_best = lay.take(n * C * sizeof(int32_t));
    void *ws;
    PHK_TRY(phk_ws(ctx, WS_WIDE, lay.bytes, &ws));
    char *wb = (char *)ws;
    const double *d_th = (const double *)(wb + o_th);
    const uint64_t *d_ge = (const uint64_t *)(wb + o_ge);
    uint32_t *d_cnt = (uint32_t *)(wb + o_cnt);
    uint64_t *d_cm = (uint64_t *)(wb + o_cm);
    int32_t *d_u = (int32_t *)(wb + o_u), *d_b = (int32_t *)(wb + o_b), *d_parent = (int32_t *)(wb + o_par),
            *d_root = (int32_t *)(wb + o_root), *d_best = (int32_t *)(wb + o_best);
    PHK_HIP(hipMemcpyAsync(wb + o_th, th.data(), E * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(wb + o_ge, ge.data(), (E + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(wb + o_ce, cell_e.data(), C, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(wb + o_or, order.data(), C, hipMemcpyHostToDevice, ctx->stream));
    PHK_HIP(hipMemcpyAsync(wb + o_ms, cell_ms.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));

    // count pass, core masks
    PHK_HIP(hipMemsetAsync(d_cnt, 0, n * E * sizeof(uint32_t), ctx->stream));
    const uint64_t T = phk_div_up(n, CL_T);
    {
        const uint32_t G = cl_groups(ctx, T, T);
        const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(CL_MAX_BLOCKS / G, limit / T));
        for (uint64_t b0 = 0; b0 < T; b0 += step) {
            PHK_LAUNCH(ctx, "phk_ds_count_kernel",
                       phk_ds_count_kernel<<<dim3((unsigned)std::min(step, T - b0), G), dim3(CL_THREADS), 0, ctx->stream>>>(
                           d_x, n, D, d_th, E, top, b0, G, d_cnt));
            if (launches) ++launches[0];
        }
    }
    PHK_LAUNCH(ctx, "phk_ds_coremask_kernel",
               phk_ds_coremask_kernel<<<dim3((unsigned)phk_div_up(n, 256)), dim3(256), 0, ctx->stream>>>(
                   d_cnt, n, E, C, (const uint8_t *)(wb + o_or), (const uint8_t *)(wb + o_ce), (const uint32_t *)(wb + o_ms), d_cm));
    std::vector<uint64_t> cm(n);
    PHK_TRY(phk_copy_to_host(ctx, cm.data(), d_cm, n * sizeof(uint64_t)));
    // U = core somewhere (the core set of the largest eps with the smallest min_samples holds every cell's); B = not core somewhere
    std::vector<int32_t> ui, bi;
    for (uint64_t i = 0; i < n; ++i) {
        if (cm[i]) ui.push_back((int32_t)i);
        if (cm[i] != full) bi.push_back((int32_t)i);
    }
    const uint64_t nu = ui.size(), nb = bi.size();
    std::vector<int32_t> root(nu * C), best(nb * C, INT32_MAX);
    if (nu) {
        PHK_HIP(hipMemcpyAsync(d_u, ui.data(), nu * 4, hipMemcpyHostToDevice, ctx->stream));
        PHK_LAUNCH(ctx, "phk_ds_fill_kernel",
                   phk_ds_fill_kernel<<<dim3((unsigned)phk_div_up(nu * C, 256)), dim3(256), 0, ctx->stream>>>(d_parent, nu * C, 0, nu));
        const uint64_t Tu = phk_div_up(nu, CL_T);
        const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(65535, limit / Tu));
        for (uint64_t i0 = 0; i0 < Tu; i0 += step) {
            PHK_LAUNCH(ctx, "phk_ds_union_kernel",
                       phk_ds_union_kernel<<<dim3((unsigned)Tu, (unsigned)std::min(step, Tu - i0)), dim3(CL_THREADS),
                                             C * DS_SLOTS * sizeof(int), ctx->stream>>>(d_x, D, d_th, d_ge, E, top, C, d_u, d_cm, nu,
                                                                                        i0, d_parent));
            if (launches) ++launches[1];
        }
        PHK_LAUNCH(ctx, "phk_ds_compress_kernel",
                   phk_ds_compress_kernel<<<dim3((unsigned)phk_div_up(nu, 256), C), dim3(256), 0, ctx->stream>>>(d_parent, nu, d_root));
        PHK_TRY(phk_copy_to_host(ctx, root.data(), d_root, nu * C * sizeof(int32_t)));
    }
    if (nu && nb) {
        PHK_HIP(hipMemcpyAsync(d_b, bi.data(), nb * 4, hipMemcpyHostToDevice, ctx->stream));
        PHK_LAUNCH(ctx, "phk_ds_fill_kernel",
                   phk_ds_fill_kernel<<<dim3((unsigned)phk_div_up(nb * C, 256)), dim3(256), 0, ctx->stream>>>(d_best, nb * C, INT32_MAX, 0));
        const uint64_t Tq = phk_div_up(nb, CL_T), Tu = phk_div_up(nu, CL_T);
        const uint32_t G = cl_groups(ctx, Tq, Tu);
        const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(CL_MAX_BLOCKS / G, limit / Tu));
        for (uint64_t b0 = 0; b0 < Tq; b0 += step) {
            PHK_LAUNCH(ctx, "phk_ds_border_kernel",
                       phk_ds_border_kernel<<<dim3((unsigned)std::min(step, Tq - b0), G), dim3(CL_THREADS), CL_T * C * sizeof(int),
                                              ctx->stream>>>(d_x, D, d_th, d_ge, E, top, C, d_b, nb, d_u, nu, d_cm, d_root, b0, G,
                                                             d_best));
            if (launches) ++launches[2];
        }
        PHK_TRY(phk_copy_to_host(ctx, best.data(), d_best, nb * C * sizeof(int32_t)));
    }
    // labels: per cell the roots (a component's smallest core row) ranked in row order -- scikit-learn's numbering; a border
    // row takes the label of the smallest root among its core neighbours
    std::vector<int32_t> clab(nu);
    for (uint32_t c = 0; c < C; ++c) {
        int32_t *lab = labels + (uint64_t)c * n;
        std::fill(lab, lab + n, -1);
        const int32_t *rc = root.data() + (uint64_t)c * nu;
        int32_t K = 0;
        for (uint64_t m = 0; m < nu; ++m) {
            if (!(cm[ui[m]] >> c & 1)) continue;
            clab[m] = rc[m] == (int32_t)m ? K++ : clab[rc[m]];
            lab[ui[m]] = clab[m];
        }
        const int32_t *bc = best.data() + (uint64_t)c * nb;
        for (uint64_t q = 0; q < nb; ++q)
            if (!(cm[bi[q]] >> c & 1) && bc[q] != INT32_MAX) lab[bi[q]] = clab[bc[q]];
        if (n_clusters) n_clusters[c] = (uint64_t)K;
    }
    if (coremask) std::copy(cm.begin(), cm.end(), coremask);
    return PHK_OK;
}
