// placement.hip -- batched per-contig k-means placement (scripts/analysis.py:754-792: for every candidate contig, k-means
// on the reference phage rows plus the contig's row, then the silhouettes of the contig's cluster).  gfx950.
//
// The reference rows X[n][D] are resident (phk_placement_create); phk_placement_run solves, for B contig rows Z[B][D], the B
// independent problems "rows 0..n-1 = X, row n = Z[b]" in chunks of problems, every stage one launch for the whole chunk:
//   centring : mean_b = (S + Z[b]) / (n + 1) with S the row-order column sum of X (NumPy's column mean of the appended
//              matrix, bit for bit); the kernels subtract it on the fly, x - mean_b: the very subtraction the host path does;
//   seeding, Lloyd : kmeans_batch.h's batched k-means (shared with sweep.hip) on the rows "reference rows, then Z[b]", every
//              problem with the same k, first row and draws; labels, sweep counts and min_gap equal the single-problem
//              path's bit for bit;
//   cluster silhouettes : for the members of the contig's cluster only, sums in an order fixed by the labels alone.
// Everything is float64 and order-deterministic (the only atomics are integer counts and minima), so a problem's result
// does not depend on its place in the batch, on the chunking or on the run.
#include "kmeans_batch.h"

#define PL_SIL_GROUPS 16      // workgroups per problem of the silhouette kernel (members are dealt round robin)
#define PL_DEFAULT_CHUNK 256

struct phk_placement {
    uint64_t n = 0, D = 0;
    PhkDevMem x;                 // the reference rows
    std::vector<double> S, SS;   // column sums of x and x^2 in row order
    PhkDevMem ws;                // the chunks' workspace
};

__device__ __forceinline__ const double *pl_row(const double *__restrict__ X, const double *__restrict__ z, uint64_t n, uint64_t D,
                                                uint64_t i) {
    return i < n ? X + i * D : z;
}

// what the placement's own kernels read and write, per problem of the chunk
struct PlView {
    const double *X;        // [n][D]
    const double *Z;        // [Bc][D]
    const uint32_t *labels; // [Bc][n1], the k-means' result
    uint32_t *dup;          // [Bc] the contig's row equals a reference row
    uint32_t *n_members;    // [Bc]
    uint32_t *members;      // [Bc][n1]
    double *sdist;          // [Bc][PL_SIL_GROUPS][n1]
    double *ssum;           // [Bc][PL_SIL_GROUPS][k]
    uint32_t *ssize;        // [Bc][PL_SIL_GROUPS][k]
    double *sil;            // [Bc][n1]
    uint64_t n, n1, D;
    uint32_t k;
};

// ---- set-up: whether the contig's row equals a reference row ---------------------------------------------------------
// one wave per (reference row, problem): an exact duplicate of the contig's row
__global__ __launch_bounds__(256) void pl_dup_kernel(PlView v) {
    const int lane = threadIdx.x & 63;
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t b = blockIdx.y;
    if (i >= v.n) return;
    const double *x = v.X + i * v.D, *z = v.Z + (uint64_t)b * v.D;
    bool same = true;
    for (uint64_t d = lane; d < v.D; d += 64) same &= x[d] == z[d];
    if (__all(same) && lane == 0) atomicOr(&v.dup[b], 1u);
}

// ---- cluster silhouettes --------------------------------------------------------------------------------------------
// the members of the contig's cluster in row order (the contig, row n, comes last): one workgroup per problem
__global__ __launch_bounds__(256) void pl_members_kernel(PlView v) {
    __shared__ uint32_t cnt[256];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t *labels = v.labels + (uint64_t)b * v.n1;
    const uint32_t own = labels[v.n];
    const uint64_t per = (v.n1 + 255) / 256, lo = kb_min(per * t, v.n1), hi = kb_min(lo + per, v.n1);
    uint32_t m = 0;
    for (uint64_t i = lo; i < hi; ++i) m += labels[i] == own ? 1u : 0u;
    cnt[t] = m;
    __syncthreads();
    uint32_t at = 0;
    for (int j = 0; j < t; ++j) at += cnt[j];
    uint32_t *members = v.members + (uint64_t)b * v.n1;
    for (uint64_t i = lo; i < hi; ++i)
        if (labels[i] == own) members[at++] = (uint32_t)i;
    if (t == 255) v.n_members[b] = at;
}

// Workgroup (g, problem) takes members g, g + PL_SIL_GROUPS, ...: distances of the member to all rows (one wave per row,
// direct differences of the rows as given), then per cluster the sum over its rows in row order (one thread per cluster),
// then scikit-learn's silhouette_samples: a = sum_own / (n_own - 1), b = min over the other non-empty clusters of
// sum_c / n_c, (b - a) / max(a, b), NaN (a singleton) -> 0.
__global__ __launch_bounds__(256) void pl_silhouette_kernel(PlView v) {
    const uint32_t g = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nm = v.n_members[b];
    const uint32_t *labels = v.labels + (uint64_t)b * v.n1;
    const uint32_t *members = v.members + (uint64_t)b * v.n1;
    const uint32_t own = labels[v.n];
    const double *z = v.Z + (uint64_t)b * v.D;
    double *dist = v.sdist + ((uint64_t)b * PL_SIL_GROUPS + g) * v.n1;
    double *csum = v.ssum + ((uint64_t)b * PL_SIL_GROUPS + g) * v.k;
    uint32_t *csize = v.ssize + ((uint64_t)b * PL_SIL_GROUPS + g) * v.k;
    for (uint32_t q = g; q < nm; q += PL_SIL_GROUPS) {
        const double *xq = pl_row(v.X, z, v.n, v.D, members[q]);
        for (uint64_t j = wave; j < v.n1; j += 4) {
            const double *xj = pl_row(v.X, z, v.n, v.D, j);
            double acc = 0.0;
            for (uint64_t d = lane; d < v.D; d += 64) {
                const double e = xq[d] - xj[d];
                acc = fma(e, e, acc);
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
            if (lane == 0) dist[j] = sqrt(acc);
        }
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < v.k; c += 256) {
            double s = 0.0;
            uint32_t m = 0;
            for (uint64_t j = 0; j < v.n1; ++j)
                if (labels[j] == c) { s += dist[j]; ++m; }
            csum[c] = s;
            csize[c] = m;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double a = csum[own] / (double)(csize[own] - 1u);
            double bb = __builtin_inf();
            for (uint32_t c = 0; c < v.k; ++c)
                if (c != own && csize[c]) bb = fmin(bb, csum[c] / (double)csize[c]);
            const double s = (bb - a) / fmax(a, bb);
            v.sil[(uint64_t)b * v.n1 + q] = s == s ? s : 0.0;
        }
        __syncthreads();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
extern "C" int phk_placement_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_placement **out) {
    PHK_ENTER(ctx, "phk_placement_create");
    PHK_REQUIRE(X && out, "phk_placement_create: NULL pointer");
    PHK_REQUIRE(n >= 1 && D >= 1 && n < (1ull << 31) - 1, "phk_placement_create: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)D);
    if (!phk_rows_finite(X, n * D)) {
        phk_set_error("phk_placement_create: the reference rows contain NaN or infinity");
        return PHK_ERR_NAN;
    }
    phk_placement *pl = new phk_placement;
    pl->n = n;
    pl->D = D;
    pl->S.assign(D, 0.0);
    pl->SS.assign(D, 0.0);
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t d = 0; d < D; ++d) {
            const double x = X[i * D + d];
            pl->S[d] += x;             // row order: NumPy's add.reduce over axis 0 of a C-contiguous matrix
            pl->SS[d] += x * x;
        }
    int rc = pl->x.alloc("phk_placement_create", "reference rows", n * D * sizeof(double));
    if (rc == PHK_OK) rc = phk_copy_to_device(ctx, pl->x.ptr, X, n * D * sizeof(double));
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PHK_ERR_HIP;
    if (rc != PHK_OK) {
        delete pl;
        return rc;
    }
    *out = pl;
    return PHK_OK;
}

extern "C" int phk_placement_destroy(phk_ctx *ctx, phk_placement *pl) {
    PHK_ENTER(ctx, "phk_placement_destroy");
    if (!pl) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    delete pl;
    return PHK_OK;
}

extern "C" int phk_placement_run(phk_ctx *ctx, phk_placement *pl, const double *Z, uint64_t B, uint32_t k, uint32_t first_seed,
                                 const double *draws, double tol_rel, int max_iter, uint32_t chunk, uint32_t *labels,
                                 uint32_t *seeds, double *sil, uint32_t *n_members, uint32_t *status, int32_t *n_iter,
                                 double *min_gap, double *seed_margin) {
    PHK_ENTER(ctx, "phk_placement_run");
    PHK_REQUIRE(pl, "phk_placement_run: NULL placement");
    const uint64_t n = pl->n, D = pl->D, n1 = n + 1;
    PHK_REQUIRE(k >= 1 && k <= n1, "phk_placement_run: need 1 <= k <= n + 1 (k=%u, n=%llu)", k, (unsigned long long)n);
    PHK_TRY(kb_check_call("phk_placement_run", max_iter, chunk));
    PHK_REQUIRE(tol_rel >= 0.0, "phk_placement_run: bad tol");
    PHK_TRY(kb_check_problem("phk_placement_run", 0, k, n1, first_seed, draws));
    if (B == 0) return PHK_OK;
    PHK_REQUIRE(Z && labels && sil && n_members && status && n_iter && min_gap && seed_margin, "phk_placement_run: NULL pointer");
    if (!phk_rows_finite(Z, B * D)) {
        phk_set_error("phk_placement_run: the contig rows contain NaN or infinity");
        return PHK_ERR_NAN;
    }
    const uint64_t Bc = std::min<uint64_t>(B, chunk ? chunk : PL_DEFAULT_CHUNK);
    // the chunk's workspace: the core's regions (every problem k centres, its own trial stride, one set of draws for all:
    // doff = 0), then the placement's
    PhkLayout ws;
    const KbSpace core(ws, {Bc, n1, D, Bc * k, kb_trials(k), kb_draws(k)});
    const uint64_t o_z = ws.take(Bc * D * 8), o_mean = ws.take(Bc * D * 8), o_own = ws.take(2 * Bc * 4), o_mem = ws.take(Bc * n1 * 4),
                   o_sd = ws.take(Bc * PL_SIL_GROUPS * n1 * 8), o_ss = ws.take(Bc * PL_SIL_GROUPS * (uint64_t)k * 8),
                   o_sc = ws.take(Bc * PL_SIL_GROUPS * (uint64_t)k * 4), o_sil = ws.take(Bc * n1 * 8);
    PHK_TRY(pl->ws.grow(ctx, "phk_placement_run", ws.bytes, Bc));
    char *w = pl->ws.as<char>();
    uint32_t *d_act;
    const KbView kv = core.bind(w, &d_act);
    PlView v;
    v.X = pl->x.as<double>();
    v.Z = (const double *)(w + o_z);
    v.labels = kv.labels;
    v.dup = (uint32_t *)(w + o_own);
    v.n_members = v.dup + Bc;
    v.members = (uint32_t *)(w + o_mem);
    v.sdist = (double *)(w + o_sd);
    v.ssum = (double *)(w + o_ss);
    v.ssize = (uint32_t *)(w + o_sc);
    v.sil = (double *)(w + o_sil);
    v.n = n; v.n1 = n1; v.D = D; v.k = k;
    const KbAppendedRows rows = {v.X, v.Z, (const double *)(w + o_mean), n};
    const KbNames names = {"pl_seed_dist_kernel", "pl_seed_choose_kernel", "pl_assign_kernel", "pl_update_kernel", "pl_stop_kernel"};
    if (k > 1) PHK_HIP(hipMemcpyAsync((double *)kv.draws, draws, kb_draws(k) * 8, hipMemcpyHostToDevice, ctx->stream));

    std::vector<double> mean(Bc * D);
    std::vector<uint32_t> own(2 * Bc);
    KbChunk ch;
    for (uint64_t b0 = 0; b0 < B; b0 += Bc) {
        const uint64_t nb = std::min(Bc, B - b0);
        const unsigned gb = (unsigned)nb;
        // centring and the stopping tolerance: mean = (S + z) / (n + 1); tol = tol_rel * mean over the columns of the
        // column variances of the appended matrix (np.mean(np.var(X, axis=0)) * tol in the single-problem path)
        ch.clear();
        for (uint64_t b = 0; b < nb; ++b) {
            const double *z = Z + (b0 + b) * D;
            double vs = 0.0;
            for (uint64_t d = 0; d < D; ++d) {
                const double m = (pl->S[d] + z[d]) / (double)n1;
                mean[b * D + d] = m;
                const double var = (pl->SS[d] + z[d] * z[d]) / (double)n1 - m * m;
                vs += var > 0.0 ? var : 0.0;
            }
            ch.add(k, first_seed, 0, vs / (double)D * tol_rel);
        }
        PHK_HIP(hipMemcpyAsync(w + o_z, Z + b0 * D, nb * D * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(w + o_mean, mean.data(), nb * D * 8, hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemsetAsync(v.dup, 0, 2 * Bc * 4, ctx->stream));
        PHK_TRY(ch.upload(ctx, kv));
        PHK_LAUNCH(ctx, "pl_dup_kernel",
                   pl_dup_kernel<<<dim3((unsigned)phk_div_up(n, 4), gb), dim3(256), 0, ctx->stream>>>(v));
        PHK_TRY(kb_solve_chunk(ctx, kv, rows, ch, max_iter, d_act, names));
        PHK_LAUNCH(ctx, "pl_members_kernel", pl_members_kernel<<<dim3(gb), dim3(256), 0, ctx->stream>>>(v));
        PHK_LAUNCH(ctx, "pl_silhouette_kernel",
                   pl_silhouette_kernel<<<dim3(PL_SIL_GROUPS, gb), dim3(256), 0, ctx->stream>>>(v));
        PHK_HIP(hipMemcpyAsync(labels + b0 * n1, v.labels, nb * n1 * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipMemcpyAsync(sil + b0 * n1, v.sil, nb * n1 * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (seeds) PHK_HIP(hipMemcpyAsync(seeds + b0 * k, kv.seeds, nb * k * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_HIP(hipMemcpyAsync(own.data(), v.dup, 2 * Bc * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_TRY(ch.download(ctx, kv));
        for (uint64_t b = 0; b < nb; ++b) {
            status[b0 + b] = (own[b] ? PHK_PLACEMENT_DUPLICATE : 0u) | (ch.met_empty(b) ? PHK_PLACEMENT_EMPTY : 0u);
            n_iter[b0 + b] = ch.n_iter(b);
            n_members[b0 + b] = own[Bc + b];
            seed_margin[b0 + b] = ch.seed_margin(b);
            min_gap[b0 + b] = ch.min_gap(b);
        }
    }
    return PHK_OK;
}
