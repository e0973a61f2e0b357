// sweep.hip -- the silhouette-against-k sweep of scripts/cluster.py:31-47 (KMeans(k, random_state) for a grid of k on one
// feature matrix, the mean silhouette of each fit) as batched k-means: the SAME rows, a different k -- and, if the caller
// wants, a different seed -- per problem.  gfx950.  (placement.hip batches along the other axis: one k, one more row each.)
//
// The rows X[n][D] are resident (phk_sweep_create), raw and centred by their column mean (NumPy's X - X.mean(axis=0), bit
// for bit: what KMeans.fit and learning.kmeans_reference_on_device run on).  phk_sweep_run solves S problems in chunks of
// problems, every stage one launch for the whole chunk, the grid's second dimension the problem:
//   seeding, Lloyd : kmeans_batch.h's batched k-means (shared with placement.hip) on the centred rows, each problem with
//              its own k_s, first row and draws; labels, sweep counts and min_gap equal the single-problem path's bit for bit;
//   silhouettes of all rows : the pair distances d[n][n] (raw rows, float64 direct differences by fma in column order,
//              pair_tile.h) do not depend on the problem: they are computed ONCE per call; per problem a thread per row
//              then adds, cluster by cluster, the stored distances in exactly the order phk_cl_silhouette_sums_kernel
//              takes them and applies phk_cl_silhouette_finish_kernel's rules: equal to phk_silhouettes bit for bit.
//              Budget: d takes n^2 * 8 bytes; when that exceeds the caller's budget (default: a quarter of the free device
//              memory at the call) the problems go one after the other through phk_silhouettes' own pass on the resident
//              rows instead: same bits, the pair pass paid per problem.
// Everything is float64 and order-deterministic (the only atomics are integer counts and minima); every sum's order is
// fixed by n, the labels and the problem alone, so a problem's result does not depend on S, on its place or on `chunk`.
#include "kmeans_batch.h"
#include "pair_tile.h"

#define SW_DEFAULT_CHUNK 64

struct phk_sweep {
    uint64_t n = 0, D = 0;
    PhkDevMem x, xc;          // raw rows, centred rows
    double var_mean = 0.0;    // np.mean(np.var(centred rows, axis=0))
    PhkDevMem ws;             // the chunks' workspace
    PhkDevMem pair;           // d[n][n], kept between calls
};

// ---- silhouettes ----------------------------------------------------------------------------------------------------
// d[q][j] = sqrt(sum_k (x_qk - x_jk)^2) for all pairs of the raw rows: pair_tile.h's tile with the square root as its
// stored value.  The same bits for (q, j) and (j, q).
struct SwStoreSqrt {
    __device__ double operator()(uint64_t, uint64_t, double s) const { return sqrt(s); }
};

// One thread per (row q, problem).  perm = the problem's rows sorted by label (stable); cluster c = perm[first[c] ..
// first[c + 1]).  phk_cl_silhouette_sums_kernel gives the 16 threads of a query the columns tx, tx + 16, tx + 32, tx + 48
// of each chunk of 64 of the cluster, chunk after chunk -- thread tx adds the members at positions tx, tx + 16, tx + 32,
// ... of the cluster in that order -- and folds the 16 sums by the butterfly xor 1, 2, 4, 8: here one thread keeps the 16
// sums and folds them as that butterfly does.  Then phk_cl_silhouette_finish_kernel's rules.  d is read as d[member][q]
// (= d[q][member] bit for bit): the 64 rows of a wave read 64 neighbouring values.
__global__ __launch_bounds__(256) void sw_silhouette_kernel(const double *__restrict__ dist, uint64_t n, const KbState *__restrict__ st,
                                                           const uint32_t *__restrict__ labels, const uint32_t *__restrict__ perm,
                                                           const uint32_t *__restrict__ first, const uint8_t *__restrict__ want,
                                                           double *__restrict__ out) {
    const uint32_t b = blockIdx.y;
    if (!want[b]) return;
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t qq = q < n ? q : n - 1;
    const uint32_t k = st[b].k;
    const uint32_t *pm = perm + (uint64_t)b * n, *fs = first + st[b].koff + b;   // (k + 1 entries per problem)
    const uint32_t own = labels[(uint64_t)b * n + qq];
    double a_own = 0.0, bb = __builtin_inf();
    uint32_t n_own = 0;
    for (uint32_t c = 0; c < k; ++c) {
        const uint32_t f0 = fs[c], size = fs[c + 1] - f0;
        if (size == 0) continue;
        double a[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = 0.0;
        for (uint32_t p = 0; p < size; p += 16) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (p + j < size) a[j] += dist[(uint64_t)pm[f0 + p + j] * n + qq];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)
#pragma unroll
            for (int j = 0; j < 16; j += 2 * o) a[j] += a[j + o];
        if (c == own) { a_own = a[0]; n_own = size; }
        else bb = fmin(bb, a[0] / (double)size);
    }
    const double aa = a_own / (double)(n_own - 1u);
    const double s = (bb - aa) / fmax(aa, bb);
    if (q < n) out[(uint64_t)b * n + q] = s == s ? s : 0.0;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// np.add.reduce of a contiguous float64 vector: pairwise, in pieces of 8192 (rows.hip's phk_np_pairwise_sum on the host)
static double sw_np_pairwise(const double *a, uint64_t n) {
    if (n < 8) {
        double r = 0.0;
        for (uint64_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        uint64_t i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    uint64_t n2 = n / 2;
    n2 -= n2 % 8;
    return sw_np_pairwise(a, n2) + sw_np_pairwise(a + n2, n - n2);
}

static double sw_np_sum(const double *a, uint64_t n) {
    double s = sw_np_pairwise(a, std::min<uint64_t>(n, 8192));
    for (uint64_t o = 8192; o < n; o += 8192) s += sw_np_pairwise(a + o, std::min<uint64_t>(n - o, 8192));
    return s;
}

extern "C" int phk_sweep_create(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, phk_sweep **out) {
    PHK_ENTER(ctx, "phk_sweep_create");
    PHK_REQUIRE(X && out, "phk_sweep_create: NULL pointer");
    PHK_REQUIRE(n >= 1 && D >= 1 && n < (1ull << 31) - 1, "phk_sweep_create: bad shape (%llu x %llu)", (unsigned long long)n,
                (unsigned long long)D);
    if (!phk_rows_finite(X, n * D)) {
        phk_set_error("phk_sweep_create: the rows contain NaN or infinity");
        return PHK_ERR_NAN;
    }
    // NumPy's X - X.mean(axis=0) and np.mean(np.var(that, axis=0)): column sums in row order, one division each -- except
    // that a matrix of ONE column is a contiguous vector to NumPy's reduction, which it sums pairwise
    std::vector<double> mean(D, 0.0), xc(n * D), m2(D, 0.0), var(D, 0.0), sq;
    auto column_sums = [&](const double *A, std::vector<double> &out) {
        if (D == 1) {
            out[0] = sw_np_sum(A, n);
            return;
        }
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t d = 0; d < D; ++d) out[d] += A[i * D + d];
    };
    column_sums(X, mean);
    for (uint64_t d = 0; d < D; ++d) mean[d] /= (double)n;
    for (uint64_t i = 0; i < n * D; ++i) xc[i] = X[i] - mean[i % D];
    column_sums(xc.data(), m2);
    for (uint64_t d = 0; d < D; ++d) m2[d] /= (double)n;
    sq.resize(n * D);
    for (uint64_t i = 0; i < n * D; ++i) {
        const double e = xc[i] - m2[i % D];
        sq[i] = e * e;
    }
    column_sums(sq.data(), var);
    for (uint64_t d = 0; d < D; ++d) var[d] /= (double)n;
    phk_sweep *sw = new phk_sweep;
    sw->n = n;
    sw->D = D;
    sw->var_mean = sw_np_sum(var.data(), D) / (double)D;
    const uint64_t bytes = n * D * sizeof(double);
    int rc = sw->x.alloc("phk_sweep_create", "rows", bytes);
    if (rc == PHK_OK) rc = sw->xc.alloc("phk_sweep_create", "centred rows", bytes);
    if (rc == PHK_OK) rc = phk_copy_to_device(ctx, sw->x.ptr, X, bytes);
    if (rc == PHK_OK) rc = phk_copy_to_device(ctx, sw->xc.ptr, xc.data(), bytes);
    if (rc == PHK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PHK_ERR_HIP;
    if (rc != PHK_OK) {
        delete sw;
        return rc;
    }
    *out = sw;
    return PHK_OK;
}

extern "C" int phk_sweep_destroy(phk_ctx *ctx, phk_sweep *sw) {
    PHK_ENTER(ctx, "phk_sweep_destroy");
    if (!sw) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    delete sw;
    return PHK_OK;
}

extern "C" int phk_sweep_run(phk_ctx *ctx, phk_sweep *sw, uint64_t S, const uint32_t *ks, const uint32_t *first_seed,
                             const double *draws, const uint64_t *draw_off, double tol_rel, int max_iter, uint32_t chunk,
                             int64_t pair_budget, uint32_t *labels, uint32_t *seeds, double *sil, uint32_t *status, int32_t *n_iter,
                             double *min_gap, double *seed_margin) {
    PHK_ENTER(ctx, "phk_sweep_run");
    PHK_REQUIRE(sw, "phk_sweep_run: NULL sweep");
    const uint64_t n = sw->n, D = sw->D;
    const double *d_x = sw->x.as<double>();
    PHK_TRY(kb_check_call("phk_sweep_run", max_iter, chunk));
    PHK_REQUIRE(tol_rel >= 0.0, "phk_sweep_run: bad tol");
    if (S == 0) return PHK_OK;
    PHK_REQUIRE(ks && first_seed && draw_off && labels && status && n_iter && min_gap && seed_margin, "phk_sweep_run: NULL pointer");
    for (uint64_t s = 0; s < S; ++s) {
        PHK_TRY(kb_check_problem("phk_sweep_run", s, ks[s], n, first_seed[s], draws));
        PHK_REQUIRE(!sil || (ks[s] >= 2 && (uint64_t)ks[s] <= n - 1 && n >= 3),
                    "phk_sweep_run: Number of labels is %u. Valid values are 2 to n_samples - 1 (inclusive)", ks[s]);
    }
    // chunks of Sc problems in the caller's order
    const uint64_t Sc = std::min<uint64_t>(S, chunk ? chunk : SW_DEFAULT_CHUNK);
    std::vector<uint64_t> cut;
    for (uint64_t s0 = 0; s0 < S; s0 += Sc) cut.push_back(s0);
    cut.push_back(S);
    // the pair distances, once per call, when they fit the budget
    bool stored = false;
    if (sil) {
        uint64_t budget;
        if (pair_budget < 0) {
            size_t free_b = 0, total_b = 0;
            PHK_HIP(hipMemGetInfo(&free_b, &total_b));
            budget = (uint64_t)free_b / 4 + sw->pair.bytes;   // (the kept matrix is not "used" memory here)
        } else {
            budget = (uint64_t)pair_budget;
        }
        stored = n * n * 8 <= budget;
        if (stored && !sw->pair.ptr) {
            if (sw->pair.alloc("phk_sweep_run", "pair distances", n * n * 8) != PHK_OK) {
                stored = false;   // no room after all: the per-problem pass
            } else {
                const uint64_t tiles = phk_div_up(n, CL_T);
                const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(65535, CL_MAX_BLOCKS / tiles));
                for (uint64_t y0 = 0; y0 < tiles; y0 += step)
                    PHK_LAUNCH(ctx, "sw_pair_kernel",
                               cl_matrix_kernel<SwStoreSqrt>
                               <<<dim3((unsigned)tiles, (unsigned)std::min(step, tiles - y0)), dim3(CL_THREADS), 0, ctx->stream>>>(
                                   d_x, n, y0, d_x, n, D, sw->pair.as<double>() + y0 * CL_T * n, nullptr));
            }
        }
    }
    // the chunk's workspace: the core's regions, then the silhouettes'
    PhkLayout ws;
    const KbSpace core(ws, kb_extent(ks, nullptr, cut, n, D));
    const uint64_t o_perm = ws.take(sil ? Sc * n * 4 : 0), o_first = ws.take(sil ? (core.e.ksum + Sc) * 4 : 0), o_want = ws.take(Sc),
                   o_sil = ws.take(sil ? Sc * n * 8 : 0);
    PHK_TRY(sw->ws.grow(ctx, "phk_sweep_run", ws.bytes, Sc));
    char *w = sw->ws.as<char>();
    uint32_t *d_act;
    const KbView v = core.bind(w, &d_act);
    const KbCentredRows rows = {sw->xc.as<double>()};
    const KbNames names = {"sw_seed_dist_kernel", "sw_seed_choose_kernel", "sw_assign_kernel", "sw_update_kernel", "sw_stop_kernel"};
    uint32_t *d_perm = (uint32_t *)(w + o_perm), *d_first = (uint32_t *)(w + o_first);
    uint8_t *d_want = (uint8_t *)(w + o_want);
    double *d_sil = (double *)(w + o_sil);

    KbChunk ch;
    std::vector<uint32_t> perm, first;
    std::vector<uint8_t> want(Sc);
    const double tol = sw->var_mean * tol_rel;
    uint64_t seed_out = 0;   // centres of the problems before the chunk
    for (uint64_t ci = 0; ci + 1 < cut.size(); ++ci) {
        const uint64_t s0 = cut[ci], nb = cut[ci + 1] - s0;
        const unsigned gb = (unsigned)nb;
        ch.clear();
        for (uint64_t s = s0; s < s0 + nb; ++s)
            PHK_TRY(ch.add(ctx, v, ks[s], first_seed[s], draws ? draws + draw_off[s] : nullptr, tol));
        PHK_TRY(ch.upload(ctx, v));
        PHK_TRY(kb_solve_chunk(ctx, v, rows, ch, max_iter, d_act, names));
        PHK_HIP(hipMemcpyAsync(labels + s0 * n, v.labels, nb * n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (seeds) PHK_HIP(hipMemcpyAsync(seeds + seed_out, v.seeds, (uint64_t)ch.ksum * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHK_TRY(ch.download(ctx, v));
        for (uint64_t b = 0; b < nb; ++b) {
            status[s0 + b] = ch.met_empty(b) ? PHK_SWEEP_EMPTY : 0u;
            n_iter[s0 + b] = ch.n_iter(b);
            seed_margin[s0 + b] = ch.seed_margin(b);
            min_gap[s0 + b] = ch.min_gap(b);
        }
        if (sil && stored) {
            // rows sorted by label (stable) and the clusters' first positions, per problem
            perm.assign(nb * n, 0);
            first.assign((uint64_t)ch.ksum + nb, 0);
            for (uint64_t b = 0; b < nb; ++b) {
                const uint32_t k = ch.st[b].k;
                const uint32_t *lab = labels + (s0 + b) * n;
                uint32_t *f = first.data() + ch.st[b].koff + b;
                bool ok = true;
                for (uint64_t i = 0; i < n; ++i) {
                    if (lab[i] >= k) { ok = false; break; }
                    ++f[lab[i] + 1];
                }
                want[b] = ok;
                if (!ok) continue;
                for (uint32_t c = 0; c < k; ++c) f[c + 1] += f[c];
                std::vector<uint32_t> at(f, f + k);
                for (uint64_t i = 0; i < n; ++i) perm[b * n + at[lab[i]]++] = (uint32_t)i;
            }
            PHK_HIP(hipMemcpyAsync(d_perm, perm.data(), nb * n * 4, hipMemcpyHostToDevice, ctx->stream));
            PHK_HIP(hipMemcpyAsync(d_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            PHK_HIP(hipMemcpyAsync(d_want, want.data(), nb, hipMemcpyHostToDevice, ctx->stream));
            PHK_LAUNCH(ctx, "sw_silhouette_kernel",
                       sw_silhouette_kernel<<<dim3((unsigned)phk_div_up(n, 256), gb), dim3(256), 0, ctx->stream>>>(
                           sw->pair.as<double>(), n, v.st, v.labels, d_perm, d_first, d_want, d_sil));
            PHK_TRY(phk_copy_to_host(ctx, sil + s0 * n, d_sil, nb * n * 8));
        } else if (sil) {
            for (uint64_t b = 0; b < nb; ++b)
                PHK_TRY(phk_silhouettes_resident(ctx, d_x, n, D, labels + (s0 + b) * n, ch.st[b].k, sil + (s0 + b) * n));
        }
        seed_out += ch.ksum;
    }
    return PHK_OK;
}
