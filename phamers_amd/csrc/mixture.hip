// mixture.hip -- the E-step of a K-component mixture of multinomials on integer count rows (gfx950): DESIGN.md 4.24.
//
//     S[i, k] = sum_j c_i[j] log theta_k[j] + log pi_k        l_i = logsumexp_k S[i, k]        r[i, k] = exp(S[i, k] - l_i)
//     T[k, j] = sum_i r[i, k] c_i[j]        N_k = sum_i r[i, k]        L = sum_i l_i
// The log profiles [K][D] and the log weights [K] are made on the host and uploaded (phk_mix_table): the device takes no
// logarithm of a profile.  A weight of exactly 0 (log = -inf) leaves its component out of every row: r = 0, T row = 0.
//
//   phk_mix_resp_kernel    the shape of phk_lik_partial_kernel: count rows as operand A of gram_tile (uint32, converted in
//                          registers), the log table as operand B, K <= 256 = one chunk, so a row's log-sum-exp is finished in
//                          the workgroup.  S goes to the batch's R buffer [rows][Kp] (Kp = K rounded up to 64) while the
//                          running (max, sum) is kept; once l_i is known every lane reads back the entries it wrote itself
//                          and overwrites them with r.  Per row: l_i, the argmax of r (lowest index on ties) and its r.
//   phk_mix_expect_kernel  T = R^T C on the fp64 matrix pipe, reduced over the ROWS: a wave holds 64 components x 64 columns
//                          (16 accumulators) and walks one block of MIX_RB rows, anchored at the global row index, four rows
//                          per MFMA.  Lane (li, kk) loads r[row + kk][c0 + 4 li .. + 3] (32 bytes) and c[row + kk][j0 + 4 li ..
//                          + 3] (16 bytes): tile (a, t) takes component c0 + 4 m + a and column j0 + 4 n + t -- a permutation
//                          of the outputs, so both operands are vector loads.  The four waves of a workgroup share the rows
//                          and the R operand and take four neighbouring column tiles; N_k and L ride along in the first
//                          column tile's wave as vector adds.  One partial vector (T, N_k, L side by side) per row block.
//   phk_mix_fold_kernel    one level of the fixed tree of 4.23 over the blocks' partial vectors, thread per element.
// T, N_k and L are a function of (rows, table) alone: not of batch_rows, the grid, the entry point or the run.
// The kernels' bodies are the __device__ functions of mixture_body.h, which mixture_sweep.hip (4.25) calls too: the kernels
// here hand them blockIdx.
#include <algorithm>
#include <cmath>

#include "mixture_body.h"   // the three kernels' bodies, shared with mixture_sweep.hip

template <bool FULL>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_mix_resp_kernel(
    const uint32_t *__restrict__ C, uint64_t nq, const double *__restrict__ L, const double *__restrict__ logw, uint32_t K,
    uint32_t Kp, uint64_t D, double *R, double *__restrict__ row_ll, int32_t *__restrict__ amax, double *__restrict__ rmax) {
    mix_resp_body<FULL, true>(C, nq, blockIdx.x, L, logw, K, Kp, D, R, row_ll, amax, rmax);
}

// grid: x = row block of the batch, y = group of four column tiles, z = component tile; the wave takes column tile 4 y + wave.
// R[nb][Kp], C[nb][D], row_ll[nb]: the batch's rows; part: the partial vector of the batch's first block, E doubles per block:
// T[k][j] at k D + j, N_k at K D + k, L at K D + K.  VEC: D % 4 == 0 (16-byte loads of the count rows).
template <bool VEC>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_mix_expect_kernel(const double *__restrict__ R, uint32_t Kp,
                                                                        const uint32_t *__restrict__ C, uint64_t D, uint64_t nb,
                                                                        const double *__restrict__ row_ll, uint32_t K, uint64_t E,
                                                                        double *__restrict__ part) {
    mix_expect_body<VEC>(R, Kp, C, D, nb, row_ll, K, blockIdx.x, blockIdx.y, blockIdx.z, part + (uint64_t)blockIdx.x * E);
}

// grid: x = 256 elements of the vector, y = block of 256 vectors; out[y] = the tree over in[256 y .. 256 y + 255].
__global__ __launch_bounds__(256) void phk_mix_fold_kernel(const double *__restrict__ in, uint64_t m, uint64_t E,
                                                           double *__restrict__ out) {
    mix_fold_body(in, m, E, blockIdx.x, blockIdx.y, out + (uint64_t)blockIdx.y * E);
}

// ---- the resident table ----------------------------------------------------------------------------------------------
struct phk_mix_table {
    uint64_t K = 0, Kp = 0, D = 0;
    PhkDevMem logp;   // [K][D] float64
    PhkDevMem logw;   // [Kp] float64, -inf past K
};

static int mix_table_upload(phk_ctx *ctx, const char *fname, phk_mix_table *t, const double *log_profiles,
                            const double *log_weights) {
    PHK_REQUIRE(log_profiles && log_weights, "%s: NULL pointer", fname);
    bool any = false;
    for (uint64_t k = 0; k < t->K; ++k) {
        const double w = log_weights[k];
        if (w != w || w == __builtin_inf()) {
            phk_set_error("%s: log weight %llu is %g", fname, (unsigned long long)k, w);
            return PHK_ERR_NAN;
        }
        any = any || w > -__builtin_inf();
    }
    if (!phk_rows_finite(log_profiles, t->K * t->D)) {
        phk_set_error("%s: the log profiles hold a value that is not finite (a zero profile entry?)", fname);
        return PHK_ERR_NAN;
    }
    PHK_REQUIRE(any, "%s: every component has weight 0", fname);
    std::vector<double> w(t->Kp, -__builtin_inf());
    std::copy(log_weights, log_weights + t->K, w.begin());
    PHK_TRY(phk_copy_to_device(ctx, t->logp.ptr, log_profiles, t->K * t->D * sizeof(double)));
    PHK_TRY(phk_copy_to_device(ctx, t->logw.ptr, w.data(), t->Kp * sizeof(double)));
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // w leaves scope
    return PHK_OK;
}

extern "C" int phk_mix_table_create(phk_ctx *ctx, const double *log_profiles, const double *log_weights, uint64_t K, uint64_t D,
                                    phk_mix_table **out) {
    PHK_ENTER(ctx, "phk_mix_table_create");
    PHK_REQUIRE(out, "phk_mix_table_create: NULL out");
    *out = nullptr;
    PHK_REQUIRE(K >= 1 && K <= MIX_KMAX, "phk_mix_table_create: %llu components (1 to %d)", (unsigned long long)K, MIX_KMAX);
    PHK_REQUIRE(D > 0 && D < (1ull << 32), "phk_mix_table_create: %llu columns", (unsigned long long)D);
    phk_mix_table *t = new phk_mix_table();
    t->K = K, t->D = D, t->Kp = phk_div_up(K, MIX_CT) * MIX_CT;
    int rc = t->logp.alloc("phk_mix_table_create", "log profiles", K * D * sizeof(double));
    if (rc == PHK_OK) rc = t->logw.alloc("phk_mix_table_create", "log weights", t->Kp * sizeof(double));
    if (rc == PHK_OK) rc = mix_table_upload(ctx, "phk_mix_table_create", t, log_profiles, log_weights);
    if (rc != PHK_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return PHK_OK;
}

extern "C" int phk_mix_table_update(phk_ctx *ctx, phk_mix_table *t, const double *log_profiles, const double *log_weights,
                                    uint64_t K, uint64_t D) {
    PHK_ENTER(ctx, "phk_mix_table_update");
    PHK_REQUIRE(t, "phk_mix_table_update: NULL table");
    PHK_REQUIRE(K == t->K && D == t->D, "phk_mix_table_update: the table is %llu x %llu, not %llu x %llu",
                (unsigned long long)t->K, (unsigned long long)t->D, (unsigned long long)K, (unsigned long long)D);
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    return mix_table_upload(ctx, "phk_mix_table_update", t, log_profiles, log_weights);
}

extern "C" int phk_mix_table_destroy(phk_ctx *ctx, phk_mix_table *t) {
    if (!t) return PHK_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete t;
    return PHK_OK;
}

extern "C" uint64_t phk_mix_block_rows(void) { return MIX_RB; }

// What a call wants back (host pointers; NULL = not asked for).  expect: T, Nk and L together.
struct MixOut {
    double *T = nullptr, *Nk = nullptr, *L = nullptr, *row_ll = nullptr, *max_resp = nullptr, *resp = nullptr;
    int32_t *argmax = nullptr;
    bool expect() const { return T != nullptr; }
};

// The loop of every entry: count rows d_counts[N][D] on the device, in batches of B rows -- a multiple of the reduction
// block, so that every block starts at a multiple of MIX_RB of the GLOBAL row index; B keeps the R buffer within 512 MiB
// (force_B != 0: that many, rounded up to the block; for tests).  Every block's partial vector is kept until the fold.
static int mix_run(phk_ctx *ctx, const char *fname, const phk_mix_table *t, const uint32_t *d_counts, uint64_t N,
                   uint64_t force_B, const MixOut &o) {
    const uint64_t K = t->K, Kp = t->Kp, D = t->D, E = K * D + K + 1;
    uint64_t B = (512ull << 20) / (Kp * sizeof(double));
    B = B > (1ull << 20) ? (1ull << 20) : B;
    B = B / MIX_RB * MIX_RB;
    if (force_B) B = phk_div_up(force_B, MIX_RB) * MIX_RB;
    const uint64_t Brows = B > N ? N : B;
    const uint64_t nblocks = phk_div_up(N, MIX_RB), nfold = phk_div_up(nblocks, 256);
    PhkLayout lay;
    const uint64_t o_R = lay.take(Brows * Kp * 8), o_ll = lay.take(N * 8), o_rmax = lay.take(N * 8), o_amax = lay.take(N * 4);
    const uint64_t o_part = lay.take(o.expect() ? nblocks * E * 8 : 0), o_f0 = lay.take(o.expect() ? nfold * E * 8 : 0),
                   o_f1 = lay.take(o.expect() ? nfold * E * 8 : 0);
    void *ws;
    PHK_TRY(phk_ws(ctx, WS_MIX, lay.bytes, &ws));
    char *w8 = (char *)ws;
    double *d_R = (double *)(w8 + o_R), *d_ll = (double *)(w8 + o_ll), *d_rmax = (double *)(w8 + o_rmax);
    int32_t *d_amax = (int32_t *)(w8 + o_amax);
    double *d_part = (double *)(w8 + o_part), *d_fold[2] = {(double *)(w8 + o_f0), (double *)(w8 + o_f1)};
    const double *d_L = t->logp.as<double>(), *d_w = t->logw.as<double>();
    const bool full = D % GT_KC == 0, vec = D % 4 == 0;
    for (uint64_t s = 0; s < N; s += B) {
        const uint64_t nb = N - s < B ? N - s : B;
        const dim3 g1((unsigned)phk_div_up(nb, GT_QB)), blk(GT_WAVES * 64);
        if (full) {
            PHK_LAUNCH(ctx, "phk_mix_resp_kernel", phk_mix_resp_kernel<true><<<g1, blk, 0, ctx->stream>>>(
                                                       d_counts + s * D, nb, d_L, d_w, (uint32_t)K, (uint32_t)Kp, D, d_R, d_ll + s,
                                                       d_amax + s, d_rmax + s));
        } else {
            PHK_LAUNCH(ctx, "phk_mix_resp_kernel", phk_mix_resp_kernel<false><<<g1, blk, 0, ctx->stream>>>(
                                                       d_counts + s * D, nb, d_L, d_w, (uint32_t)K, (uint32_t)Kp, D, d_R, d_ll + s,
                                                       d_amax + s, d_rmax + s));
        }
        if (o.expect()) {
            const dim3 g2((unsigned)phk_div_up(nb, MIX_RB), (unsigned)phk_div_up(D, GT_WAVES * MIX_CT), (unsigned)(Kp / MIX_CT));
            double *part = d_part + (s / MIX_RB) * E;
            if (vec) {
                PHK_LAUNCH(ctx, "phk_mix_expect_kernel", phk_mix_expect_kernel<true><<<g2, blk, 0, ctx->stream>>>(
                                                             d_R, (uint32_t)Kp, d_counts + s * D, D, nb, d_ll + s, (uint32_t)K, E, part));
            } else {
                PHK_LAUNCH(ctx, "phk_mix_expect_kernel", phk_mix_expect_kernel<false><<<g2, blk, 0, ctx->stream>>>(
                                                             d_R, (uint32_t)Kp, d_counts + s * D, D, nb, d_ll + s, (uint32_t)K, E, part));
            }
        }
        if (o.resp) {
            PHK_HIP(hipMemcpy2DAsync(o.resp + s * K, K * 8, d_R, Kp * 8, K * 8, nb, hipMemcpyDeviceToHost, ctx->stream));
            PHK_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    if (o.expect()) {
        const double *in = d_part;
        uint64_t m = nblocks;
        int level = 0;
        for (;; ++level) {
            const uint64_t blocks = phk_div_up(m, 256);
            PHK_LAUNCH(ctx, "phk_mix_fold_kernel",
                       phk_mix_fold_kernel<<<dim3((unsigned)phk_div_up(E, 256), (unsigned)blocks), dim3(256), 0, ctx->stream>>>(
                           in, m, E, d_fold[level & 1]));
            in = d_fold[level & 1], m = blocks;
            if (blocks == 1) break;
        }
        std::vector<double> tot(E);
        PHK_TRY(phk_copy_to_host(ctx, tot.data(), in, E * 8));
        std::copy(tot.begin(), tot.begin() + K * D, o.T);
        std::copy(tot.begin() + K * D, tot.begin() + K * D + K, o.Nk);
        *o.L = tot[K * D + K];
    }
    if (o.row_ll) PHK_TRY(phk_copy_to_host(ctx, o.row_ll, d_ll, N * 8));
    if (o.argmax) PHK_TRY(phk_copy_to_host(ctx, o.argmax, d_amax, N * 4));
    if (o.max_resp) PHK_TRY(phk_copy_to_host(ctx, o.max_resp, d_rmax, N * 8));
    return PHK_OK;
}

// the checks of the four entries; N == 0: PHK_OK with zeros, nothing launched
static int mix_enter(const char *fname, const phk_mix_table *t, uint64_t D, uint64_t N, const MixOut &o, bool *empty) {
    PHK_REQUIRE(t, "%s: NULL table", fname);
    PHK_REQUIRE(D == t->D, "%s: the counts have %llu columns, the table %llu", fname, (unsigned long long)D,
                (unsigned long long)t->D);
    PHK_REQUIRE(N < (1ull << 32), "%s: 2^32 rows or more in one call", fname);
    PHK_REQUIRE(!o.T == !o.Nk && !o.T == !o.L, "%s: T, Nk and L go together", fname);
    PHK_REQUIRE(o.T || o.resp, "%s: NULL pointer", fname);
    *empty = N == 0;
    if (N == 0 && o.T) {
        std::fill(o.T, o.T + t->K * t->D, 0.0);
        std::fill(o.Nk, o.Nk + t->K, 0.0);
        *o.L = 0.0;
    }
    return PHK_OK;
}

static int mix_host(phk_ctx *ctx, const char *fname, const phk_mix_table *t, const uint32_t *counts, uint64_t N, uint64_t D,
                    uint64_t batch_rows, const MixOut &o) {
    bool empty;
    PHK_TRY(mix_enter(fname, t, D, N, o, &empty));
    if (empty) return PHK_OK;
    PHK_REQUIRE(counts, "%s: NULL counts", fname);
    void *d_c;
    PHK_TRY(phk_ws(ctx, WS_COUNTS, N * D * sizeof(uint32_t), &d_c));
    PHK_TRY(phk_copy_to_device(ctx, d_c, counts, N * D * sizeof(uint32_t)));
    return mix_run(ctx, fname, t, (const uint32_t *)d_c, N, batch_rows, o);
}

static int mix_batch(phk_ctx *ctx, const char *fname, const phk_mix_table *t, const phk_batch *b, uint64_t batch_rows,
                     const MixOut &o) {
    PHK_REQUIRE(b, "%s: NULL batch", fname);
    bool empty;
    PHK_TRY(mix_enter(fname, t, b->D, b->n, o, &empty));
    if (empty) return PHK_OK;
    return mix_run(ctx, fname, t, b->d_counts, b->n, batch_rows, o);
}

static MixOut mix_out(double *T, double *Nk, double *L, double *row_ll, int32_t *argmax, double *max_resp, double *resp) {
    MixOut o;
    o.T = T, o.Nk = Nk, o.L = L, o.row_ll = row_ll, o.argmax = argmax, o.max_resp = max_resp, o.resp = resp;
    return o;
}

extern "C" int phk_mix_expect(phk_ctx *ctx, const phk_mix_table *t, const uint32_t *counts, uint64_t N, uint64_t D,
                              uint64_t batch_rows, double *T, double *Nk, double *L, double *row_ll, int32_t *argmax,
                              double *max_resp) {
    PHK_ENTER(ctx, "phk_mix_expect");
    PHK_REQUIRE(T && Nk && L, "phk_mix_expect: NULL T, Nk or L");
    return mix_host(ctx, "phk_mix_expect", t, counts, N, D, batch_rows, mix_out(T, Nk, L, row_ll, argmax, max_resp, nullptr));
}

extern "C" int phk_batch_mix_expect(phk_ctx *ctx, const phk_mix_table *t, const phk_batch *b, uint64_t batch_rows, double *T,
                                    double *Nk, double *L, double *row_ll, int32_t *argmax, double *max_resp) {
    PHK_ENTER(ctx, "phk_batch_mix_expect");
    PHK_REQUIRE(T && Nk && L, "phk_batch_mix_expect: NULL T, Nk or L");
    return mix_batch(ctx, "phk_batch_mix_expect", t, b, batch_rows, mix_out(T, Nk, L, row_ll, argmax, max_resp, nullptr));
}

extern "C" int phk_mix_responsibilities(phk_ctx *ctx, const phk_mix_table *t, const uint32_t *counts, uint64_t N, uint64_t D,
                                        uint64_t batch_rows, double *resp, double *row_ll) {
    PHK_ENTER(ctx, "phk_mix_responsibilities");
    PHK_REQUIRE(resp, "phk_mix_responsibilities: NULL resp");
    return mix_host(ctx, "phk_mix_responsibilities", t, counts, N, D, batch_rows,
                    mix_out(nullptr, nullptr, nullptr, row_ll, nullptr, nullptr, resp));
}

extern "C" int phk_batch_mix_responsibilities(phk_ctx *ctx, const phk_mix_table *t, const phk_batch *b, uint64_t batch_rows,
                                              double *resp, double *row_ll) {
    PHK_ENTER(ctx, "phk_batch_mix_responsibilities");
    PHK_REQUIRE(resp, "phk_batch_mix_responsibilities: NULL resp");
    return mix_batch(ctx, "phk_batch_mix_responsibilities", t, b, batch_rows,
                     mix_out(nullptr, nullptr, nullptr, row_ll, nullptr, nullptr, resp));
}
