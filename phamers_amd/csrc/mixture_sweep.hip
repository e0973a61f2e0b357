// mixture_sweep.hip -- the mixture E-step of mixture.hip for many (row set, table) jobs in one call (gfx950): DESIGN.md 4.25.
//
// A sweep object holds count rows and a list of row sets (ascending row indices); each set is gathered once into its own
// contiguous [n_s][D] buffer (a set of all rows aliases the source), so the kernels keep gram_tile.h's contiguous-row
// loaders.  A step takes J jobs (set, K_j, log profiles, log weights) and returns every job's T, N_k, L (and l_i):
//
//   phk_mixsweep_resp_kernel    mix_resp_body for the workgroup's (job, row tile)
//   phk_mixsweep_expect_kernel  mix_expect_body for the workgroup's (job, row block, column group, component tile)
//   phk_mixsweep_fold_kernel    mix_fold_body for the workgroup's (job, block of vectors, 256 elements), one launch per level
//
// A workgroup finds its work in a descriptor table the host builds per call and the kernel reads at blockIdx.x (a uniform
// address: scalar loads); K_j and n_s are uniform inside a workgroup.  The bodies are those of the single-table kernels
// (mixture_body.h), the blocks are anchored at the position in the row set, and the tree runs over a job's own partial
// vectors: a job's results are the bits phk_mix_expect gives for that job's rows alone.  The jobs go in groups whose
// buffers (R, partial vectors, fold levels) stay under a byte budget; a job never learns which group it is in.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mixture_body.h"

struct MixSweepJob {       // one per job of a call
    const uint32_t *C;     // the set's rows [n][D]
    uint64_t n;
    uint64_t logp, logw;   // first double of the job's table / padded weights in the call's uploads
    uint64_t R;            // first double of the job's R [n][Kp] in the group's buffer
    uint64_t ll;           // first double of the job's l_i in the call's row buffer
    uint64_t part;         // first double of the job's partial vectors [blocks][E] in the group's buffer
    uint64_t E;            // K D + K + 1
    uint32_t K, Kp;
};
struct MixSweepTile {      // resp: tile = row tile (x = y = 0); expect: tile = row block, y = column group, z = component tile
    uint32_t job, tile, y, z;
};
struct MixSweepFold {      // one workgroup of a fold level: 256 elements ex of the tree over vectors 256 vb .. of in (m vectors)
    uint64_t in, out;      // first double of the input vectors / of the output vector, in the call's workspace
    uint64_t m, E;
    uint32_t ex, vb;
};

template <bool FULL>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_mixsweep_resp_kernel(const MixSweepJob *__restrict__ jobs,
                                                                           const MixSweepTile *__restrict__ tiles, uint64_t D,
                                                                           const double *__restrict__ logp,
                                                                           const double *__restrict__ logw, double *R,
                                                                           double *__restrict__ row_ll) {
    const MixSweepTile t = tiles[blockIdx.x];
    const MixSweepJob j = jobs[t.job];
    mix_resp_body<FULL, false>(j.C, j.n, t.tile, logp + j.logp, logw + j.logw, j.K, j.Kp, D, R + j.R, row_ll + j.ll, nullptr,
                               nullptr);
}

template <bool VEC>
__global__ __launch_bounds__(GT_WAVES * 64, 2) void phk_mixsweep_expect_kernel(const MixSweepJob *__restrict__ jobs,
                                                                             const MixSweepTile *__restrict__ tiles, uint64_t D,
                                                                             const double *__restrict__ R,
                                                                             const double *__restrict__ row_ll,
                                                                             double *__restrict__ part) {
    const MixSweepTile t = tiles[blockIdx.x];
    const MixSweepJob j = jobs[t.job];
    mix_expect_body<VEC>(R + j.R, j.Kp, j.C, D, j.n, row_ll + j.ll, j.K, t.tile, t.y, t.z, part + j.part + (uint64_t)t.tile * j.E);
}

__global__ __launch_bounds__(256) void phk_mixsweep_fold_kernel(const MixSweepFold *__restrict__ folds, double *ws) {
    const MixSweepFold f = folds[blockIdx.x];
    mix_fold_body(ws + f.in, f.m, f.E, f.ex, f.vb, ws + f.out);
}

// dst[i][:] = src[idx[i]][:], thread per element
__global__ __launch_bounds__(256) void phk_mixsweep_gather_kernel(const uint32_t *__restrict__ src, uint64_t D,
                                                                  const uint32_t *__restrict__ idx, uint64_t n,
                                                                  uint32_t *__restrict__ dst) {
    const uint64_t total = n * D;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        const uint64_t i = e / D;
        dst[e] = src[(uint64_t)idx[i] * D + (e - i * D)];
    }
}

// ---- the sweep object --------------------------------------------------------------------------------------------------
struct phk_mix_sweep {
    uint64_t N = 0, D = 0;
    PhkDevMem own;                       // the source rows when they came from the host
    const uint32_t *src = nullptr;       // [N][D]: own, or the batch's rows (the batch outlives the sweep)
    PhkDevMem rows;                      // the gathered sets, one after another
    std::vector<const uint32_t *> set;   // every set's rows
    std::vector<uint64_t> n;             // every set's size
};

static int sweep_sets(phk_ctx *ctx, const char *fname, phk_mix_sweep *s, const uint32_t *set_rows, const uint64_t *set_offsets,
                      uint64_t n_sets) {
    PHK_REQUIRE(n_sets == 0 || (set_rows && set_offsets), "%s: NULL row sets", fname);
    PhkLayout lay;
    std::vector<uint64_t> at(n_sets, 0);
    for (uint64_t i = 0; i < n_sets; ++i) {
        const uint64_t a = set_offsets[i], b = set_offsets[i + 1];
        PHK_REQUIRE(b > a, "%s: row set %llu is empty", fname, (unsigned long long)i);
        for (uint64_t p = a; p < b; ++p)
            PHK_REQUIRE(set_rows[p] < s->N && (p == a || set_rows[p] > set_rows[p - 1]),
                        "%s: row set %llu is not an ascending list of rows below %llu", fname, (unsigned long long)i,
                        (unsigned long long)s->N);
        s->n.push_back(b - a);
        if (b - a != s->N) at[i] = lay.take((b - a) * s->D * sizeof(uint32_t));   // (all rows in order: the source itself)
    }
    PHK_TRY(s->rows.alloc(fname, "row sets", lay.bytes));
    const uint64_t total = n_sets ? set_offsets[n_sets] : 0;
    void *d_idx;
    PHK_TRY(phk_ws(ctx, WS_WIDE, (total ? total : 1) * sizeof(uint32_t), &d_idx));
    if (total) PHK_TRY(phk_copy_to_device(ctx, d_idx, set_rows, total * sizeof(uint32_t)));
    for (uint64_t i = 0; i < n_sets; ++i) {
        const uint64_t ns = s->n[i];
        if (ns == s->N) {
            s->set.push_back(s->src);
            continue;
        }
        uint32_t *dst = (uint32_t *)((char *)s->rows.ptr + at[i]);
        const uint64_t blocks = std::min<uint64_t>(phk_div_up(ns * s->D, 256), 1u << 20);
        PHK_LAUNCH(ctx, "phk_mixsweep_gather_kernel",
                   phk_mixsweep_gather_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(
                       s->src, s->D, (const uint32_t *)d_idx + set_offsets[i], ns, dst));
        s->set.push_back(dst);
    }
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // the caller's index list and the workspace are free again
    return PHK_OK;
}

static int sweep_create(phk_ctx *ctx, const char *fname, const uint32_t *counts, const phk_batch *b, uint64_t N, uint64_t D,
                        const uint32_t *set_rows, const uint64_t *set_offsets, uint64_t n_sets, phk_mix_sweep **out) {
    PHK_REQUIRE(out, "%s: NULL out", fname);
    *out = nullptr;
    PHK_REQUIRE(N >= 1 && N < (1ull << 32), "%s: %llu rows (1 to 2^32 - 1)", fname, (unsigned long long)N);
    PHK_REQUIRE(D > 0 && D < (1ull << 32), "%s: %llu columns", fname, (unsigned long long)D);
    phk_mix_sweep *s = new phk_mix_sweep();
    s->N = N, s->D = D;
    int rc = PHK_OK;
    if (b) {
        s->src = b->d_counts;
    } else {
        rc = s->own.alloc(fname, "count rows", N * D * sizeof(uint32_t));
        if (rc == PHK_OK) rc = phk_copy_to_device(ctx, s->own.ptr, counts, N * D * sizeof(uint32_t));
        s->src = s->own.as<uint32_t>();
    }
    if (rc == PHK_OK) rc = sweep_sets(ctx, fname, s, set_rows, set_offsets, n_sets);
    if (rc != PHK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        delete s;
        return rc;
    }
    *out = s;
    return PHK_OK;
}

extern "C" int phk_mix_sweep_create(phk_ctx *ctx, const uint32_t *counts, uint64_t N, uint64_t D, const uint32_t *set_rows,
                                    const uint64_t *set_offsets, uint64_t n_sets, phk_mix_sweep **out) {
    PHK_ENTER(ctx, "phk_mix_sweep_create");
    PHK_REQUIRE(counts, "phk_mix_sweep_create: NULL counts");
    return sweep_create(ctx, "phk_mix_sweep_create", counts, nullptr, N, D, set_rows, set_offsets, n_sets, out);
}

extern "C" int phk_batch_mix_sweep_create(phk_ctx *ctx, const phk_batch *b, const uint32_t *set_rows,
                                          const uint64_t *set_offsets, uint64_t n_sets, phk_mix_sweep **out) {
    PHK_ENTER(ctx, "phk_batch_mix_sweep_create");
    PHK_REQUIRE(b, "phk_batch_mix_sweep_create: NULL batch");
    return sweep_create(ctx, "phk_batch_mix_sweep_create", nullptr, b, b->n, b->D, set_rows, set_offsets, n_sets, out);
}

extern "C" int phk_mix_sweep_destroy(phk_ctx *ctx, phk_mix_sweep *s) {
    if (!s) return PHK_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete s;
    return PHK_OK;
}

// ---- a step --------------------------------------------------------------------------------------------------------------
// The group's buffers of one job: R, and for an expectation its partial vectors and the two fold buffers.
static uint64_t sweep_job_bytes(uint64_t n, uint64_t Kp, uint64_t E, bool expect) {
    const uint64_t blocks = phk_div_up(n, MIX_RB);
    return n * Kp * 8 + (expect ? (blocks + 2 * phk_div_up(blocks, 256)) * E * 8 : 0);
}

extern "C" int phk_mix_sweep_step(phk_ctx *ctx, const phk_mix_sweep *s, const uint32_t *job_set, const uint32_t *job_K,
                                  uint64_t n_jobs, const double *log_profiles, const double *log_weights, int expect, int rows,
                                  uint64_t budget_bytes, double *out) {
    const char *fname = "phk_mix_sweep_step";
    PHK_ENTER(ctx, "phk_mix_sweep_step");
    PHK_REQUIRE(s, "%s: NULL sweep", fname);
    PHK_REQUIRE(expect || rows, "%s: neither the expectation nor the rows asked for", fname);
    if (n_jobs == 0) return PHK_OK;
    PHK_REQUIRE(job_set && job_K && log_profiles && log_weights && out, "%s: NULL pointer", fname);
    PHK_REQUIRE(n_jobs < (1ull << 32), "%s: 2^32 jobs or more", fname);
    const uint64_t D = s->D, budget = budget_bytes ? budget_bytes : 512ull << 20;
    const double inf = __builtin_inf();

    // the jobs: checks, the offsets of their tables, results and rows
    std::vector<MixSweepJob> jobs(n_jobs);
    uint64_t n_logp = 0, n_logw = 0, n_res = 0, n_ll = 0;
    for (uint64_t j = 0; j < n_jobs; ++j) {
        PHK_REQUIRE(job_set[j] < s->set.size(), "%s: job %llu names row set %u of %llu", fname, (unsigned long long)j, job_set[j],
                    (unsigned long long)s->set.size());
        const uint64_t K = job_K[j];
        PHK_REQUIRE(K >= 1 && K <= MIX_KMAX, "%s: job %llu has %llu components (1 to %d)", fname, (unsigned long long)j,
                    (unsigned long long)K, MIX_KMAX);
        const double *w = log_weights + (n_logp / D);   // (the weights lie as the profiles' rows do: sum of K so far)
        bool any = false;
        for (uint64_t k = 0; k < K; ++k) {
            if (w[k] != w[k] || w[k] == inf) {
                phk_set_error("%s: job %llu: log weight %llu is %g", fname, (unsigned long long)j, (unsigned long long)k, w[k]);
                return PHK_ERR_NAN;
            }
            any = any || w[k] > -inf;
        }
        if (!phk_rows_finite(log_profiles + n_logp, K * D)) {
            phk_set_error("%s: job %llu: the log profiles hold a value that is not finite (a zero profile entry?)", fname,
                          (unsigned long long)j);
            return PHK_ERR_NAN;
        }
        PHK_REQUIRE(any, "%s: job %llu: every component has weight 0", fname, (unsigned long long)j);
        MixSweepJob &d = jobs[j];
        d.C = s->set[job_set[j]], d.n = s->n[job_set[j]];
        d.K = (uint32_t)K, d.Kp = (uint32_t)(phk_div_up(K, MIX_CT) * MIX_CT), d.E = K * D + K + 1;
        d.logp = n_logp, d.logw = n_logw, d.ll = n_ll, d.R = 0, d.part = 0;
        n_logp += K * D, n_logw += d.Kp, n_ll += d.n;
        if (expect) n_res += d.E;
    }

    // the groups: consecutive jobs whose buffers stay under the budget (a job above it goes alone)
    struct Group {
        uint64_t j0, j1, bytes, tiles0, tiles1, exp0, exp1;
        std::vector<std::pair<uint64_t, uint64_t>> levels;   // [first, last) of the fold descriptors, level by level
    };
    std::vector<Group> groups;
    uint64_t group_bytes = 0;
    for (uint64_t j = 0; j < n_jobs; ++j) {
        const uint64_t b = sweep_job_bytes(jobs[j].n, jobs[j].Kp, jobs[j].E, expect);
        if (groups.empty() || groups.back().bytes + b > budget) groups.push_back(Group{j, j, 0, 0, 0, 0, 0, {}});
        groups.back().bytes += b, groups.back().j1 = j + 1;
        group_bytes = std::max(group_bytes, groups.back().bytes);
    }

    // the call's workspace: [results | rows] as the host takes them back, the tables, the group's buffers
    PhkLayout lay;
    (void)lay.take((n_res + n_ll) * 8);   // at the workspace's start
    const uint64_t o_logp = lay.take(n_logp * 8), o_logw = lay.take(n_logw * 8), o_grp = lay.take(group_bytes);
    const uint64_t w_ll = n_res, w_grp = o_grp / 8;   // in doubles from the workspace's start

    // the descriptors of every group: buffers are laid out per group, the same place for every group
    std::vector<MixSweepTile> tiles, etiles;
    std::vector<MixSweepFold> folds;
    uint64_t res_at = 0;
    for (Group &g : groups) {
        uint64_t at = w_grp;
        for (uint64_t j = g.j0; j < g.j1; ++j) jobs[j].R = at - w_grp, at += jobs[j].n * jobs[j].Kp;
        const uint64_t w_part = at;
        if (expect)
            for (uint64_t j = g.j0; j < g.j1; ++j)
                jobs[j].part = at - w_part, at += phk_div_up(jobs[j].n, MIX_RB) * jobs[j].E;
        g.tiles0 = tiles.size(), g.exp0 = etiles.size();
        for (uint64_t j = g.j0; j < g.j1; ++j) {
            const MixSweepJob &d = jobs[j];
            for (uint64_t t = 0; t < phk_div_up(d.n, GT_QB); ++t) tiles.push_back(MixSweepTile{(uint32_t)j, (uint32_t)t, 0, 0});
            if (!expect) continue;
            for (uint64_t b = 0; b < phk_div_up(d.n, MIX_RB); ++b)
                for (uint64_t y = 0; y < phk_div_up(D, GT_WAVES * MIX_CT); ++y)
                    for (uint32_t z = 0; z < d.Kp / MIX_CT; ++z)
                        etiles.push_back(MixSweepTile{(uint32_t)j, (uint32_t)b, (uint32_t)y, z});
        }
        g.tiles1 = tiles.size(), g.exp1 = etiles.size();
        if (!expect) continue;
        // the fold: a job's level l reads m vectors and writes ceil(m / 256); the last one goes to the job's result
        struct Live { uint64_t j, in, m, f[2], res; };
        std::vector<Live> live;
        for (uint64_t j = g.j0; j < g.j1; ++j) {
            const uint64_t nf = phk_div_up(phk_div_up(jobs[j].n, MIX_RB), 256) * jobs[j].E;
            live.push_back(Live{j, w_part + jobs[j].part, phk_div_up(jobs[j].n, MIX_RB), {at, at + nf}, res_at});
            at += 2 * nf, res_at += jobs[j].E;
        }
        for (int level = 0; !live.empty(); ++level) {
            const uint64_t first = folds.size();
            std::vector<Live> next;
            for (Live &v : live) {
                const uint64_t E = jobs[v.j].E, blocks = phk_div_up(v.m, 256);
                const uint64_t o = blocks == 1 ? v.res : v.f[level & 1];
                for (uint64_t vb = 0; vb < blocks; ++vb)
                    for (uint64_t ex = 0; ex < phk_div_up(E, 256); ++ex)
                        folds.push_back(MixSweepFold{v.in, o + vb * E, v.m, E, (uint32_t)ex, (uint32_t)vb});
                if (blocks > 1) v.in = o, v.m = blocks, next.push_back(v);
            }
            g.levels.push_back({first, folds.size()});
            live.swap(next);
        }
    }
    PHK_REQUIRE(tiles.size() < (1ull << 31) && etiles.size() < (1ull << 31) && folds.size() < (1ull << 31),
                "%s: more than 2^31 workgroups in one launch", fname);
    const uint64_t o_jobs = lay.take(jobs.size() * sizeof(MixSweepJob)), o_tiles = lay.take(tiles.size() * sizeof(MixSweepTile)),
                   o_etiles = lay.take(etiles.size() * sizeof(MixSweepTile)), o_folds = lay.take(folds.size() * sizeof(MixSweepFold));

    void *ws;
    PHK_TRY(phk_ws(ctx, WS_MIX, lay.bytes, &ws));
    char *w8 = (char *)ws;
    double *d_ws = (double *)ws, *d_logp = (double *)(w8 + o_logp), *d_logw = (double *)(w8 + o_logw);
    std::vector<double> w(n_logw, -inf);
    for (uint64_t j = 0; j < n_jobs; ++j)
        std::copy(log_weights + jobs[j].logp / D, log_weights + jobs[j].logp / D + jobs[j].K, w.begin() + jobs[j].logw);
    PHK_TRY(phk_copy_to_device(ctx, d_logp, log_profiles, n_logp * 8));
    PHK_TRY(phk_copy_to_device(ctx, d_logw, w.data(), n_logw * 8));
    PHK_TRY(phk_copy_to_device(ctx, w8 + o_jobs, jobs.data(), jobs.size() * sizeof(MixSweepJob)));
    PHK_TRY(phk_copy_to_device(ctx, w8 + o_tiles, tiles.data(), tiles.size() * sizeof(MixSweepTile)));
    if (expect) {
        PHK_TRY(phk_copy_to_device(ctx, w8 + o_etiles, etiles.data(), etiles.size() * sizeof(MixSweepTile)));
        PHK_TRY(phk_copy_to_device(ctx, w8 + o_folds, folds.data(), folds.size() * sizeof(MixSweepFold)));
    }
    const MixSweepJob *d_jobs = (const MixSweepJob *)(w8 + o_jobs);
    const MixSweepTile *d_tiles = (const MixSweepTile *)(w8 + o_tiles), *d_etiles = (const MixSweepTile *)(w8 + o_etiles);
    const MixSweepFold *d_folds = (const MixSweepFold *)(w8 + o_folds);
    double *d_R = d_ws + w_grp, *d_ll = d_ws + w_ll;
    const bool full = D % GT_KC == 0, vec = D % 4 == 0;
    const dim3 blk(GT_WAVES * 64);
    for (const Group &g : groups) {
        uint64_t n_R = 0;
        for (uint64_t j = g.j0; j < g.j1; ++j) n_R += jobs[j].n * jobs[j].Kp;
        double *d_part = d_R + n_R;
        const dim3 g1((unsigned)(g.tiles1 - g.tiles0));
        if (full) {
            PHK_LAUNCH(ctx, "phk_mixsweep_resp_kernel", phk_mixsweep_resp_kernel<true><<<g1, blk, 0, ctx->stream>>>(
                                                            d_jobs, d_tiles + g.tiles0, D, d_logp, d_logw, d_R, d_ll));
        } else {
            PHK_LAUNCH(ctx, "phk_mixsweep_resp_kernel", phk_mixsweep_resp_kernel<false><<<g1, blk, 0, ctx->stream>>>(
                                                            d_jobs, d_tiles + g.tiles0, D, d_logp, d_logw, d_R, d_ll));
        }
        if (!expect) continue;
        const dim3 g2((unsigned)(g.exp1 - g.exp0));
        if (vec) {
            PHK_LAUNCH(ctx, "phk_mixsweep_expect_kernel", phk_mixsweep_expect_kernel<true><<<g2, blk, 0, ctx->stream>>>(
                                                              d_jobs, d_etiles + g.exp0, D, d_R, d_ll, d_part));
        } else {
            PHK_LAUNCH(ctx, "phk_mixsweep_expect_kernel", phk_mixsweep_expect_kernel<false><<<g2, blk, 0, ctx->stream>>>(
                                                              d_jobs, d_etiles + g.exp0, D, d_R, d_ll, d_part));
        }
        for (const auto &lv : g.levels)
            PHK_LAUNCH(ctx, "phk_mixsweep_fold_kernel",
                       phk_mixsweep_fold_kernel<<<dim3((unsigned)(lv.second - lv.first)), dim3(256), 0, ctx->stream>>>(
                           d_folds + lv.first, d_ws));
    }
    // one copy back: every job's (T, N_k, L) and then, where asked for, every job's l_i; without them the rows alone
    if (rows) return phk_copy_to_host(ctx, out, d_ws, (n_res + n_ll) * 8);
    return phk_copy_to_host(ctx, out, d_ws, n_res * 8);
}
