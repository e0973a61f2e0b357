// score_mfma.hip -- the fast scoring path's model and driver (k = 4 .. 6: D = 256 .. 4096):
//
//   1. a proposal pass (score_f16.hip, score_i8.hip): an MFMA "distance GEMM" of the centred count rows against the centred
//      reference rows + centroids with a fused running top-4 per (query, column segment, half-list) kept in registers --
//      nothing of the N x (M + C) product ever reaches memory.  This is the dense contraction behind scikit-learn's
//      brute-force k-NN (scripts/learning.py:127) and behind the nearest-centroid search (scripts/learning.py:59-66).
//   2. the decision stage (score_decide.hip, score_rerank.hip): per query, certify the candidate order against a rigorous
//      error bound; where certified take the vote from the labels, otherwise (and always for the two nearest-centroid
//      distances the proximity metric needs, scripts/phamer.py:198-210) recompute direct-difference float64 distances for
//      the candidates.  A query whose candidate set cannot be certified to contain the true neighbours is queued for
//   3. the exact float64 brute force over every column (score_fallback.hip).
//
// So the MFMA pass only ever PROPOSES candidates; every emitted number is decided by float64 arithmetic of the same form as
// the reference's (direct differences), or by a certified ordering.
//
// Ranking quantity.  With mu = mean train row, r' = r - mu, q' = q - mu (distances are translation invariant) the proposal
// maximises  v = q'.r' - |r'|^2/2  = (|q'|^2 - |q-r|^2)/2; the -|r'|^2/2 term rides through the MFMA as one more k-step
// (score_f16.hip: phk_bias_pieces).
//
// This file: the host-side model build (centring, norms, the float64 copies the decision stage reads) and the driver
// phk_score_fast: the route of a call (ScoreRoute), its workspaces (ScoreWs), the error models that fill the parameter blocks
// (score_decide.h), and the stages that enqueue the launch chain of a batch.
#include <stdlib.h>

#include <cmath>
#include <vector>

#include "score_decide.h"

__global__ void phk_rowsum_kernel(const uint32_t *__restrict__ counts, uint64_t N, uint64_t D, uint32_t *__restrict__ out);   // score_f16.hip

bool phk_fast_supports_dim(uint64_t D);

// Column mask -> the train segment's candidate lists.  A masked column carries padding terms, so its value (~ -1e30) loses
// to every unmasked one -- but it keeps its real index, and where fewer unmasked columns than list slots reach a half-list
// it fills the slot.  The decision stages compute exact distances for every slot whose index is < M: such a column would
// be a candidate again (a held-out row, its own nearest neighbour).  It is turned into an empty slot, as the proposal
// kernels write them.  (Segment 0 is the first 2 CAND N entries of a list set.)
__global__ __launch_bounds__(256) void phk_mask_lists_kernel(float *__restrict__ cv, uint32_t *__restrict__ ci, uint64_t n,
                                                             uint64_t M, const uint8_t *__restrict__ mask) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t c = ci[t];
    if (c < M && mask[c]) {
        ci[t] = 0xFFFFFFFFu;
        cv[t] = -3.0e38f;
    }
}
static int phk_mask_lists(phk_ctx *ctx, const phk_model *m, float *cv, uint32_t *ci, uint64_t N) {
    const uint64_t n = 2ull * CAND * N;
    if (!m->has_mask || n == 0) return PHK_OK;
    PHK_LAUNCH(ctx, "phk_mask_lists_kernel",
               phk_mask_lists_kernel<<<dim3((unsigned)phk_div_up(n, 256)), dim3(256), 0, ctx->stream>>>(cv, ci, n, m->M, m->d_col_mask));
    return PHK_OK;
}

// ------------------------------------------------------------------------------------
// model build (host): centre, round to fp32, fragment-order, upload
// ------------------------------------------------------------------------------------
int phk_model_build_fast(phk_ctx *ctx, phk_model *m, const double *pos, const double *neg,
                         const double *cpos, const double *cneg) {
    (void)ctx;
    m->fast = false;
    const uint64_t D = m->D;
    // MFMA proposal paths: D a multiple of 256 up to 4096 (k = 4, 5, 6) and up to 3 neighbours
    if (!phk_fast_supports_dim(D) || m->kn > CAND - 1) return PHK_OK;  // exact path serves other shapes
    if (m->M >= (1ull << 31)) return PHK_OK;
    // the MFMA path's last resort (phk_fallback_partial_kernel) keeps one chunk of float64 distances + the query in LDS
    if (((m->M + m->n_cpos + m->n_cneg + FB_CHUNKS - 1) / FB_CHUNKS + D) * sizeof(double) > FB_LDS_MAX) return PHK_OK;
    std::vector<double> mu(D, 0.0);
    for (uint64_t r = 0; r < m->n_pos; ++r)
        for (uint64_t d = 0; d < D; ++d) mu[d] += pos[r * D + d];
    for (uint64_t r = 0; r < m->n_neg; ++r)
        for (uint64_t d = 0; d < D; ++d) mu[d] += neg[r * D + d];
    double mu2 = 0.0;
    std::vector<float> mu32(D);
    for (uint64_t d = 0; d < D; ++d) {
        mu[d] /= (double)m->M;
        if (!(mu[d] == mu[d]) || std::isinf(mu[d])) return PHK_OK;  // NaN/inf train data: exact path
        mu32[d] = (float)mu[d];
        mu[d] = (double)mu32[d];  // centre by the fp32-representable vector: q' is then formed alike on both paths
        mu2 += mu[d] * mu[d];
    }
    m->n_rblk_ref = (uint32_t)phk_div_up(m->M, 32);
    m->n_rblk_pos = (uint32_t)phk_div_up(m->n_cpos, 32);
    m->n_rblk_neg = (uint32_t)phk_div_up(m->n_cneg, 32);
    double max_norm = 0.0;
    std::vector<double> colnorm(m->M + m->n_cpos + m->n_cneg + 1, 0.0);  // |r'| of every real column
    {   // |r'| of every column as the float32-rounded centred row gives it
        auto norms = [&](const double *rows, uint64_t n, double *out) {
            phk_parallel_for(n, [&](uint64_t r) {
                double s2 = 0.0;
                for (uint64_t d = 0; d < D; ++d) {
                    const double v = (double)(float)(rows[r * D + d] - mu[d]);
                    s2 += v * v;
                }
                out[r] = std::sqrt(s2);
            });
            for (uint64_t r = 0; r < n; ++r)
                if (out[r] > max_norm) max_norm = out[r];
        };
        norms(pos, m->n_pos, colnorm.data());
        norms(neg, m->n_neg, colnorm.data() + m->n_pos);
        if (m->n_cpos) norms(cpos, m->n_cpos, colnorm.data() + m->M);
        if (m->n_cneg) norms(cneg, m->n_cneg, colnorm.data() + m->M + m->n_cpos);
    }
    if (!(max_norm == max_norm) || std::isinf(max_norm)) return PHK_OK;
    if (hipMalloc(&m->d_mu32, D * sizeof(float)) != hipSuccess) return PHK_ERR_NOMEM;
    if (hipMalloc(&m->d_mu64, D * sizeof(double)) != hipSuccess) return PHK_ERR_NOMEM;
    if (hipMalloc(&m->d_colnorm, colnorm.size() * sizeof(double)) != hipSuccess) return PHK_ERR_NOMEM;
    if (hipMemcpy(m->d_colnorm, colnorm.data(), colnorm.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->d_mu32, mu32.data(), D * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->d_mu64, mu.data(), D * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return PHK_ERR_HIP;
    PHK_TRY(phk_model_build_f16(m, pos, neg, cpos, cneg, mu.data(), colnorm.data()));
    PHK_TRY(phk_model_build_i8(m, pos, neg, cpos, cneg, mu.data(), colnorm.data()));
    m->h_mu = mu;
    m->max_colnorm_train = 0.0;
    for (uint64_t c = 0; c < m->M; ++c)
        if (colnorm[c] > m->max_colnorm_train) m->max_colnorm_train = colnorm[c];
    m->max_colnorm = max_norm;
    m->mu_norm = std::sqrt(mu2);
    {
        double t2 = 0.0;
        for (uint64_t d = 0; d < D; ++d) t2 += (mu[d] - 1.0 / (double)D) * (mu[d] - 1.0 / (double)D);
        m->mu_tilde_norm = std::sqrt(t2) * (1.0 + 1.0e-12);
    }
    m->fast = true;
    return PHK_OK;
}

template <typename T>
static void free_null(T *&p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
void phk_model_free_fast(phk_model *m) {
    free_null(m->d_colnorm); free_null(m->d_Af16); free_null(m->d_A8); free_null(m->d_A8h); free_null(m->d_L8);
    free_null(m->d_T8); free_null(m->d_T8h); free_null(m->d_term_orig); free_null(m->d_col_mask); free_null(m->d_betah16);
    free_null(m->d_Af16h); free_null(m->d_lo16); free_null(m->d_cn16); free_null(m->d_beta16); free_null(m->d_mu32);
    free_null(m->d_mu64);
}

// ------------------------------------------------------------------------------------
// driver: phk_score_fast = route, workspace, loop over batches, join
// ------------------------------------------------------------------------------------
bool phk_fast_supports_dim(uint64_t D) { return D == 256 || D == 512 || D == 1024 || D == 2048 || D == 4096; }

// ---- the route: what is fixed for a call ----
// The first pass of a batch, by the rows, the dimension, the model and the "proposal" option (PhkProposal, phk_common.h):
//
//   flavour          rows     D      option        sweep                                   a test that takes it (tests/)
//   FIRST_HI_K4      counts   256    "" hi cxf i83 phk_launch_proposal_f16h, high parts    test_gpu_score.py: every k = 4 count-rows test
//   FIRST_SPLIT_F16  float64  any    any           phk_launch_proposal_f16 / _f16_general, test_model_score_k4_golden, test_highdim_golden
//                    counts   any    f16             split query                           test_fast_and_exact_gpu_paths_agree_on_a_larger_batch
//   FIRST_I8_TWO     counts   > 256  ""            phk_launch_proposal_i8_general, 2 parts test_general_dim_mfma_path_agrees_with_exact_path
//   FIRST_I8_THREE   counts   > 256  i83           ... all 3 parts in the sweep            test_two_digit_int8_sweep_adversarial_queries_and_batch_split
//   FIRST_CX_F16     counts   > 256  cxf           _f16_general, count-exact               test_general_dim_mfma_path_agrees_with_exact_path
//   FIRST_HI_GEN     counts   > 256  hi            _f16_general, high parts                test_gpu_fold_state.py
//
// A model without the operand a flavour needs moves along the table: the int8 sweeps stand down to FIRST_CX_F16 while the
// centroids were replaced or a column mask is set (their records are not updated by the cross-validation service), a model
// without low parts takes the default at general D, and a k = 4 model without high parts FIRST_SPLIT_F16.  Any other option
// value means "".
enum PhkFirstPass { FIRST_SPLIT_F16, FIRST_HI_K4, FIRST_CX_F16, FIRST_HI_GEN, FIRST_I8_TWO, FIRST_I8_THREE };

struct ScoreRoute {
    const phk_model *m;
    int method;
    bool counts;          // the rows are uint32 counts (else normalised float64)
    PhkFirstPass first;
    // Second chance (FIRST_HI_K4): what the first pass cannot decide -- rows holding a count above 2048, which the fp16 count
    // operand cannot carry, and queries whose lists fail certification -- goes through the split-query sweep, addressed
    // through the first pass's queue, with list sets of its own; only what that cannot certify either is brute-forced.
    bool second;
    bool tail_aside;      // multi-batch calls at k = 4: a batch's tail on the second stream, beside the NEXT batch's sweep (stage_tail)
    uint64_t BATCH;       // queries per batch: bounds the candidate (200 B/query), fallback (1 KiB/query) and split-query workspaces
    uint64_t nb_max;      // the largest batch of this call
    uint64_t cap2;        // queries a second-chance sweep takes
    uint64_t gen_sets;    // general D: list sets = the column groups of the f16 sweep's 2-D launch
    uint32_t i8_groups;   // ... and those of the int8 sweep
    bool use_i8() const { return first == FIRST_I8_TWO || first == FIRST_I8_THREE; }
    bool count_exact() const { return first != FIRST_SPLIT_F16; }   // the integer counts are the MFMA operand
    int src_kind() const { return counts ? 0 : 1; }                 // as the launchers take it
};

static ScoreRoute score_route(const PhkKnobs &knobs, const phk_model *m, bool counts, int method, uint64_t N) {
    const uint64_t D = m->D;
    const PhkProposal prop = knobs.proposal;
    ScoreRoute r;
    r.m = m; r.method = method; r.counts = counts;
    if (!counts || prop == PHK_PROP_F16 || (D == FAST_D && !m->d_Af16h)) r.first = FIRST_SPLIT_F16;
    else if (D == FAST_D) r.first = FIRST_HI_K4;
    // general D, high parts: opt-in -- on nearly equidistant references its wide windows lose in the tail what the sweep saves
    // (20 % of config 4's queries brute-forced, profiles/r02/README.md)
    else if (prop == PHK_PROP_HI && m->d_lo16 && m->d_betah16) r.first = FIRST_HI_GEN;
    // the int8 sweep (3 exact-integer MFMAs per 32 dimensions where the f16 count-exact kernel issues 4); by default with the H and
    // M digits in the sweep and the L product added by the decision kernel to the window's members
    else if (prop != PHK_PROP_CXF && m->d_A8 && !m->bf_stale)
        r.first = (prop != PHK_PROP_I83 && m->d_A8h && m->d_L8) ? FIRST_I8_TWO : FIRST_I8_THREE;
    else r.first = FIRST_CX_F16;
    r.second = r.first == FIRST_HI_K4;
    // (the split-query workspace bounds a batch: 4 D bytes per query for the f16 sweeps, D for the int8 sweep)
    r.BATCH = 1ull << 20;
    while (r.BATCH > 4096 && r.BATCH * D * (r.use_i8() ? 1 : 4) > (2ull << 30)) r.BATCH >>= 1;
    if (knobs.score_batch) r.BATCH = knobs.score_batch < 64 ? 64 : knobs.score_batch;
    r.nb_max = N < r.BATCH ? N : r.BATCH;
    r.cap2 = r.second ? (r.nb_max / 8 > 4096 ? r.nb_max / 8 : (r.nb_max < 4096 ? r.nb_max : 4096)) : 0;
    r.gen_sets = knobs.gen_groups > 0 ? (uint64_t)(knobs.gen_groups < 16 ? knobs.gen_groups : 16) : (D >= 2048 ? PHK_GEN_GROUPS : 1);
    // (the int8 sweep's optimum at D >= 2048 is 2 groups -- configs[4]: 40.1 / 38.5 / 42.3 / 40.3 ms with 1 / 2 / 3 / 4)
    r.i8_groups = knobs.gen_groups > 0 ? (uint32_t)r.gen_sets : (r.gen_sets > 2 ? 2u : (uint32_t)r.gen_sets);
    r.tail_aside = r.second && N > r.BATCH && knobs.tail_aside;
    return r;
}

// ---- the workspaces of a call, carved once ----
// candidate lists, structure of arrays (score_lists.h: cand_at / candu_at)
struct ScoreLists {
    float *v;
    uint32_t *i;
    float *u;
};
static ScoreLists score_lists_at(char *base, uint64_t per_list) {
    ScoreLists l;
    l.v = (float *)base;
    l.i = (uint32_t *)(base + per_list * sizeof(float4));
    l.u = (float *)(base + per_list * (sizeof(float4) + sizeof(uint4)));
    return l;
}
// The control words of the batches of one parity (WS_SCTL).  Counter words: [0] first-pass queue length, [1] exact-distance
// decisions, [2] decide kernel's hand-over count, [3] brute-force queue length after the second chance, [4] its
// exact-distance decisions, [5], [6] lengths of the general-D hand-over queues, [8..11] why the high-parts-only decision
// stage passed a query on (window wider than the refined set, window reaching past the lists, refined values too close,
// centroid leader not certified), [15] the merge kernel's ticket.  (The call's totals, WS_SCTL's first 32 words: brute-forced
// queries, exact-distance decisions, second-chance queries, the four reasons, the two general-D second passes.)
struct ScoreSet {
    uint32_t *counters, *stripes;              // 32 counter words; the striped statistics words (RerankParams::stripes)
    uint32_t *fb_list, *slow_list, *fb2_list;  // brute-force queue, the decision kernels' hand-over lists, the queue after the second chance
};
struct ScoreWs {
    ScoreLists first, second;       // WS_CAND: gen_sets list sets set_bytes apart; PHK_SECOND_SPLITS sets set2_bytes apart
    uint64_t set_bytes, set2_bytes;
    float *ca;                      // general D: the sweeps' observed running sums (RerankParams::cand_a), else null
    double *pend;                   // general D with centroids: the decision kernel's pending centroid distances, else null
    uint32_t *totals;               // WS_SCTL: the call's totals (read by phk_score_stats), then ...
    ScoreSet set[2];                // ... what alternate batches use
    void *rec;                      // WS_QF32: the brute force's partial records, nb_max * FB_CHUNKS of them
    uint32_t *q2_wide, *q2_big;     // WS_QUEUE (int8 first pass): the two hand-over queues
    size_t fb_lds;                  // dynamic LDS of the k = 4 brute force
};

// WS_SCTL: [32 words: the call's totals] then TWO sets of {32 counter words, the striped statistics words, the three query
// lists}, used by alternate batches: batch b's tail (second stream) still reads set b & 1 while batch b + 1's first pass
// fills the other.  Nothing here is memset per call or per batch: the last workgroup of a batch's last kernel
// (phk_fallback_merge_kernel) zeroes the set's counters and stripes after everybody has read them; a memset happens once per
// allocation and after a call that failed half way.  The words that must read zero sit at FIXED offsets in front -- totals,
// then each set's counters and stripes -- and the lists, whose size follows the batch, behind them: a call with another
// batch size finds the same words zeroed.  The totals of THIS call start from zero: the count planner's kernel zeroed them
// (link, see PhkStepLink), or a memset does.
// (WS_QF32 and the brute force's LDS check sit between the two memsets because the order of allocations and memsets is
// the parent call chain's: which ws_fail index hits which slot, and what a failed call has already enqueued, depend on it.)
static int score_control_words(phk_ctx *ctx, const ScoreRoute &r, const PhkStepLink *link, ScoreWs &ws) {
    const uint64_t ctl_words = 32 + (uint64_t)PHK_STRIPES * 32, list_words = 3 * r.nb_max + 64 * PHK_SUB_LISTS;
    PhkLayout ctl;
    ctl.align = sizeof(uint32_t);
    const uint64_t o_totals = ctl.take(32 * sizeof(uint32_t));
    const uint64_t o_ctl[2] = {ctl.take(ctl_words * sizeof(uint32_t)), ctl.take(ctl_words * sizeof(uint32_t))};
    const uint64_t zero_bytes = ctl.bytes;
    const uint64_t o_lists[2] = {ctl.take(list_words * sizeof(uint32_t)), ctl.take(list_words * sizeof(uint32_t))};
    void *fb;
    PHK_TRY(phk_ws(ctx, WS_SCTL, ctl.bytes, &fb));
    ws.totals = (uint32_t *)((char *)fb + o_totals);
    for (int par = 0; par < 2; ++par) {
        ScoreSet &s = ws.set[par];
        s.counters = (uint32_t *)((char *)fb + o_ctl[par]);
        s.stripes = s.counters + 32;
        s.fb_list = (uint32_t *)((char *)fb + o_lists[par]);
        s.slow_list = s.fb_list + r.nb_max;
        s.fb2_list = s.slow_list + r.nb_max + 64 * PHK_SUB_LISTS;
    }
    bool totals_zeroed = link && link->zeroed(ws.totals);
    if (ctx->score_ctl_dirty || ctx->score_ctl_gen != ctx->ws[WS_SCTL].gen) {
        PHK_HIP(hipMemsetAsync(fb, 0, zero_bytes, ctx->stream));
        ctx->score_ctl_gen = ctx->ws[WS_SCTL].gen;
        totals_zeroed = true;
    }
    ctx->score_ctl_dirty = true;   // (cleared at the end of a call that launched everything)
    PHK_TRY(phk_ws(ctx, WS_QF32, r.nb_max * FB_CHUNKS * sizeof(FbRecord), &ws.rec));
    const uint64_t ncols = r.m->M + r.m->n_cpos + r.m->n_cneg;
    ws.fb_lds = ((ncols + FB_CHUNKS - 1) / FB_CHUNKS + r.m->D) * sizeof(double);
    PHK_REQUIRE(ws.fb_lds <= FB_LDS_MAX, "phk_score: %llu columns exceed the fallback kernel's LDS", (unsigned long long)ncols);  // phk_model_build_fast keeps such models off this path
    if (!totals_zeroed) PHK_HIP(hipMemsetAsync(ws.totals, 0, 32 * sizeof(uint32_t), ctx->stream));
    return PHK_OK;
}

static int score_workspace(phk_ctx *ctx, const ScoreRoute &r, const PhkStepLink *link, ScoreWs &ws) {
    const uint64_t D = r.m->D;
    // WS_CAND: the first pass's list sets, their running sums, the second chance's list sets (its sweep takes the reference in
    // PHK_SECOND_SPLITS column parts, each with a list set of its own), the pending centroid distances.  (Every piece is a
    // multiple of 8 bytes, the widest element: nothing is padded.)
    const uint64_t per_list = r.nb_max * NSEG * 2, per_list2 = r.cap2 * NSEG * 2;
    const uint64_t list_bytes = sizeof(float4) + sizeof(uint4) + sizeof(float);
    ws.set_bytes = per_list * list_bytes;
    ws.set2_bytes = per_list2 * list_bytes;
    const uint64_t ca_bytes = D != FAST_D ? r.gen_sets * 2 * r.nb_max * sizeof(float) : 0;
    const uint64_t pend_bytes = (D != FAST_D && (r.method & PHK_METHOD_KMEANS)) ? r.nb_max * 2 * sizeof(double) : 0;
    PhkLayout cand;
    cand.align = sizeof(double);
    const uint64_t o_first = cand.take(r.gen_sets * ws.set_bytes), o_ca = cand.take(ca_bytes);
    const uint64_t o_second = cand.take(PHK_SECOND_SPLITS * ws.set2_bytes), o_pend = cand.take(pend_bytes);
    void *cv;
    PHK_TRY(phk_ws(ctx, WS_CAND, cand.bytes, &cv));
    ws.first = score_lists_at((char *)cv + o_first, per_list);
    ws.second = score_lists_at((char *)cv + o_second, per_list2);
    ws.ca = ca_bytes ? (float *)((char *)cv + o_ca) : nullptr;
    ws.pend = pend_bytes ? (double *)((char *)cv + o_pend) : nullptr;
    PHK_TRY(score_control_words(ctx, r, link, ws));
    ws.q2_wide = ws.q2_big = nullptr;
    if (r.use_i8()) {   // the two queues its decision kernel hands rows on through (decide_second_passes)
        void *q2;
        PHK_TRY(phk_ws(ctx, WS_QUEUE, 2 * r.nb_max * sizeof(uint32_t), &q2));
        ws.q2_wide = (uint32_t *)q2;
        ws.q2_big = ws.q2_wide + r.nb_max;
    }
    return PHK_OK;
}

// ---- the error models of the proposal passes (ErrBound in score_decide.h evaluates them) ----
// These doubles are kernel arguments: coefficients and the order of the operations are part of the result.
static double model_rho(const phk_model &m) { return m.rho_inf > 0.0 && m.rho_inf < 1.0 ? m.rho_inf : 1.0; }   // max_j |r~'_j|_inf / |r'_j|

// split f16:  eps(R) = u R (6 A + cQ Q + 18 n rho I + cP P + (6 + x) R) + c_abs (R + P)
// f16 MFMA chains: n instructions, each charged u (PHK_MFMA_ACC |x| |y| + PHK_MFMA_PROD |x|_inf |y|_inf).
// n = 3D/16 instructions on (q' S as hi + lo) x (r' S as hi + lo); running sums <= (P + dq) R S^2; plus the input terms
// (3 * 2^-22 / u = 12, doubled for dq); subnormal quantum sqrt(D) 2^-25 / S.
// D = 256 (phk_knn_f16_kernel): the hi.hi chain (D/16 instructions) and the cross terms (2D/16 instructions on running sums
// and products 2^-10 of the first chain's: 11 * 32 * 2^-10 < 1, 18 * 32 * 2^-11 < 1) accumulate separately and meet in two
// float32 additions (+2 on cP, +1 on cR); the general-D kernel keeps one accumulator.
// D > 256: Q = the largest chunk norm of q' and the observed running sums carry the chain (see ErrBound).
static void split_f16_bound(RerankParams &r, const phk_model &m) {
    const uint64_t D = m.D;
    const double rho = model_rho(m);
    const double n = (D == FAST_D ? 1.0 : 3.0) * (double)D / 16.0, x = D == FAST_D ? 1.0 : 0.0;
    r.vscale = 1.0 / (4096.0 * 4096.0);
    r.per_row_scale = 0; r.eb_hsum = 0.0;
    r.eb_cA = 6.0; r.eb_cI = (PHK_MFMA_PROD * n + x) * rho; r.eb_cIf = PHK_MFMA_PROD * n + x; r.eb_cR = 6.0 + x;
    if (D == FAST_D) {
        r.eb_cQ = 0.0; r.eb_cP = PHK_MFMA_ACC * n + 24.0 + 3.0 * x; r.eb_cAmax = 0.0;
    } else {
        r.eb_cQ = PHK_MFMA_ACC * n; r.eb_cP = 24.0; r.eb_cAmax = PHK_MFMA_ACC * n;
    }
    r.eb_abs = std::sqrt((double)D) * 5.9604644775390625e-08 / 4096.0;
}

// int8:  eps(R) = u R (2 A + 4 Q + (kappa/u + 2) P + (kappa (1 + kappa)/u + 3) R) + habs
// values are T v (per row), from exact integer sums: no chain term.
// two: a refined value of the two-part sweep -- one more fused multiply-add on |v| (u |v| <= u (P R + R^2 / 2)); the
// conversion of S_L (|g S_L| <= 2^-15 |x| |y|) is inside cQ, which the two-part value's single conversion leaves room in; its
// lists carry 5 index bits in the value (score_i8.hip): 31 ulp <= 62 u |v|.
static void i8_bound(RerankParams &r, const phk_model &m, bool two) {
    const double ku = m.kappa8 / 5.9604644775390625e-08;
    r.vscale = 1.0; r.per_row_scale = 1; r.cand_a = nullptr;
    r.eb_cA = 2.0; r.eb_cQ = 4.0; r.eb_cI = 0.0; r.eb_cIf = 0.0; r.eb_cAmax = 0.0;
    r.eb_cP = ku + 2.0; r.eb_cR = ku * (1.0 + m.kappa8) + 3.0; r.eb_abs = 0.0;
    r.eb_hsum = m.hsum8;
    r.L8 = nullptr;
    if (two) {
        r.eb_cP += 1.0; r.eb_cR += 1.0;
        r.eb_cP += 62.0; r.eb_cR += 31.0;
        r.L8 = m.d_L8; r.T8 = m.d_T8;
        r.t8_blk[0] = 0; r.t8_blk[1] = m.n_rblk_ref; r.t8_blk[2] = m.n_rblk_ref + m.n_rblk_pos;
        for (int sg = 0; sg < 3; ++sg) r.lam8[sg] = m.lam8[sg];
    }
}

// count-exact f16:  eps(R) = u R (A + (11 n + 3) Q + 18 n rho I + cP P + cR R) + c_abs (R + P) + habs
// values are T S v (per row); n = 2D/16 instructions on (c - c0) x (r~' S as hi, lo), + 3 for the bias -> fp32, the final fma
// and slack; the residue of the centring through hsum.  cP / cR = 67 / 36 at k = 4, whose lists embed 5 index bits in the
// value; general D keeps its indices in registers: 62 / 31 less.  ca: the sweep's observed running sums (general D).
static void cx_bound(RerankParams &r, const phk_model &m, const float *ca) {
    const uint64_t D = m.D;
    const double rho = model_rho(m);
    const double n = 2.0 * (double)D / 16.0;
    r.vscale = 1.0 / 4096.0; r.per_row_scale = 1; r.L8 = nullptr;
    r.cand_a = ca;
    r.eb_cA = 1.0; r.eb_cQ = PHK_MFMA_ACC * n + 3.0; r.eb_cI = PHK_MFMA_PROD * n * rho; r.eb_cIf = PHK_MFMA_PROD * n;
    r.eb_cAmax = D != FAST_D ? PHK_MFMA_ACC * n : 0.0;
    r.eb_cP = D == FAST_D ? 67.0 : 5.0; r.eb_cR = D == FAST_D ? 36.0 : 5.0;
    r.eb_abs = std::sqrt((double)D) * 5.9604644775390625e-08 / 4096.0;
    r.eb_hsum = m.hsum_train > m.hsum_cen ? m.hsum_train : m.hsum_cen;
}

// k = 4 high parts only, on top of cx_bound (what phk_decide_h_kernel certifies with; the low product it adds has its own
// term, see there): the sweep issues D/16 MFMAs per value, not the count-exact kernel's 2D/16, plus the bias step --
//     cQ = 11 (D/16 + 1) + 3,  cI = 18 (D/16) rho,  cM M with M = |mu - 1/D|,  cR += cM / 2,  babs = 2^-15 2^-e / S.
// Round 5: the bias is the sweep's 17th MFMA step, - T b~_j as nine products of float16 pieces.  That instruction runs on
// |running sum| <= |counts' sum| + T |b~| and its largest nominal product is <= T |b~| (1 + 2^-11)^2: u (11 A + 18 p) adds
// 11 u on the counts' sum (the Q R term), and (11 + 18 (1 + 2^-10)) u on T |b~|, in v units |b~| / S per column.  The pieces
// carry the bias rounded to the 2^-14 2^-e grid: an absolute 2^-15 2^-e / S per value.
// (charged per column: |b_j| / S = |(mu - 1/D) . r~'_j + |r~'_j|^2 / 2| <= |mu - 1/D| R + R^2 / 2 with R >= |r'_j| (1 + 2^-21);
// by the model's largest bias, an absolute term, the exact-distance kernel got 26 % more queries, by |mu| 16 %)
static void hi_k4_bound(RerankParams &r, const phk_model &m) {
    const uint64_t D = m.D;
    const double rho = model_rho(m);
    r.eb_cQ = PHK_MFMA_ACC * ((double)D / 16.0) + 3.0;
    r.eb_cI = PHK_MFMA_PROD * ((double)D / 16.0) * rho;
    r.eb_cIf = PHK_MFMA_PROD * ((double)D / 16.0);
    r.eb_cQ += PHK_MFMA_ACC;
    const double cb = (PHK_MFMA_ACC + PHK_MFMA_PROD * (1.0 + 1.0 / 1024.0)) * (1.0 + 1.0 / 512.0);   // (|hi_j| <= S |r'_j| (1 + 2^-11); the pieces' own rounding)
    r.eb_cM = cb;
    r.eb_M = m.mu_tilde_norm;
    r.eb_cR += 0.5 * cb;
    r.eb_babs = std::ldexp(1.0, -15 - m.bias_e) / 4096.0;
}

// High-part lists read by a kernel that decides by exact candidate distances (what the high-parts decision kernels pass on):
// the lists' own model plus the missing low product, |q'| |lo_j| / S with |lo_j| <= 2^-11 (1 + 2^-11) S |r'_j| + sqrt(D) 2^-25
// (half an ulp of the high part per element; the second term covers fp16 subnormals):
//     cP += 2^-11 / u (1 + 2^-11) + 1 = 8192 (1 + 2^-11) + 1,  c_abs doubled.
static void hi_missing_low_bound(RerankParams &r) {
    r.eb_cP += 8192.0 * (1.0 + 1.0 / 2048.0) + 1.0;
    r.eb_abs *= 2.0;
}

// the high-parts decision kernels' own block: low parts and the lam* table (score_decide.hip 2d)
static void fill_hi_params(HiParams &hp, const phk_model &m) {
    hp.lo16 = m.d_lo16;
    for (int sg = 0; sg < 3; ++sg) {
        for (int i = 0; i <= 64; ++i) hp.lam_tab[sg][i] = m.lam_tab[sg][i];
        hp.lam_r0[sg] = m.lam_r0[sg];
        hp.lam_inv_step[sg] = 1.0 / m.lam_step[sg];
    }
}

// ---- the stages of a batch ----
struct ScoreBatch {
    uint64_t s, nb;               // first row within the call, rows
    int par;                      // batch number & 1: which ScoreSet, which pair of events
    const void *src;              // the rows: counts or float64 (ScoreRoute::counts)
    const uint32_t *rsum;         // their row sums, or null
    uint32_t nref, npos, nneg;    // column blocks of the three segments; a segment the method does not need has none
};

// what every kernel of the batch starts from; the stages copy it and set their own fields
static RerankParams batch_params(const ScoreRoute &r, const ScoreWs &ws, const ScoreSet &set, const ScoreBatch &b, double *d_scores,
                                 uint32_t *d_status) {
    const phk_model *m = r.m;
    RerankParams p;
    p.N = b.nb; p.M = m->M; p.n_cpos = m->n_cpos; p.n_cneg = m->n_cneg; p.D = m->D;
    p.kn = m->kn; p.method = r.method; p.rmax = m->max_colnorm; p.mu_norm = m->mu_norm;
    p.R64 = m->d_R64; p.C64 = m->d_C64; p.mu64 = m->d_mu64; p.colnorm = m->d_colnorm; p.labels = m->d_labels;
    p.cand_v = ws.first.v; p.cand_i = ws.first.i; p.cand_u = ws.first.u; p.fb_rec = ws.rec;
    p.scores = d_scores; p.status = d_status;
    p.fb_count = set.counters; p.fb_list = set.fb_list; p.slow_list = set.slow_list; p.q_base = b.s;
    p.stat_total = ws.totals;
    p.counters = set.counters;
    p.stripes = set.stripes;
    p.col_mask = m->has_mask ? m->d_col_mask : nullptr;
    p.slow_cap = r.nb_max;
    p.eb_cQ = 0.0; p.eb_cI = 0.0; p.eb_hsum = 0.0; p.per_row_scale = 0;
    p.cand_a = ws.ca; p.eb_cAmax = 0.0;
    return p;
}

// One decision pass over the lists of a (sub-)batch.  src_kind: 0 = count rows, 1 = normalised float64 rows.
static int launch_rerank(phk_ctx *ctx, int src_kind, unsigned blocks, const void *src, const RerankParams &p) {
    // phk_rerank_kernel walks the queries grid-stride (its workgroups keep the training mean in LDS): a few workgroups per CU
    const unsigned cap = (unsigned)ctx->num_cus * 16u;
    const unsigned wblocks = (p.D >= 2048 && blocks > cap) ? cap : blocks;
    if (p.D == FAST_D) {
        const char rr = ctx->knobs.rerank;
        if (rr == 'w')   // one wave per query (the general kernel), for A/B comparison
            return phk_launch_rerank_wave(ctx, src_kind, 1, false, wblocks, src, p);
        if (rr == 'g')   // four queries per wave for every query (the decision kernel off)
            return phk_launch_rerank16(ctx, src_kind, 0, (unsigned)phk_div_up(p.N, 16), src, p);
        // one lane per query for what the margin test certifies, then four per wave for the rest
        PHK_TRY(phk_launch_decide(ctx, src_kind, src, p));
        return phk_launch_rerank16(ctx, src_kind, 1, (unsigned)phk_div_up(p.N, 16), src, p);
    }
    if (!phk_fast_supports_dim(p.D)) {
        phk_set_error("phk_score: no decision kernel for D = %llu", (unsigned long long)p.D);
        return PHK_ERR_UNSUPPORTED;
    }
    const int dsub = (int)(p.D / 256);
    const bool i8h = src_kind == 0 && p.L8;
    if (i8h && p.rowsum && ctx->knobs.rerank != 'w') {
        // the lane-per-query decision kernel first; what it hands on, listed, to the wave-per-query kernel
        PHK_TRY(phk_launch_decide_gen(ctx, dsub, static_cast<const uint32_t *>(src), p));
        RerankParams pl = p;
        pl.slow_back = 2;
        return phk_launch_rerank_wave(ctx, 0, dsub, true, wblocks, src, pl);
    }
    return phk_launch_rerank_wave(ctx, src_kind, dsub, i8h, wblocks, src, p);
}

// First pass: the proposal sweep of the route's flavour into ws.first, and the error model of its lists into p.
static int stage_first_pass(phk_ctx *ctx, const ScoreRoute &r, const ScoreWs &ws, const ScoreSet &set, const ScoreBatch &b,
                            RerankParams &p, const PhkStepLink *link) {
    const phk_model *m = r.m;
    const ScoreLists &l = ws.first;
    if (r.use_i8()) {
        const bool two = r.first == FIRST_I8_TWO;
        PHK_TRY(phk_launch_proposal_i8_general(ctx, m, (const uint32_t *)b.src, b.rsum, b.nb, b.nref, b.npos, b.nneg, l.v, l.i, l.u,
                                               r.i8_groups, ws.set_bytes, two, link));
        i8_bound(p, *m, two);
        p.q2_count = set.counters + 5; p.q2_big = ws.q2_big; p.q2_wide = two ? ws.q2_wide : nullptr;
        p.rowsum = b.rsum;
    } else {
        if (r.count_exact()) cx_bound(p, *m, ws.ca);
        else split_f16_bound(p, *m);
        if (m->D != FAST_D) {
            PHK_TRY(phk_launch_proposal_f16_general(ctx, m, b.src, r.counts, r.count_exact(), b.rsum, b.nb, b.nref, b.npos, b.nneg, l.v,
                                                    l.i, l.u, ws.ca, r.first == FIRST_HI_GEN, (uint32_t)r.gen_sets, ws.set_bytes));
        } else if (r.first == FIRST_HI_K4) {
            PHK_TRY(phk_launch_proposal_f16h(ctx, m, (const uint32_t *)b.src, b.rsum, b.nb, b.nref, b.npos, b.nneg, l.v, l.i, l.u));
        } else {
            PHK_TRY(phk_launch_proposal_f16(ctx, m, b.src, r.counts, b.rsum, b.nb, b.nref, b.npos, b.nneg, l.v, l.i, l.u));
        }
    }
    if (b.nref) PHK_TRY(phk_mask_lists(ctx, m, l.v, l.i, b.nb));
    return PHK_OK;
}

// Decision at k = 4 (FIRST_HI_K4): the lane-per-query kernel on the high-part lists, then exact candidate distances for what
// it passes on -- from the same lists where possible.
static int stage_decide_k4(phk_ctx *ctx, const ScoreRoute &r, const ScoreBatch &b, const RerankParams &p) {
    HiParams hp;
    fill_hi_params(hp, *r.m);
    const dim3 dg((unsigned)phk_div_up(b.nb, 64)), db(64);
    const bool d_knn = (p.method & PHK_METHOD_KNN) != 0, d_cen = (p.method & PHK_METHOD_KMEANS) != 0;
    RerankParams pd = p;
    pd.sub_lists = PHK_SUB_LISTS;
    pd.sub_cap = 64 * phk_div_up(phk_div_up(b.nb, 64), PHK_SUB_LISTS);
    hi_k4_bound(pd, *r.m);
    PHK_TRY(phk_launch_decide_h(ctx, d_knn, d_cen, dg, db, (const uint32_t *)b.src, pd, hp));
    RerankParams ph = pd;
    hi_missing_low_bound(ph);
    ph.slow_back = 3;   // front and back list in one launch
    // (waves: sub_lists x (sub_cap / 4 + 2) local ones, four per workgroup)
    return phk_launch_rerank16(ctx, 0, 1, (unsigned)phk_div_up((uint64_t)PHK_SUB_LISTS * (pd.sub_cap / 4 + 2), 4), b.src, ph);
}

// The second passes of the int8 first pass.  Routing is PER ROW, never per batch: the first pass's decision kernel hands on what
// its lists cannot decide -- rows whose two-digit window holds more columns than the lists (clusters of near-duplicate
// references) or whose exact candidate distances do not certify to one device queue, rows beyond the int8 operand (a bin more
// than 127 from the row's centre: long or skewed contigs) to another.  One 8-byte read-back per batch tells the host the two
// lengths; each queue's rows are gathered into a dense sub-batch and swept ALONE -- the first by the three-digit int8 sweep
// (windows 2^-24 wide), the second by the f16 count-exact kernel (operand up to +-2048); only what that cannot certify either
// is brute-forced.
static int decide_second_passes(phk_ctx *ctx, const ScoreRoute &r, const ScoreWs &ws, const ScoreSet &set, const ScoreBatch &b,
                                const RerankParams &pr) {
    const phk_model *m = r.m;
    const uint64_t D = m->D;
    const ScoreLists &l = ws.first;
    uint32_t *const q2c = set.counters + 5;
    uint32_t q2n[2] = {0, 0};
    PHK_HIP(hipMemcpyAsync(q2n, q2c, sizeof(q2n), hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    for (int pass = 0; pass < 2; ++pass) {   // 0: three digits for the wide windows; 1: the f16 kernel for the long rows
        const uint64_t nq = q2n[pass];
        if (!nq) continue;
        const uint32_t *list = pass == 0 ? ws.q2_wide : ws.q2_big;
        // A sweep of the whole reference for a handful of rows is one workgroup walking every column block (0.5 ms at
        // configs[2], where a batch queues ~7 rows): below PHK_SUBPASS_MIN rows the float64 brute force, which takes eight
        // queued rows per workgroup and cuts the reference into chunks, is cheaper.
        if (nq < PHK_SUBPASS_MIN) {
            PHK_TRY(phk_launch_append_queue(ctx, list, (uint32_t)nq, set.fb_list, set.counters, q2c + pass));
            continue;
        }
        void *sub;
        PHK_TRY(phk_ws(ctx, WS_SUB, nq * (D + 1) * sizeof(uint32_t), &sub));
        uint32_t *sub_counts = (uint32_t *)sub, *sub_sum = sub_counts + nq * D;
        PHK_TRY(phk_launch_gather_list_rows(ctx, (const uint32_t *)b.src, b.rsum, list, nq, D, sub_counts, sub_sum));
        const uint32_t *sub_rs = b.rsum ? sub_sum : nullptr;
        RerankParams p2 = pr;
        p2.N = nq; p2.out_map = list; p2.status = nullptr; p2.rowsum = sub_rs;
        p2.q2_count = nullptr; p2.q2_wide = p2.q2_big = nullptr;
        if (pass == 0) {
            PHK_TRY(phk_launch_proposal_i8_general(ctx, m, sub_counts, sub_rs, nq, b.nref, b.npos, b.nneg, l.v, l.i, l.u, r.i8_groups,
                                                   ws.set_bytes, false));
            i8_bound(p2, *m, false);
        } else {
            PHK_TRY(phk_launch_proposal_f16_general(ctx, m, sub_counts, true, true, sub_rs, nq, b.nref, b.npos, b.nneg, l.v, l.i, l.u,
                                                    ws.ca, false, (uint32_t)r.gen_sets, ws.set_bytes));
            cx_bound(p2, *m, ws.ca);
        }
        PHK_TRY(launch_rerank(ctx, 0, (unsigned)phk_div_up(nq, 4), sub_counts, p2));
    }
    return PHK_OK;
}

// Decision of every other flavour: general D (k = 5, 6) and the split-query lists at k = 4.
static int stage_decide(phk_ctx *ctx, const ScoreRoute &r, const ScoreWs &ws, const ScoreSet &set, const ScoreBatch &b,
                        const RerankParams &p) {
    const unsigned rblocks = (unsigned)phk_div_up(b.nb, 4);
    if (r.first == FIRST_HI_GEN) {
        HiParams hp;
        fill_hi_params(hp, *r.m);
        PHK_TRY(phk_launch_rerank_h(ctx, (int)(r.m->D / 256), rblocks, (const uint32_t *)b.src, p, hp));
        // what it passes on: the one-wave-per-query kernel on the listed queries
        RerankParams ph = p;
        hi_missing_low_bound(ph);
        ph.slow_back = 2;
        return launch_rerank(ctx, 0, rblocks, b.src, ph);
    }
    RerankParams pr = p;
    if (ws.pend && ctx->knobs.rerank != 'w') {   // general D: the proximity metric is finished by a lane-per-query kernel
        PHK_HIP(hipMemsetAsync(ws.pend, 0xFF, b.nb * 2 * sizeof(double), ctx->stream));   // NaN: not decided here
        pr.pend = ws.pend;
    }
    PHK_TRY(launch_rerank(ctx, r.src_kind(), rblocks, b.src, pr));
    if (r.use_i8()) PHK_TRY(decide_second_passes(ctx, r, ws, set, b, pr));
    if (pr.pend) PHK_TRY(phk_launch_finish_cen(ctx, b.nb, ws.pend, p.scores + b.s));
    return PHK_OK;
}

// Tail: the second chance (k = 4) for the first pass's queue, the float64 brute force for what is queued after it, the merge
// -- the set's last kernel, which leaves its counters and stripes zeroed for batch b + 2 / the next call.
static int stage_tail(phk_ctx *ctx, const ScoreRoute &r, const ScoreWs &ws, const ScoreSet &set, const ScoreBatch &b,
                      const RerankParams &p) {
    const phk_model *m = r.m;
    RerankParams pf = p;   // what the brute force works from
    if (r.second) {
        const ScoreLists &l = ws.second;
        const uint64_t cap = b.nb < r.cap2 ? b.nb : r.cap2;
        PHK_TRY(phk_launch_proposal_f16(ctx, m, b.src, true, b.rsum, cap, b.nref, b.npos, b.nneg, l.v, l.i, l.u, set.fb_list,
                                        set.counters, PHK_SECOND_SPLITS, ws.set2_bytes));
        if (b.nref) PHK_TRY(phk_mask_lists(ctx, m, l.v, l.i, cap));
        RerankParams p2 = p;
        split_f16_bound(p2, *m);
        p2.N = cap;
        p2.cand_v = l.v; p2.cand_i = l.i; p2.cand_u = l.u; p2.cand_a = nullptr;
        p2.map = set.fb_list; p2.map_count = set.counters;
        p2.fb_count = set.counters + 3; p2.fb_list = set.fb2_list;
        p2.exact_extra = set.counters + 1;
        PHK_TRY(phk_launch_rerank16(ctx, 0, 2, (unsigned)phk_div_up(cap, 16), b.src, p2));
        pf = p2;
        pf.N = b.nb;
    }
    pf.fb_rec_cap = r.nb_max * FB_CHUNKS;
    if (m->D == FAST_D) {
        PHK_TRY(phk_launch_fallback_partial(ctx, r.src_kind(), ws.fb_lds, b.src, pf));
    } else {   // general D: the queued queries eight at a time against a chunk of the reference (see the kernel)
        PHK_TRY(phk_launch_fallback_group(ctx, r.src_kind(), (int)(m->D / 256), b.src, pf));
    }
    pf.clean_counters = set.counters;
    pf.clean_stripes = set.stripes;
    return phk_launch_fallback_merge(ctx, pf);
}

// ---- the second stream ----
// ctx->stream for the lifetime of the scope, restored on every way out: the launchers enqueue on it and the profiler's events
// (phk_prof_begin) follow it.
struct StreamScope {
    phk_ctx *ctx;
    hipStream_t saved;
    StreamScope(phk_ctx *c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
    ~StreamScope() { ctx->stream = saved; }
};

static int ensure_second_stream(phk_ctx *ctx) {
    if (ctx->aux) return PHK_OK;
    PHK_HIP(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
    for (auto &e : ctx->ev_fork) PHK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : ctx->ev_tail) PHK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return PHK_OK;
}

// tail_used[par]: a tail on the second stream recorded ev_tail[par] and nothing on the main stream has waited for it yet
static int wait_tail(phk_ctx *ctx, bool (&tail_used)[2], int par) {
    if (tail_used[par]) {
        PHK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_tail[par], 0));
        tail_used[par] = false;
    }
    return PHK_OK;
}

// One batch: first pass and decision on the main stream; the tail there too, or (tail_aside) forked onto the second stream,
// where it runs beside the next batch's sweep.  Main-stream work on set b & 1 waits for the tail of batch b - 2, which read it.
static int score_batch(phk_ctx *ctx, const ScoreRoute &r, const ScoreWs &ws, ScoreBatch b, double *d_scores, uint32_t *d_status,
                       const PhkStepLink *link, bool (&tail_used)[2]) {
    const ScoreSet &set = ws.set[b.par];
    PHK_TRY(wait_tail(ctx, tail_used, b.par));
    if (r.use_i8() && !b.rsum) {   // the int8 path's kernels (fragments, sweep, lane-per-query decision) take the row sums as input
        void *rs;
        PHK_TRY(phk_ws(ctx, WS_NWIN, b.nb * sizeof(uint32_t), &rs));
        PHK_LAUNCH(ctx, "phk_rowsum_kernel",
                   phk_rowsum_kernel<<<dim3((unsigned)phk_div_up(b.nb, 4)), dim3(256), 0, ctx->stream>>>((const uint32_t *)b.src, b.nb, r.m->D, (uint32_t *)rs));
        b.rsum = (const uint32_t *)rs;
    }
    RerankParams p = batch_params(r, ws, set, b, d_scores, d_status);
    PHK_TRY(stage_first_pass(ctx, r, ws, set, b, p, link));
    if (r.first == FIRST_HI_K4) PHK_TRY(stage_decide_k4(ctx, r, b, p));
    else PHK_TRY(stage_decide(ctx, r, ws, set, b, p));
    if (!r.tail_aside) return stage_tail(ctx, r, ws, set, b, p);
    PHK_HIP(hipEventRecord(ctx->ev_fork[b.par], ctx->stream));
    PHK_HIP(hipStreamWaitEvent(ctx->aux, ctx->ev_fork[b.par], 0));
    StreamScope aside(ctx, ctx->aux);
    PHK_TRY(stage_tail(ctx, r, ws, set, b, p));
    PHK_HIP(hipEventRecord(ctx->ev_tail[b.par], ctx->aux));
    tail_used[b.par] = true;
    return PHK_OK;
}

// link: the hand-over from the count stage of the same phk_count_score_dev call (PhkStepLink), or null
int phk_score_fast(phk_ctx *ctx, const phk_model *m, const double *d_Q, const uint32_t *d_counts, const uint32_t *d_rowsum,
                   uint64_t N, int method, double *d_scores, uint32_t *d_status, const PhkStepLink *link) {
    const uint64_t D = m->D;
    const ScoreRoute r = score_route(ctx->knobs, m, d_counts != nullptr, method, N);
    ScoreWs ws;
    PHK_TRY(score_workspace(ctx, r, link, ws));
    if (r.tail_aside) PHK_TRY(ensure_second_stream(ctx));
    bool tail_used[2] = {false, false};
    int rc = PHK_OK;
    for (uint64_t s = 0; s < N && rc == PHK_OK; s += r.BATCH) {
        ScoreBatch b;
        b.s = s;
        b.nb = N - s < r.BATCH ? N - s : r.BATCH;
        b.par = (int)((s / r.BATCH) & 1);
        b.src = d_counts ? (const void *)(d_counts + s * D) : (const void *)(d_Q + s * D);
        b.rsum = d_rowsum ? d_rowsum + s : nullptr;
        b.nref = (method & PHK_METHOD_KNN) ? m->n_rblk_ref : 0;
        b.npos = (method & PHK_METHOD_KMEANS) ? m->n_rblk_pos : 0;
        b.nneg = (method & PHK_METHOD_KMEANS) ? m->n_rblk_neg : 0;
        rc = score_batch(ctx, r, ws, b, d_scores, d_status, link, tail_used);
    }
    for (int par = 0; par < 2; ++par) {   // on every way out of the loop: the second stream's work is done before what the caller enqueues next
        const int rcj = wait_tail(ctx, tail_used, par);
        if (rc == PHK_OK) rc = rcj;
    }
    if (rc == PHK_OK) ctx->score_ctl_dirty = false;
    return rc;
}

// per-device kernel attributes, called from phk_create
int phk_score_mfma_init_device(phk_ctx *ctx) { return phk_score_fallback_init_device(ctx); }

// ---- cross-validation service: one resident model, a fold = a column mask + that fold's centroids ----
extern "C" int phk_model_set_centroids(phk_ctx *ctx, phk_model *m, const double *cpos, uint64_t n_cpos, const double *cneg,
                                       uint64_t n_cneg) {
    PHK_ENTER(ctx, "phk_model_set_centroids");
    PHK_REQUIRE(m && cpos && cneg, "phk_model_set_centroids: NULL");
    PHK_REQUIRE(n_cpos == m->n_cpos && n_cneg == m->n_cneg && n_cpos > 0,
                "phk_model_set_centroids: the model was created with %llu + %llu centroids (got %llu + %llu)",
                (unsigned long long)m->n_cpos, (unsigned long long)m->n_cneg, (unsigned long long)n_cpos, (unsigned long long)n_cneg);
    const uint64_t D = m->D;
    PHK_HIP(hipStreamSynchronize(ctx->stream));   // kernels still reading the old centroids
    PHK_HIP(hipMemcpy(m->d_C64, cpos, n_cpos * D * sizeof(double), hipMemcpyHostToDevice));
    PHK_HIP(hipMemcpy(m->d_C64 + n_cpos * D, cneg, n_cneg * D * sizeof(double), hipMemcpyHostToDevice));
    if (!m->fast) return PHK_OK;
    std::vector<double> cnorm(n_cpos + n_cneg);
    double mx = m->max_colnorm_train;
    for (uint64_t r = 0; r < n_cpos + n_cneg; ++r) {
        const double *row = r < n_cpos ? cpos + r * D : cneg + (r - n_cpos) * D;
        double s2 = 0.0;
        for (uint64_t d = 0; d < D; ++d) {
            const double v = (double)(float)(row[d] - m->h_mu[d]);
            s2 += v * v;
        }
        cnorm[r] = std::sqrt(s2);
        PHK_REQUIRE(cnorm[r] == cnorm[r] && !std::isinf(cnorm[r]), "phk_model_set_centroids: centroid %llu is not finite", (unsigned long long)r);
        mx = cnorm[r] > mx ? cnorm[r] : mx;
    }
    PHK_HIP(hipMemcpy(m->d_colnorm + m->M, cnorm.data(), cnorm.size() * sizeof(double), hipMemcpyHostToDevice));
    m->max_colnorm = mx;
    m->cen_replaced = true;
    m->bf_stale = true;
    PHK_TRY(phk_model_update_centroids_f16(m, cpos, cneg, cnorm.data()));
    if (m->has_mask) {
        // new centroids that move the bias exponent rewrite the bias pieces of every block, the train blocks' from the
        // unmasked host copy: mask them again, so the order of set_centroids and set_column_mask does not matter
        PHK_TRY(phk_model_apply_mask_f16(ctx, m));
        PHK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PHK_OK;
}

extern "C" int phk_model_set_column_mask(phk_ctx *ctx, phk_model *m, const uint8_t *mask) {
    PHK_ENTER(ctx, "phk_model_set_column_mask");
    PHK_REQUIRE(m, "phk_model_set_column_mask: NULL model");
    if (!mask && !m->has_mask) return PHK_OK;
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (mask) {
        uint64_t kept = 0;
        for (uint64_t c = 0; c < m->M; ++c) kept += mask[c] ? 0 : 1;
        PHK_REQUIRE(kept >= (uint64_t)m->kn, "phk_model_set_column_mask: %llu unmasked train rows, k_neighbors = %d",
                    (unsigned long long)kept, m->kn);
        if (!m->d_col_mask) PHK_HIP(hipMalloc((void **)&m->d_col_mask, m->M + 16));
        PHK_HIP(hipMemcpy(m->d_col_mask, mask, m->M, hipMemcpyHostToDevice));
    }
    m->has_mask = mask != nullptr;
    m->eff_pos = m->n_pos;   // (unmasked rows per class: the density method's n_c_eff)
    m->eff_neg = m->n_neg;
    if (mask) {
        for (uint64_t c = 0; c < m->n_pos; ++c) m->eff_pos -= mask[c] ? 1 : 0;
        for (uint64_t c = m->n_pos; c < m->M; ++c) m->eff_neg -= mask[c] ? 1 : 0;
    }
    if (m->fast) {
        // (the fp32 / int8 operands are never masked -- those sweeps stand down while a mask is set -- so clearing the mask
        // makes them valid again unless the centroids were replaced meanwhile)
        m->bf_stale = m->has_mask || m->cen_replaced;
        PHK_TRY(phk_model_apply_mask_f16(ctx, m));
        PHK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PHK_OK;
}
