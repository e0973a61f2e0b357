// svm_sweep.hip -- the Nu-SVC of svm.hip over a grid gamma x nu x row subset, every problem in a workgroup of its own (gfx950):
// the fits behind a choice of the svm method's nu and gamma (phamers_amd/svm_grid.py).  Subset 0 is all rows, subset f + 1 the
// rows whose fold is not f; a fold problem also gives libsvm's decision values of its held-out rows.
//
// Bit for bit phk_nusvc_fit / phk_nusvc_decision per problem:
//   * One kernel matrix Qf (n x n float32 over ALL grouped rows, svm.hip's own Gram launch) per gamma serves every nu and
//     subset of that gamma.  An entry of the Gram tile depends on its two rows only, not on their place in the matrix, so the
//     entries a subset reads are the entries a Gram build on the gathered subset holds.
//   * A subset is a row mask: y = 0 marks a held-out row and every loop of the solver skips it.  The rows that stay keep their
//     order, and every choice of the solver -- the (value, index) reductions with their last-index ties, the row-order
//     gradient start, the row-order calculate_rho -- depends on the order of the rows only.
//   * The iteration is phk_svm_solve_kernel's own: both kernels instantiate svm_solve_steps of svm_shared.h (no fp contraction,
//     thread 0's two-variable update, G += Q_i d_i + Q_j d_j).  Its reductions are exact (max / min of pairs), so the workgroup
//     size is free: it is chosen per call from n.
//   * alpha, G and y of a problem (17 bytes per row) live in LDS for the whole launch when n rows fit, read from global memory
//     at the start of a launch and written back at its end; past that (or on request) the same kernel source works on the
//     global arrays.
// A launch runs at most SVM_STEPS iterations per open problem; the host reads the control blocks back and relaunches the
// problems that are still open.  No workgroup waits on another.
#include <cmath>
#include <vector>

#include "svm_shared.h"

// dynamic LDS of the solver: 160 KiB a workgroup may declare less the kernel's static words (below, 412 bytes)
#define SVS_LDS_DYN (160 * 1024 - 1024)
#define SVS_LDS_ROWS (SVS_LDS_DYN / 17)
#define SVS_Q_BYTES (4ull << 30)   // kernel matrices resident per pass of gammas

struct SvsProb {
    const float *Qf;     // the gamma's matrix
    const int8_t *y;     // the subset's rows: +1 / -1, 0 = held out
    double *alpha, *G;   // [n]
};

// Solver::Solve's gradient start for every problem of a pass: grid y = problem, G[j] = sum over rows i with alpha_i > 0, in row
// order, of alpha_i Q[i][j] (a held-out row has alpha = 0)
__global__ __launch_bounds__(256) void phk_svm_sweep_grad_init_kernel(const SvsProb *__restrict__ probs, uint64_t n) {
#pragma clang fp contract(off)
    const SvsProb p = probs[blockIdx.y];
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double g = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        const double a = p.alpha[i];
        if (a > 0.0) g = g + a * (double)p.Qf[i * n + j];
    }
    p.G[j] = g;
}

// Solver_NU (svm_solve_steps) for problem open[blockIdx.x]: at most max_steps iterations from the state in (alpha, G, ctl), then
// -- once the stop test holds or max_iter is reached -- calculate_rho.  LDS: the state in dynamic LDS (17 n bytes), else in place.
template <bool LDS>
__global__ __launch_bounds__(SVM_T) void phk_svm_sweep_solve_kernel(const SvsProb *__restrict__ probs,
                                                                    const uint32_t *__restrict__ open, uint64_t n, double eps,
                                                                    int32_t max_iter, int32_t max_steps,
                                                                    SvmCtl *__restrict__ ctls) {
#pragma clang fp contract(off)
    extern __shared__ double s_state[];
    __shared__ SvmShared sh;
    const uint32_t pi = open[blockIdx.x];
    const SvsProb p = probs[pi];
    SvmCtl *ctl = ctls + pi;
    const int tid = threadIdx.x, T = blockDim.x;
    const int ni = (int)n;
    const float *__restrict__ Qf = p.Qf;
    if (ctl->done) return;
    double *alpha, *G;
    const int8_t *y;
    if (LDS) {
        alpha = s_state;
        G = s_state + n;
        int8_t *ys = (int8_t *)(s_state + 2 * n);
        for (int t = tid; t < ni; t += T) {
            alpha[t] = p.alpha[t];
            G[t] = p.G[t];
            ys[t] = p.y[t];
        }
        y = ys;
        __syncthreads();
    } else {
        alpha = p.alpha;
        G = p.G;
        y = p.y;
    }
    int iter = ctl->iter;
    const bool finished = svm_solve_steps(Qf, y, n, eps, max_iter, max_steps, alpha, G, iter, sh);
    if (finished && tid == 0) {
        svm_calculate_rho(y, n, alpha, G, ctl);
        ctl->done = 1;
    }
    if (tid == 0) ctl->iter = iter;
    if (LDS) {
        for (int t = tid; t < ni; t += T) {
            p.alpha[t] = alpha[t];
            p.G[t] = G[t];
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
namespace {

// solve_nu_svc's start for the rows with y != 0: alpha filled class by class, in row order, up to nu l / 2
void svs_alpha_start(const int8_t *y, uint64_t n, uint64_t m, double nu, double *a0) {
#pragma clang fp contract(off)
    double nu_l = 0.0;
    for (uint64_t i = 0; i < m; ++i) nu_l += nu * 1.0;
    double sp = nu_l / 2, sn = nu_l / 2;
    for (uint64_t i = 0; i < n; ++i) {
        if (y[i] == 1) {
            a0[i] = 1.0 < sp ? 1.0 : sp;
            sp -= a0[i];
        } else if (y[i] == -1) {
            a0[i] = 1.0 < sn ? 1.0 : sn;
            sn -= a0[i];
        } else {
            a0[i] = 0.0;
        }
    }
}

// the workgroup size for n rows: the smallest power of two of whole waves that leaves a thread ten rows or fewer (measured on
// the reference rows, 216 problems of 4 673 rows: 14.2 us per iteration at 512 threads, 17.1 at 1 024, 18.7 at 256 --
// profiles/svm_grid/README.md)
uint32_t svs_threads(uint64_t n) {
    uint32_t t = 64;
    while (t < SVM_T && (uint64_t)t * 10 < n) t *= 2;
    return t;
}

}   // namespace

extern "C" uint32_t phk_nusvc_sweep_lds_rows(void) { return SVS_LDS_ROWS; }

extern "C" int phk_nusvc_sweep(phk_ctx *ctx, const double *X, uint64_t n, uint64_t D, const double *labels, const double *gammas,
                               uint32_t Gm, const double *nus, uint32_t V, const int32_t *fold_of, uint32_t F, double tol,
                               int32_t max_iter, int64_t lds_rows, uint32_t gammas_per_pass, uint32_t threads, int32_t *status,
                               int32_t *n_iter, int32_t *n_sv, double *rho, double *coef, double *held_dec) {
    PHK_ENTER(ctx, "phk_nusvc_sweep");
    PHK_REQUIRE(X && labels && status && n_iter && n_sv && rho && coef && D > 0 && n > 0,
                "phk_nusvc_sweep: NULL pointer, no rows or D = 0");
    PHK_REQUIRE(gammas && Gm >= 1 && nus && V >= 1, "phk_nusvc_sweep: an empty axis of the grid");
    PHK_REQUIRE(F == 0 || (fold_of && held_dec), "phk_nusvc_sweep: folds without fold ids or a place for the held-out decisions");
    PHK_REQUIRE(max_iter == -1 || max_iter > 0, "phk_nusvc_sweep: max_iter must be -1 or > 0 (got %d)", max_iter);
    PHK_REQUIRE(tol > 0.0 && tol < __builtin_inf(), "phk_nusvc_sweep: tol must be finite and > 0 (got %g)", tol);
    PHK_REQUIRE(n <= SVM_MAX_ROWS, "phk_nusvc_sweep: %llu training rows (at most %u)", (unsigned long long)n, SVM_MAX_ROWS);
    PHK_REQUIRE(threads == 0 || (threads % 64 == 0 && threads <= SVM_T),
                "phk_nusvc_sweep: threads must be a multiple of 64 up to %d (got %u)", SVM_T, threads);
    for (uint32_t g = 0; g < Gm; ++g)
        PHK_REQUIRE(gammas[g] > 0.0 && gammas[g] < __builtin_inf(), "phk_nusvc_sweep: gamma must be finite and > 0 (got %g)",
                    gammas[g]);
    for (uint32_t v = 0; v < V; ++v)
        PHK_REQUIRE(nus[v] > 0.0 && nus[v] <= 1.0, "phk_nusvc_sweep: nu <= 0 or nu > 1 (got %g)", nus[v]);
    // svm_group_classes: label 0 first, then label 1
    std::vector<uint32_t> perm;
    perm.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        PHK_REQUIRE(labels[i] == 0.0 || labels[i] == 1.0, "phk_nusvc_sweep: labels must be 0 or 1 (row %llu: %g)",
                    (unsigned long long)i, labels[i]);
        PHK_REQUIRE(F == 0 || (fold_of[i] >= 0 && (uint32_t)fold_of[i] < F), "phk_nusvc_sweep: fold id %d of row %llu (folds: %u)",
                    F ? fold_of[i] : 0, (unsigned long long)i, F);
        if (labels[i] == 0.0) perm.push_back((uint32_t)i);
    }
    const uint64_t n0 = perm.size();
    for (uint64_t i = 0; i < n; ++i)
        if (labels[i] == 1.0) perm.push_back((uint32_t)i);
    for (uint64_t e = 0; e < n * D; ++e)
        if (X[e] != X[e]) {
            phk_set_error("phk_nusvc_sweep: row %llu contains NaN", (unsigned long long)(e / D));
            return PHK_ERR_NAN;
        }

    // the subsets as masks over the grouped rows, their class sizes, and the held-out rows fold by fold
    const uint32_t S = F + 1;
    const uint64_t P = (uint64_t)Gm * V * S;
    std::vector<int8_t> ysub((uint64_t)S * n);
    std::vector<uint64_t> sub0(S, 0), sub1(S, 0);
    for (uint32_t s = 0; s < S; ++s)
        for (uint64_t g = 0; g < n; ++g) {
            const bool held = s > 0 && (uint32_t)fold_of[perm[g]] == s - 1;
            ysub[(uint64_t)s * n + g] = held ? 0 : (g < n0 ? 1 : -1);
            if (!held) ++(g < n0 ? sub0[s] : sub1[s]);
        }
    std::vector<uint32_t> held_rows;      // grouped indices, fold by fold
    std::vector<uint64_t> held_off(S, 0);   // fold f: held_rows[held_off[f] .. held_off[f + 1])
    for (uint32_t f = 0; f < F; ++f) {
        for (uint64_t g = 0; g < n; ++g)
            if ((uint32_t)fold_of[perm[g]] == f) held_rows.push_back((uint32_t)g);
        held_off[f + 1] = held_rows.size();
    }

    for (uint64_t q = 0; q < P; ++q) {
        status[q] = PHK_SVM_INFEASIBLE;
        n_iter[q] = 0;
        n_sv[q] = 0;
        rho[q] = __builtin_nan("");
    }
    for (uint64_t e = 0; e < P * n; ++e) coef[e] = 0.0;
    const double nan = __builtin_nan("");
    if (F)
        for (uint64_t e = 0; e < (uint64_t)Gm * V * n; ++e) held_dec[e] = nan;

    // svm_check_parameter per (nu, subset); what is left is launched
    std::vector<uint8_t> feasible((uint64_t)V * S);
    uint64_t per_gamma = 0;
    for (uint32_t v = 0; v < V; ++v)
        for (uint32_t s = 0; s < S; ++s) {
            const uint64_t a = sub0[s], b = sub1[s];
            const bool ok = a > 0 && b > 0 && !(nus[v] * (double)(a + b) / 2 > (double)(a < b ? a : b));
            feasible[(uint64_t)v * S + s] = ok;
            per_gamma += ok;
        }
    if (per_gamma == 0) return PHK_OK;

    const bool use_lds = lds_rows < 0 ? n <= SVS_LDS_ROWS : (uint64_t)lds_rows >= n && n <= SVS_LDS_ROWS;
    const uint32_t T = threads ? threads : svs_threads(n);
    uint32_t gp = (uint32_t)(SVS_Q_BYTES / (n * n * sizeof(float)));
    if (gammas_per_pass) gp = gammas_per_pass;
    PHK_REQUIRE(per_gamma <= 65535, "phk_nusvc_sweep: %llu problems per gamma (at most 65535)", (unsigned long long)per_gamma);
    if ((uint64_t)gp * per_gamma > 65535) gp = (uint32_t)(65535 / per_gamma);   // (a pass is one grid: y = problem)
    gp = gp < 1 ? 1 : (gp > Gm ? Gm : gp);
    const uint64_t NP = per_gamma * gp;   // problems of a pass, at most

    const char *fn = "phk_nusvc_sweep";
    PhkDevMem m_xg, m_xn, m_y, m_Q, m_state, m_ctl, m_probs, m_open, m_held, m_sv, m_dec;   // the call's buffers, freed on every way out
    void *d_x, *d_idx, *d_flags;
    PHK_TRY(phk_ws(ctx, WS_WIDE, n * D * sizeof(double), &d_x));
    PHK_TRY(phk_ws(ctx, WS_OFFSETS, n * sizeof(uint32_t), &d_idx));
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &d_flags));
    PHK_TRY(m_xg.alloc(fn, "grouped rows", n * D * sizeof(double)));
    PHK_TRY(m_xn.alloc(fn, "row norms", n * sizeof(double)));
    PHK_TRY(m_y.alloc(fn, "y", (uint64_t)S * n));
    PHK_TRY(m_Q.alloc(fn, "Q", (uint64_t)gp * n * n * sizeof(float)));
    PHK_TRY(m_state.alloc(fn, "solver states", NP * 2 * n * sizeof(double)));
    PHK_TRY(m_ctl.alloc(fn, "control words", NP * sizeof(SvmCtl)));
    PHK_TRY(m_probs.alloc(fn, "problems", NP * sizeof(SvsProb)));
    PHK_TRY(m_open.alloc(fn, "open problems", NP * sizeof(uint32_t)));
    PHK_TRY(m_held.alloc(fn, "held-out rows", F ? n * D * sizeof(double) : 0));
    PHK_TRY(m_sv.alloc(fn, "support vectors", F ? n * D * sizeof(double) + 2 * n * sizeof(double) : 0));
    PHK_TRY(m_dec.alloc(fn, "decision values", F ? (uint64_t)Gm * V * n * sizeof(double) : 0));
    void *v_probs = m_probs.ptr, *v_open = m_open.ptr, *v_held = m_held.ptr;
    double *d_xg = m_xg.as<double>(), *d_xn = m_xn.as<double>(), *d_state = m_state.as<double>();
    double *d_sv = m_sv.as<double>(), *d_svn = d_sv + n * D, *d_svcoef = d_svn + n, *d_dec = m_dec.as<double>();
    int8_t *d_y = m_y.as<int8_t>();
    float *d_Q = m_Q.as<float>();
    SvmCtl *d_ctl = m_ctl.as<SvmCtl>();

    PHK_TRY(phk_copy_to_device(ctx, d_x, X, n * D * sizeof(double)));
    PHK_HIP(hipMemcpyAsync(d_idx, perm.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PHK_TRY(svm_launch_gather(ctx, (const double *)d_x, D, (const uint32_t *)d_idx, n, d_xg));
    PHK_HIP(hipMemcpyAsync(d_y, ysub.data(), (uint64_t)S * n, hipMemcpyHostToDevice, ctx->stream));
    PHK_TRY(phk_launch_rownorm(ctx, d_xg, n, D, d_xn));
    if (F) {
        PHK_HIP(hipMemcpyAsync(d_idx, held_rows.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        PHK_TRY(svm_launch_gather(ctx, d_xg, D, (const uint32_t *)d_idx, n, (double *)v_held));
        PHK_HIP(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), ctx->stream));
    }
    if (use_lds)
        PHK_HIP(hipFuncSetAttribute((const void *)phk_svm_sweep_solve_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    SVS_LDS_DYN));

    // the starts per (nu, subset), shared by every gamma
    std::vector<double> start((uint64_t)V * S * n, 0.0);
    for (uint32_t v = 0; v < V; ++v)
        for (uint32_t s = 0; s < S; ++s)
            if (feasible[(uint64_t)v * S + s])
                svs_alpha_start(&ysub[(uint64_t)s * n], n, sub0[s] + sub1[s], nus[v], &start[((uint64_t)v * S + s) * n]);

    std::vector<uint64_t> which;   // problem of the call behind each problem of the pass
    std::vector<SvsProb> probs;
    std::vector<SvmCtl> ctls;
    std::vector<uint32_t> open;
    std::vector<double> a_host;
    std::vector<std::vector<uint32_t>> sv_idx;
    std::vector<std::vector<double>> sv_coef;
    for (uint32_t g0 = 0; g0 < Gm; g0 += gp) {
        const uint32_t g1 = g0 + gp < Gm ? g0 + gp : Gm;
        which.clear();
        probs.clear();
        for (uint32_t g = g0; g < g1; ++g) {
            float *Qg = d_Q + (uint64_t)(g - g0) * n * n;
            PHK_TRY(svm_launch_gram(ctx, d_xg, d_xn, n, D, gammas[g], d_y, Qg));   // (subset 0's y: every row signed)
            for (uint32_t v = 0; v < V; ++v)
                for (uint32_t s = 0; s < S; ++s) {
                    if (!feasible[(uint64_t)v * S + s]) continue;
                    const uint64_t k = which.size();
                    which.push_back(((uint64_t)g * V + v) * S + s);
                    probs.push_back(SvsProb{Qg, d_y + (uint64_t)s * n, d_state + k * n, d_state + (NP + k) * n});
                }
        }
        const uint64_t np = which.size();
        a_host.resize(np * n);
        for (uint64_t k = 0; k < np; ++k) {
            const uint64_t vs = which[k] % ((uint64_t)V * S);
            std::copy(start.begin() + vs * n, start.begin() + (vs + 1) * n, a_host.begin() + k * n);
        }
        ctls.assign(np, SvmCtl{0, 0, 0.0, 0.0});
        PHK_TRY(phk_copy_to_device(ctx, d_state, a_host.data(), np * n * sizeof(double)));
        PHK_HIP(hipMemcpyAsync(v_probs, probs.data(), np * sizeof(SvsProb), hipMemcpyHostToDevice, ctx->stream));
        PHK_HIP(hipMemcpyAsync(d_ctl, ctls.data(), np * sizeof(SvmCtl), hipMemcpyHostToDevice, ctx->stream));
        PHK_LAUNCH(ctx, "phk_svm_sweep_grad_init_kernel",
                   phk_svm_sweep_grad_init_kernel<<<dim3((unsigned)phk_div_up(n, 256), (unsigned)np), dim3(256), 0, ctx->stream>>>(
                       (const SvsProb *)v_probs, n));
        for (;;) {
            open.clear();
            for (uint64_t k = 0; k < np; ++k)
                if (!ctls[k].done) open.push_back((uint32_t)k);
            if (open.empty()) break;
            PHK_HIP(hipMemcpyAsync(v_open, open.data(), open.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            if (use_lds) {
                PHK_LAUNCH(ctx, "phk_svm_sweep_solve_kernel",
                           phk_svm_sweep_solve_kernel<true><<<dim3((unsigned)open.size()), dim3(T), 17 * n, ctx->stream>>>(
                               (const SvsProb *)v_probs, (const uint32_t *)v_open, n, tol, max_iter, SVM_STEPS, d_ctl));
            } else {
                PHK_LAUNCH(ctx, "phk_svm_sweep_solve_kernel",
                           phk_svm_sweep_solve_kernel<false><<<dim3((unsigned)open.size()), dim3(T), 0, ctx->stream>>>(
                               (const SvsProb *)v_probs, (const uint32_t *)v_open, n, tol, max_iter, SVM_STEPS, d_ctl));
            }
            PHK_HIP(hipMemcpyAsync(ctls.data(), d_ctl, np * sizeof(SvmCtl), hipMemcpyDeviceToHost, ctx->stream));
            PHK_HIP(hipStreamSynchronize(ctx->stream));
        }
        PHK_TRY(phk_copy_to_host(ctx, a_host.data(), d_state, np * n * sizeof(double)));

        // solve_nu_svc: alpha_i *= y_i / r, rho /= r; a fold problem then scores its held-out rows
        sv_idx.clear();
        sv_coef.clear();
        for (uint64_t k = 0; k < np; ++k) {
            const uint64_t q = which[k];
            const uint32_t s = (uint32_t)(q % S);
            const uint32_t g = (uint32_t)(q / ((uint64_t)V * S));
            const int8_t *y = &ysub[(uint64_t)s * n];
            const double *a = &a_host[k * n];
            const SvmCtl &c = ctls[k];
            double *out = coef + q * n;
            const double rho_q = c.rho / c.r;
            bool finite = std::isfinite(rho_q);
            int32_t ns = 0;
            std::vector<uint32_t> idx;
            std::vector<double> cf;
            for (uint64_t i = 0; i < n; ++i) {
                const double ci = a[i] * ((double)y[i] / c.r);
                finite = finite && (a[i] == 0.0 || std::isfinite(ci));
                if (ci != 0.0 && y[i] != 0) {
                    ++ns;
                    idx.push_back((uint32_t)i);
                    cf.push_back(ci);
                }
            }
            n_iter[q] = c.iter;
            if (!finite) {   // r = 0: scikit-learn refuses such a fit (svm.hip)
                status[q] = PHK_SVM_NOT_FINITE;
                continue;
            }
            status[q] = PHK_SVM_OK;
            n_sv[q] = ns;
            rho[q] = rho_q;
            for (size_t e = 0; e < idx.size(); ++e) out[perm[idx[e]]] = cf[e];
            const uint64_t nh = s ? held_off[s] - held_off[s - 1] : 0;
            if (s == 0 || ns == 0 || nh == 0) continue;
            sv_idx.push_back(std::move(idx));   // (kept until the pass has drained: the copies below are stream ordered)
            sv_coef.push_back(std::move(cf));
            PHK_HIP(hipMemcpyAsync(d_idx, sv_idx.back().data(), (uint64_t)ns * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            PHK_HIP(hipMemcpyAsync(d_svcoef, sv_coef.back().data(), (uint64_t)ns * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            PHK_TRY(svm_launch_gather(ctx, d_xg, D, (const uint32_t *)d_idx, (uint64_t)ns, d_sv));
            PHK_TRY(phk_launch_rownorm(ctx, d_sv, (uint64_t)ns, D, d_svn));
            PHK_TRY(svm_decision_run(ctx, (const double *)v_held + held_off[s - 1] * D, nullptr, nh, d_sv, d_svn, d_svcoef,
                                     (uint64_t)ns, D, gammas[g], rho_q, false, d_dec + (q / S) * n + held_off[s - 1],
                                     (uint32_t *)d_flags));
        }
        PHK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (F) {
        std::vector<double> dec((uint64_t)Gm * V * n);
        PHK_TRY(phk_copy_to_host(ctx, dec.data(), d_dec, dec.size() * sizeof(double)));
        for (uint64_t cell = 0; cell < (uint64_t)Gm * V; ++cell)
            for (uint32_t f = 0; f < F; ++f) {
                const uint64_t q = cell * S + f + 1;
                if (status[q] != PHK_SVM_OK || n_sv[q] == 0) continue;
                for (uint64_t h = held_off[f]; h < held_off[f + 1]; ++h) held_dec[cell * n + perm[held_rows[h]]] = dec[cell * n + h];
            }
    }
    return PHK_OK;
}
