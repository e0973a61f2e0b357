// svm_shared.h -- what the Nu-SVC of svm.hip lends the nu x gamma sweep of svm_sweep.hip: the solver's constants and the host
// launchers of its kernel matrix, row gather and decision path (one definition of each, so a sweep cell gets the bits of the
// single fit by construction).
#pragma once
#include "phk_common.h"

#define SVM_T 1024      // solver threads (one workgroup)
#define SVM_STEPS 4096  // solver iterations per launch
#define SVM_TAU 1e-12   // libsvm's TAU
// libsvm's largest problem here: Q is n x n float32
#define SVM_MAX_ROWS 65536u

// svm.hip
// Qf[n][n] = the signed Qfloat matrix of the grouped rows d_Xg[n][D] (norms xn, y = +1 / -1) at gamma; profiled as
// phk_svm_gram_kernel
int svm_launch_gram(phk_ctx *ctx, const double *d_Xg, const double *xn, uint64_t n, uint64_t D, double gamma, const int8_t *dy,
                    float *Qf);
// rows d_idx[0..n) of d_X[][D] -> d_out[n][D]; profiled as phk_svm_gather_kernel
int svm_launch_gather(phk_ctx *ctx, const double *d_X, uint64_t D, const uint32_t *d_idx, uint64_t n, double *d_out);
// libsvm's decision values (score: the method's 1.0 / 0.0) of device rows under device support vectors, see svm.hip
int svm_decision_run(phk_ctx *ctx, const double *d_Q, const uint32_t *d_counts, uint64_t N, const double *d_sv,
                     const double *d_svn, const double *d_coef, uint64_t n_sv, uint64_t D, double gamma, double rho, bool score,
                     double *d_out, uint32_t *d_status);

// ---- the solver's device code: one definition for the single fit (svm.hip) and the batched one (svm_sweep.hip) ----------
struct SvmCtl {
    int32_t iter;   // iterations done
    int32_t done;   // the stop test held (or max_iter was reached)
    double rho, r;  // calculate_rho (before the 1/r scaling)
};

// a solver workgroup's words in LDS
struct SvmShared {
    double v[2 * (SVM_T / 64)];   // the reductions' slots, two pairs per wave
    int i[2 * (SVM_T / 64)];
    int ij[2];                    // the working pair and its two steps
    double d[2];
    int stop;
};

// (value, index) pairs ordered by value, then by index: the larger pair wins a max, the (smaller value, larger index) pair
// a min -- what the sequential scans with ">=" / "<=" keep (the last of equal values).
__device__ __forceinline__ void svm_argmax(double &v, int &i, double v2, int i2) {
    if (v2 > v || (v2 == v && i2 > i)) {
        v = v2;
        i = i2;
    }
}
__device__ __forceinline__ void svm_argmin(double &v, int &i, double v2, int i2) {
    if (v2 < v || (v2 == v && i2 > i)) {
        v = v2;
        i = i2;
    }
}

// block-wide reduction of two (value, index) pairs over a workgroup of nw waves: MAX0 / MAX1 = true for max, false for min.
// The result is in every thread.  (Commutative and associative: neither the order of the folds nor nw matters.)  s_v / s_i:
// 2 * nw slots each.
template <bool MAX0, bool MAX1>
__device__ void svm_reduce2(double &v0, int &i0, double &v1, int &i1, double *s_v, int *s_i, int nw) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double a = __shfl_xor(v0, o), b = __shfl_xor(v1, o);
        const int ia = __shfl_xor(i0, o), ib = __shfl_xor(i1, o);
        if (MAX0) svm_argmax(v0, i0, a, ia); else svm_argmin(v0, i0, a, ia);
        if (MAX1) svm_argmax(v1, i1, b, ib); else svm_argmin(v1, i1, b, ib);
    }
    if (nw == 1) return;
    if (lane == 0) {
        s_v[2 * wave] = v0;
        s_i[2 * wave] = i0;
        s_v[2 * wave + 1] = v1;
        s_i[2 * wave + 1] = i1;
    }
    __syncthreads();
    for (int w = 0; w < nw; ++w) {
        if (MAX0) svm_argmax(v0, i0, s_v[2 * w], s_i[2 * w]); else svm_argmin(v0, i0, s_v[2 * w], s_i[2 * w]);
        if (MAX1) svm_argmax(v1, i1, s_v[2 * w + 1], s_i[2 * w + 1]); else svm_argmin(v1, i1, s_v[2 * w + 1], s_i[2 * w + 1]);
    }
    __syncthreads();   // (s_v / s_i are reused by the next reduction)
}

// Solver_NU, no shrinking, C_i = 1 (scikit-learn passes unit sample weights), by one workgroup of any whole number of waves:
// at most max_steps iterations from the state (alpha, G, iter); thread t owns rows t, t + blockDim.x, ...  y in the grouped
// order: +1 / -1, and 0 for a row that is not part of the problem (every loop skips it, so the rows that are keep their order
// and with it every tie).  alpha_i >= 1: upper bound, alpha_i <= 0: lower bound (update_alpha_status).  An iteration is
// (i) two (value, index) arg-max reductions, (ii) the j choice (min obj_diff, last index on ties) with the two second maxima,
// (iii) the two-variable update by thread 0, (iv) G += Q_i d_i + Q_j d_j by the row owners.  Returns true (in every thread)
// once the stop test holds or iter has reached max_iter (-1: no limit).  alpha, G and y may live in LDS or in global memory.
// TC: the workgroup's threads where the kernel fixes them (the loops over waves and rows then have constant bounds), 0 = blockDim.x.
template <int TC = 0>
__device__ __forceinline__ bool svm_solve_steps(const float *__restrict__ Qf, const int8_t *y, uint64_t n, double eps,
                                                int32_t max_iter, int32_t max_steps, double *alpha, double *G, int &iter,
                                                SvmShared &sh) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, T = TC ? TC : (int)blockDim.x, nw = T >> 6;
    const int ni = (int)n;
    const double INF = __builtin_inf();
    bool finished = false;
    for (int step = 0; step < max_steps; ++step) {
        if (max_iter != -1 && iter >= max_iter) {
            finished = true;
            break;
        }
        // (i) i candidates: -G[t] over y = +1 rows below the upper bound, G[t] over y = -1 rows above the lower bound
        double gp = -INF, gn = -INF;
        int ip = -1, in = -1;
        for (int t = tid; t < ni; t += T) {
            const double a = alpha[t], g = G[t];
            const int yt = y[t];
            if (yt == 1) {
                if (!(a >= 1.0) && -g >= gp) {
                    gp = -g;
                    ip = t;
                }
            } else if (yt == -1 && !(a <= 0.0) && g >= gn) {
                gn = g;
                in = t;
            }
        }
        svm_reduce2<true, true>(gp, ip, gn, in, sh.v, sh.i, nw);
        // (ii) j: min obj_diff (last index on ties) + the second maxima Gmaxp2 / Gmaxn2
        double gp2 = -INF, gn2 = -INF, od_min = INF;
        int jmin = -1, dummy0 = -1, dummy1 = -1;
        const float *Qp = ip >= 0 ? Qf + (uint64_t)ip * n : nullptr;
        const float *Qn = in >= 0 ? Qf + (uint64_t)in * n : nullptr;
        for (int t = tid; t < ni; t += T) {
            const double a = alpha[t], g = G[t];
            const int yt = y[t];
            if (yt == 1) {
                if (!(a <= 0.0)) {
                    const double gd = gp + g;
                    if (g >= gp2) gp2 = g;
                    if (gd > 0.0) {
                        const double qc = 2.0 - (double)(2.0f * Qp[t]);
                        const double od = -(gd * gd) / (qc > 0.0 ? qc : SVM_TAU);
                        if (od <= od_min) {
                            od_min = od;
                            jmin = t;
                        }
                    }
                }
            } else if (yt == -1 && !(a >= 1.0)) {
                const double gd = gn - g;
                if (-g >= gn2) gn2 = -g;
                if (gd > 0.0) {
                    const double qc = 2.0 - (double)(2.0f * Qn[t]);
                    const double od = -(gd * gd) / (qc > 0.0 ? qc : SVM_TAU);
                    if (od <= od_min) {
                        od_min = od;
                        jmin = t;
                    }
                }
            }
        }
        svm_reduce2<true, true>(gp2, dummy0, gn2, dummy1, sh.v, sh.i, nw);
        double od2 = 0.0;
        int dummy2 = -1;
        svm_reduce2<false, true>(od_min, jmin, od2, dummy2, sh.v, sh.i, nw);
        // (iii) stop test and the two-variable update (thread 0)
        if (tid == 0) {
            const double m1 = gp + gp2, m2 = gn + gn2;
            if ((m1 > m2 ? m1 : m2) < eps || jmin == -1) {
                sh.stop = 1;
            } else {
                sh.stop = 0;
                const int j = jmin, i = y[j] == 1 ? ip : in;
                const double Qij = (double)Qf[(uint64_t)i * n + j];
                double ai = alpha[i], aj = alpha[j];
                const double oi = ai, oj = aj;
                const double Gi = G[i], Gj = G[j];
                if (y[i] != y[j]) {
                    double qc = 2.0 + (double)(2.0f * (float)Qij);
                    if (qc <= 0.0) qc = SVM_TAU;
                    const double delta = (-Gi - Gj) / qc;
                    const double diff = ai - aj;
                    ai += delta;
                    aj += delta;
                    if (diff > 0.0) {
                        if (aj < 0.0) { aj = 0.0; ai = diff; }
                    } else {
                        if (ai < 0.0) { ai = 0.0; aj = -diff; }
                    }
                    if (diff > 0.0) {   // (C_i - C_j = 0)
                        if (ai > 1.0) { ai = 1.0; aj = 1.0 - diff; }
                    } else {
                        if (aj > 1.0) { aj = 1.0; ai = 1.0 + diff; }
                    }
                } else {
                    double qc = 2.0 - (double)(2.0f * (float)Qij);
                    if (qc <= 0.0) qc = SVM_TAU;
                    const double delta = (Gi - Gj) / qc;
                    const double sum = ai + aj;
                    ai -= delta;
                    aj += delta;
                    if (sum > 1.0) {
                        if (ai > 1.0) { ai = 1.0; aj = sum - 1.0; }
                    } else {
                        if (aj < 0.0) { aj = 0.0; ai = sum; }
                    }
                    if (sum > 1.0) {
                        if (aj > 1.0) { aj = 1.0; ai = sum - 1.0; }
                    } else {
                        if (ai < 0.0) { ai = 0.0; aj = sum; }
                    }
                }
                alpha[i] = ai;
                alpha[j] = aj;
                sh.ij[0] = i;
                sh.ij[1] = j;
                sh.d[0] = ai - oi;
                sh.d[1] = aj - oj;
            }
        }
        __syncthreads();
        if (sh.stop) {
            finished = true;
            break;
        }
        ++iter;
        // (iv) G += Q_i d_i + Q_j d_j
        {
            const float *Qi = Qf + (uint64_t)sh.ij[0] * n, *Qj = Qf + (uint64_t)sh.ij[1] * n;
            const double di = sh.d[0], dj = sh.d[1];
            for (int t = tid; t < ni; t += T) G[t] = G[t] + ((double)Qi[t] * di + (double)Qj[t] * dj);
        }
        __syncthreads();
    }
    return finished;
}

// Solver_NU::calculate_rho by the calling thread, rows in order (rows with y = 0 skipped): ctl->rho, ctl->r
__device__ __forceinline__ void svm_calculate_rho(const int8_t *y, uint64_t n, const double *alpha, const double *G,
                                                  SvmCtl *ctl) {
#pragma clang fp contract(off)
    const int ni = (int)n;
    const double INF = __builtin_inf();
    int nf1 = 0, nf2 = 0;
    double ub1 = INF, ub2 = INF, lb1 = -INF, lb2 = -INF, sf1 = 0.0, sf2 = 0.0;
    for (int i = 0; i < ni; ++i) {
        const double a = alpha[i], g = G[i];
        const int yi = y[i];
        if (yi == 1) {
            if (a >= 1.0) lb1 = fmax(lb1, g);
            else if (a <= 0.0) ub1 = fmin(ub1, g);
            else { ++nf1; sf1 += g; }
        } else if (yi == -1) {
            if (a >= 1.0) lb2 = fmax(lb2, g);
            else if (a <= 0.0) ub2 = fmin(ub2, g);
            else { ++nf2; sf2 += g; }
        }
    }
    const double r1 = nf1 > 0 ? sf1 / nf1 : (ub1 + lb1) / 2;
    const double r2 = nf2 > 0 ? sf2 / nf2 : (ub2 + lb2) / 2;
    ctl->r = (r1 + r2) / 2;
    ctl->rho = (r1 - r2) / 2;
}
