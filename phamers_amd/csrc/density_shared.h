// density_shared.h -- what the Gaussian-KDE translation units (density.hip: two classes at one bandwidth each;
// density_sweep.hip: one data set at many bandwidths) share: the log-sum-exp pair merge and the host-side normaliser.
#pragma once
#include <cmath>

#include "phk_common.h"

// (m1, s1) <- the log-sum-exp pair of the union of two sets: m = max term, s = sum of exp(term - m).  s == 0 = empty set.
// Symmetric in its operands (so the two lanes of a butterfly step hold the same result).
__device__ __forceinline__ void kde_merge(double &m1, double &s1, double m2, double s2) {
    if (s2 == 0.0) return;
    if (s1 == 0.0) {
        m1 = m2;
        s1 = s2;
        return;
    }
    const double m = fmax(m1, m2);
    s1 = s1 * exp(m1 - m) + s2 * exp(m2 - m);
    m1 = m;
}

// log(n) + (D/2) log(2 pi) + D log(h): what score_samples subtracts from the log-sum-exp (sklearn/neighbors/_kde.py:
// log_density -= log(N); _binary_tree.pxi _log_kernel_norm for the Gaussian kernel)
static inline double kde_lognorm(uint64_t n, uint64_t D, double h) {
    return std::log((double)n) + 0.5 * (double)D * std::log(2.0 * M_PI) + (double)D * std::log(h);
}

static inline bool kde_bandwidth_ok(double h) { return h > 0.0 && h < __builtin_inf(); }   // (false for NaN)
