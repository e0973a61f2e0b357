// row_list.h -- the per-thread register list of the smallest (value, row index) pairs that the selections after the fp64 Gram
// tile keep (neighbors.hip: Gram-form distances; hosts.hip: negated log-likelihoods), and the step of the tile they scan.
#pragma once
#include "gram_tile.h"

#define NN_NOROW 0x7fffffff   // index of an empty list entry (value +inf): after every real entry
#define NN_STEP (GT_RT * 16)  // rows per row step of the tile (64)

__device__ __forceinline__ bool nn_less(double a, int32_t ja, double b, int32_t jb) { return a < b || (a == b && ja < jb); }

// (v, j) into the list sorted by (value, index): one pass of compare-exchanges over registers, the displaced entry moves on.
// A NaN value compares false everywhere and drops out.
template <int KC>
__device__ __forceinline__ void nn_insert(double (&lv)[KC], int32_t (&lj)[KC], double v, int32_t j) {
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        const bool lt = nn_less(v, j, lv[i], lj[i]);
        const double tv = lv[i];
        const int32_t tj = lj[i];
        lv[i] = lt ? v : tv;
        lj[i] = lt ? j : tj;
        v = lt ? tv : v;
        j = lt ? tj : j;
    }
}
