// row_select.h -- "the first k in order of (value, index)" of a row of non-negative doubles, by one workgroup of 256
// threads: the selection of the t-SNE neighbour graph (tsne.hip, k <= 4096) and of the nearest-reference fallback
// (neighbors.hip, k <= 28).
// Non-negative doubles order like their bit patterns, so the k-th smallest value T is found by a radix select on the 64-bit
// keys (8 passes of 8 bits, integer histogram in LDS); entries below T are collected in any order, ties at T in index order
// (an ordered scan) until k are taken; a bitonic sort of the kp (key, index) slots -- the real ones all distinct, so the
// result is unique -- puts them in order.
#pragma once
#include "phk_common.h"

struct RsScratch {   // the routine's own LDS
    uint32_t hist[256];
    uint32_t wsum[4];
    uint64_t prefix;
    uint32_t need, cnt, eq;
};

// row[n]: the keys (bit patterns; +inf and NaN sort last); 1 <= k <= min(n, kp), kp a power of two >= 2, the size of the
// caller's slot arrays skey / sidx.  On return (behind a barrier) slots 0 .. k - 1 hold the first k in order of (key, index).
__device__ __forceinline__ void rs_select_sorted(const uint64_t *__restrict__ row, uint64_t n, uint32_t k, uint32_t kp, uint64_t *skey,
                                                 int32_t *sidx, RsScratch &sc) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint64_t prefix = 0;
    uint32_t need = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        sc.hist[t] = 0;
        __syncthreads();
        const uint64_t hi = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (uint64_t j = t; j < n; j += 256) {
            const uint64_t key = row[j];
            if ((key & hi) == prefix) atomicAdd(&sc.hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (t == 0) {
            uint32_t cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (cum + sc.hist[b] >= need) break;
                cum += sc.hist[b];
            }
            sc.prefix = prefix | ((uint64_t)b << shift);
            sc.need = need - cum;
        }
        __syncthreads();
        prefix = sc.prefix;
        need = sc.need;
        __syncthreads();
    }
    const uint64_t T = prefix;          // the k-th smallest key; `need` of the entries equal to it are taken
    const uint32_t nless = k - need;
    if (t == 0) {
        sc.cnt = 0;
        sc.eq = 0;
    }
    for (uint32_t e = k + t; e < kp; e += 256) {   // padding of the sort: after every real entry
        skey[e] = ~0ull;
        sidx[e] = INT32_MAX;
    }
    __syncthreads();
    for (uint64_t base = 0; base < n; base += 256) {
        const uint64_t j = base + t;
        const uint64_t key = j < n ? row[j] : ~0ull;
        if (key < T) {
            const uint32_t slot = atomicAdd(&sc.cnt, 1u);
            if (slot < nless) {
                skey[slot] = key;
                sidx[slot] = (int32_t)j;
            }
        }
        const bool eq = key == T;
        const unsigned long long bal = __ballot(eq);
        if (lane == 0) sc.wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t rank = sc.eq + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += sc.wsum[w];
        if (eq && rank < need) {
            skey[nless + rank] = key;
            sidx[nless + rank] = (int32_t)j;
        }
        __syncthreads();
        if (t == 0) sc.eq += sc.wsum[0] + sc.wsum[1] + sc.wsum[2] + sc.wsum[3];
        __syncthreads();
    }
    for (uint32_t size = 2; size <= kp; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t e = t; e < kp; e += 256) {
                const uint32_t o = e ^ stride;
                if (o > e) {
                    const uint64_t ka = skey[e], kb = skey[o];
                    const int32_t ia = sidx[e], ib = sidx[o];
                    const bool gt = ka > kb || (ka == kb && ia > ib);
                    if (gt == ((e & size) == 0)) {
                        skey[e] = kb;
                        skey[o] = ka;
                        sidx[e] = ib;
                        sidx[o] = ia;
                    }
                }
            }
        }
    __syncthreads();
}
