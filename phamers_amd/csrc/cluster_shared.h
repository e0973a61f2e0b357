// cluster_shared.h -- what cluster.hip (phk_dbscan) and dbscan_sweep.hip (phk_dbscan_sweep) both use: the lock-free
// union-find of the core points on the device, and cluster.hip's host helpers of the DBSCAN passes.
#pragma once
#include "phk_common.h"

// Union-find on the parent array of the core points (compact indices: core point m is row core[m] of X; compact order is
// row order).  The larger root is hooked under the smaller, so a component's root is its smallest member.  The array is
// written by workgroups on all XCDs at once and the XCD L2s are not coherent: every access here is an agent-scope atomic.
__device__ __forceinline__ int32_t uf_load(int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x) {
    for (;;) {
        const int32_t p = uf_load(parent + x);
        if (p == x) return x;
        const int32_t gp = uf_load(parent + p);
        if (gp != p) {   // path halving: parent[x] moves to an ancestor only
            int32_t e = p;
            __hip_atomic_compare_exchange_strong(parent + x, &e, gp, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        x = gp;
    }
}

__device__ __forceinline__ void uf_union(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        int32_t e = b;   // b is (was) a root: hook it under the smaller root a
        if (__hip_atomic_compare_exchange_strong(parent + b, &e, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

// the same on the tile's 128 slots in LDS (one workgroup: workgroup-scope atomics)
__device__ __forceinline__ int lf_find(int *lp, int x) {
    for (;;) {
        const int p = __hip_atomic_load(lp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void lf_union(int *lp, int a, int b) {
    for (;;) {
        a = lf_find(lp, a);
        b = lf_find(lp, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        int e = b;
        if (__hip_atomic_compare_exchange_strong(lp + b, &e, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
            return;
    }
}

// ---- cluster.hip, host side ----
// the largest double t with sqrt(t) <= eps (sqrt correctly rounded and monotone): s <= t  <=>  sqrt(s) <= eps
double cl_eps_threshold(double eps);
// workgroups per query block so that a launch fills the chip (~8 workgroups per CU), at most `tiles`
uint32_t cl_groups(phk_ctx *ctx, uint64_t qblocks, uint64_t tiles);
// PHK_ERR_NAN (and the message "<fname>: the data contain NaN") when any of the `count` doubles at d_p is NaN; synchronises
int cl_refuse_nan(phk_ctx *ctx, const char *fname, const double *d_p, uint64_t count);
