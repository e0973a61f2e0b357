// rows.hip -- operations on count rows: widening, row normalisation, column gather, the count check (gfx950).
//
// Replaces kmer.normalize_counts (scripts/kmer.py:209-221) and the column gathers of scripts/transform_kmers.py:68-88.
#include "phk_common.h"

// ------------------------------------------------------------------------------------
// widen uint32 -> int64 (the reference returns NumPy's default int, scripts/kmer.py:46)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void phk_widen_kernel(const uint32_t *__restrict__ in, uint64_t count,
                                                        int64_t *__restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) out[i] = (int64_t)in[i];
}

int phk_launch_widen(phk_ctx *ctx, const uint32_t *d_in, uint64_t count, int64_t *d_out) {
    if (count == 0) return PHK_OK;
    uint64_t blocks = phk_div_up(count, 256);
    if (blocks > (uint64_t)ctx->num_cus * 16) blocks = (uint64_t)ctx->num_cus * 16;
    PHK_LAUNCH(ctx, "phk_widen_kernel",
               phk_widen_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(d_in, count, d_out));
    return PHK_OK;
}

// ------------------------------------------------------------------------------------
// normalise: one wavefront per row; out = (double)c / (double)rowsum  (0/0 -> NaN)
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void phk_normalize_int_kernel(const T *__restrict__ counts, uint64_t n,
                                                                uint64_t D, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t total = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n; r += total) {
        const T *row = counts + r * D;
        long long s = 0;  // exact: integer row sums of a count matrix are far below 2^63
        for (uint64_t j = lane; j < D; j += 64) s += (long long)row[j];
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
        const double ds = (double)s, ry = 1.0 / ds;
        if (s != 0) {
            for (uint64_t j = lane; j < D; j += 64) out[r * D + j] = phk_div_row((double)row[j], ds, ry);
        } else {   // ry = inf makes every Newton residual NaN: a zero-sum int64 row with entries (1, -1) is +-inf there, NaN elsewhere
            for (uint64_t j = lane; j < D; j += 64) out[r * D + j] = (double)row[j] / ds;
        }
    }
}

// float rows: the row sum follows NumPy's pairwise summation (what np.sum does on a
// contiguous float64 row: 8 running partial sums per <=128-element block, blocks combined by
// halving; a row wider than 8 192 elements in pieces of 8 192 whose sums are added in order) so that renormalising
// float rows matches the reference bit for bit (tests/test_gpu_rows.py; the order itself is pinned to np.sum by
// tests/test_rows_host.py).
// (The halving is a recursion in NumPy; here its frames live in an explicit stack in LDS, one per wave, walked by lane 0:
// as a recursive device function it was the library's last kernel with a call stack in scratch memory.)
__device__ __forceinline__ double phk_np_pairwise_leaf(const double *a, uint64_t n) {   // n <= 128
    if (n < 8) {
        double r = 0.0;  // NumPy starts from the first element; 0.0 + a0 is exact
        for (uint64_t i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    uint64_t i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

#define PW_DEPTH 48   // frames: a row of 2^40 elements halves 34 times
#define PW_NP_BUFSIZE 8192   // np.getbufsize(): the most elements one call of NumPy's reduction loop sees
struct PwStack {
    uint64_t off[PW_DEPTH], len[PW_DEPTH];
    double left[PW_DEPTH];
    uint32_t state[PW_DEPTH];   // 0 new, 1 waiting for the left half, 2 waiting for the right half
};

__device__ double phk_np_pairwise_sum(const double *a, uint64_t n, PwStack &st) {
    int sp = 0;
    st.off[0] = 0; st.len[0] = n; st.state[0] = 0;
    double ret = 0.0;
    while (sp >= 0) {
        const uint64_t o = st.off[sp], m = st.len[sp];
        const uint32_t state = st.state[sp];
        if (state == 0) {
            if (m <= 128) {
                ret = phk_np_pairwise_leaf(a + o, m);
                --sp;
            } else {
                uint64_t n2 = m / 2;
                n2 -= n2 % 8;
                st.state[sp] = 1;
                ++sp;
                st.off[sp] = o; st.len[sp] = n2; st.state[sp] = 0;
            }
        } else if (state == 1) {
            uint64_t n2 = m / 2;
            n2 -= n2 % 8;
            st.left[sp] = ret;
            st.state[sp] = 2;
            ++sp;
            st.off[sp] = o + n2; st.len[sp] = m - n2; st.state[sp] = 0;
        } else {
            ret = st.left[sp] + ret;
            --sp;
        }
    }
    return ret;
}

__global__ __launch_bounds__(256) void phk_normalize_f64_kernel(const double *__restrict__ rows, uint64_t n,
                                                                uint64_t D, double *__restrict__ out) {
    __shared__ PwStack stacks[4];
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t total = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n; r += total) {
        const double *row = rows + r * D;
        double s = 0.0;
        if (lane == 0) {
            // NumPy hands its reduction loop at most PW_NP_BUFSIZE elements at a time: each piece is summed pairwise and
            // the pieces' sums are added to the first piece's one after another
            s = phk_np_pairwise_sum(row, D < PW_NP_BUFSIZE ? D : PW_NP_BUFSIZE, stacks[threadIdx.x >> 6]);
            for (uint64_t o = PW_NP_BUFSIZE; o < D; o += PW_NP_BUFSIZE)
                s += phk_np_pairwise_sum(row + o, D - o < PW_NP_BUFSIZE ? D - o : PW_NP_BUFSIZE, stacks[threadIdx.x >> 6]);
        }
        s = __shfl(s, 0);
        for (uint64_t j = lane; j < D; j += 64) out[r * D + j] = row[j] / s;
    }
}

static unsigned norm_blocks(phk_ctx *ctx, uint64_t n) {
    uint64_t blocks = phk_div_up(n, 4);
    if (blocks > (uint64_t)ctx->num_cus * 8) blocks = (uint64_t)ctx->num_cus * 8;
    return (unsigned)blocks;
}

int phk_launch_normalize_u32(phk_ctx *ctx, const uint32_t *d_counts, uint64_t n, uint64_t D,
                             double *d_out) {
    if (n == 0 || D == 0) return PHK_OK;
    PHK_LAUNCH(ctx, "phk_normalize_int_kernel",
               phk_normalize_int_kernel<uint32_t><<<dim3(norm_blocks(ctx, n)), dim3(256), 0, ctx->stream>>>(
                   d_counts, n, D, d_out));
    return PHK_OK;
}

int phk_launch_normalize_i64(phk_ctx *ctx, const int64_t *d_counts, uint64_t n, uint64_t D,
                             double *d_out) {
    if (n == 0 || D == 0) return PHK_OK;
    PHK_LAUNCH(ctx, "phk_normalize_int_kernel",
               phk_normalize_int_kernel<int64_t><<<dim3(norm_blocks(ctx, n)), dim3(256), 0, ctx->stream>>>(
                   d_counts, n, D, d_out));
    return PHK_OK;
}

int phk_launch_normalize_f64(phk_ctx *ctx, const double *d_rows, uint64_t n, uint64_t D,
                             double *d_out) {
    if (n == 0 || D == 0) return PHK_OK;
    PHK_LAUNCH(ctx, "phk_normalize_f64_kernel",
               phk_normalize_f64_kernel<<<dim3(norm_blocks(ctx, n)), dim3(256), 0, ctx->stream>>>(
                   d_rows, n, D, d_out));
    return PHK_OK;
}

// ------------------------------------------------------------------------------------
// column gather: out[r][j] = in[r][perm[j]]  (reverse / complement / reverse-complement count vectors,
// scripts/transform_kmers.py:68-88)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void phk_permute_columns_kernel(const int64_t *__restrict__ in, uint64_t n, uint64_t D,
                                                                  const uint32_t *__restrict__ perm,
                                                                  int64_t *__restrict__ out) {
    const uint64_t total = n * D;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / D, j = i % D;
        out[i] = in[r * D + perm[j]];
    }
}

int phk_launch_permute_columns(phk_ctx *ctx, const int64_t *d_in, uint64_t n, uint64_t D, const uint32_t *d_perm,
                               int64_t *d_out) {
    if (n == 0 || D == 0) return PHK_OK;
    uint64_t blocks = phk_div_up(n * D, 256);
    if (blocks > (uint64_t)ctx->num_cus * 16) blocks = (uint64_t)ctx->num_cus * 16;
    PHK_LAUNCH(ctx, "phk_permute_columns_kernel",
               phk_permute_columns_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(d_in, n, D, d_perm, d_out));
    return PHK_OK;
}

// ------------------------------------------------------------------------------------
// verification helper: row sums against an expected value and word-wise comparison of two count matrices,
// both on the device (full-size batches are tens of GB: they are never brought to the host to be checked)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void phk_check_counts_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                               uint64_t n, uint64_t D, unsigned long long expect,
                                                               unsigned long long *__restrict__ result) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t total = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long bad_rows = 0, bad_words = 0;
    for (uint64_t r = wave; r < n; r += total) {
        unsigned long long s = 0, diff = 0;
        for (uint64_t j = lane; j < D; j += 64) {
            const uint32_t x = a[r * D + j];
            s += x;
            if (b) diff += x != b[r * D + j];
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            s += __shfl_xor(s, sh);
            diff += __shfl_xor(diff, sh);
        }
        bad_rows += (expect != ~0ull && s != expect) ? 1 : 0;
        bad_words += diff;
    }
    if (lane == 0) {
        if (bad_rows) atomicAdd(result, bad_rows);
        if (bad_words) atomicAdd(result + 1, bad_words);
    }
}

int phk_launch_check_counts(phk_ctx *ctx, const uint32_t *d_counts, const uint32_t *d_other, uint64_t n, uint64_t D,
                            uint64_t expected_rowsum, uint64_t *d_result) {
    PHK_REQUIRE(d_result && (n == 0 || d_counts), "phk_check_counts_dev: NULL pointer");
    PHK_HIP(hipMemsetAsync(d_result, 0, 2 * sizeof(uint64_t), ctx->stream));
    if (n == 0 || D == 0) return PHK_OK;
    uint64_t blocks = phk_div_up(n, 4);
    if (blocks > (uint64_t)ctx->num_cus * 16) blocks = (uint64_t)ctx->num_cus * 16;
    PHK_LAUNCH(ctx, "phk_check_counts_kernel",
               phk_check_counts_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(
                   d_counts, d_other, n, D, (unsigned long long)expected_rowsum, (unsigned long long *)d_result));
    return PHK_OK;
}
