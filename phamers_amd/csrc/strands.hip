// strands.hip -- strand-symmetric counts: a count row added to its reverse-complement permutation.
//
// An assembler emits a contig on an arbitrary strand, and the count kernels (count_wave.hip, count_slots.hip, windows.hip) restate the
// reference's single-strand window loop (scripts/kmer.py:32-79).  The fold F[c] = C[c] + C[rc(c)], rc(c) = the column of
// the reverse-complement k-mer, is what counting the sequence AND its reverse complement gives -- for every string,
// invalid characters included, because a window holds an invalid character exactly when its mirror image does -- so
// fold(count(s)) == fold(count(revcomp(s))) and everything computed from folded rows is the same for the two strands.
//
// rc pairs the base-4 digits 0 <-> 1 and 2 <-> 3 and reverses their order: with the symbol orders the package counts
// over, 'ATGC' (DNA) and 'AUGC' (RNA), that is A <-> T(U), G <-> C.  It is transform_kmers.exact_indices(k, True, True),
// an involution, with 4^(k/2) fixed points (palindromes) at even k and none at odd k.
//
// phk_batch_fold_strands works on the RESIDENT rows of a batch, whatever produced them, in place (a batch can be most of
// the device's memory).  One wave (k <= 6) or one workgroup (k = 7, a 64 KB row) owns a whole row: it reads the row into
// LDS -- every element from HBM once, 16 bytes per lane and instruction -- and only when all of it has arrived writes the
// sums back, the partner of every element coming from LDS.  No row is read while another owner writes it.
#include "phk_common.h"

#define PHK_FOLD_BLOCKS_MAX 2048u   // 256 threads each: the grid of the fold kernel (more rows are taken by its grid-stride loop)

// column of the reverse-complement k-mer: the K base-4 digits of c reversed, bit 0 of each flipped
__device__ __forceinline__ uint32_t fold_rc(uint32_t c, int K) {
    uint32_t x = __brev(c);   // the digits reversed (into the top 2 K bits), the two bits of each digit swapped as well ...
    x = ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);   // ... and swapped back
    return (x >> (32 - 2 * K)) ^ (0x55555555u >> (32 - 2 * K));
}

template <int GROUP>
__device__ __forceinline__ void fold_sync() {
    if (GROUP == 64) {   // the row's owner is one wave: its LDS accesses are ordered, the compiler must keep them so
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// rows with a sum of 2^31 or more: doubling them would wrap
__global__ __launch_bounds__(256) void phk_fold_check_kernel(const uint32_t *__restrict__ nwin, uint64_t n,
                                                             uint32_t *__restrict__ over) {
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        bad += nwin[i] >> 31;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) bad += __shfl_xor(bad, sh);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(over, bad);
}

// GROUP threads own a row of D = 4^K words: 256 / GROUP rows per workgroup, each with D words of the dynamic LDS.
// (The trip count of the row loop is the same for every thread of a GROUP, so the barriers inside it are met by all.)
template <int K, int GROUP>
__global__ __launch_bounds__(256) void phk_fold_strands_kernel(uint32_t *counts, uint32_t *nwin, uint64_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fold_lds[];
    constexpr uint32_t D = 1u << (2 * K), V = D / 4;   // V 16-byte pieces per row
    constexpr uint32_t RPB = 256 / GROUP;
    const uint32_t t = threadIdx.x % GROUP, g = threadIdx.x / GROUP;
    uint32_t *row = fold_lds + g * D;
    uint4 *row4 = reinterpret_cast<uint4 *>(row);
    for (uint64_t r = (uint64_t)blockIdx.x * RPB + g; r < n; r += (uint64_t)gridDim.x * RPB) {
        uint4 *grow = reinterpret_cast<uint4 *>(counts + r * D);
        for (uint32_t i = t; i < V; i += GROUP) row4[i] = grow[i];
        fold_sync<GROUP>();   // the whole row is in LDS: from here on it may be overwritten in HBM
        for (uint32_t i = t; i < V; i += GROUP) {
            uint4 v = row4[i];
            v.x += row[fold_rc(4 * i + 0, K)];
            v.y += row[fold_rc(4 * i + 1, K)];
            v.z += row[fold_rc(4 * i + 2, K)];
            v.w += row[fold_rc(4 * i + 3, K)];
            grow[i] = v;
        }
        if (t == 0) nwin[r] = nwin[r] * 2u;
        fold_sync<GROUP>();   // (the next row of this owner replaces the LDS image)
    }
}

static uint64_t fold_rows_per_block(int k) { return k <= 6 ? 4 : 1; }

extern "C" int phk_fold_grid_pass(int k, uint64_t *rows) {
    PHK_REQUIRE(rows && k >= 1 && k <= PHK_MAX_K, "phk_fold_grid_pass: bad argument");
    *rows = (uint64_t)PHK_FOLD_BLOCKS_MAX * fold_rows_per_block(k);
    return PHK_OK;
}

template <int K>
static int fold_launch(phk_ctx *ctx, uint32_t *d_counts, uint32_t *d_nwin, uint64_t n) {
    constexpr int GROUP = K <= 6 ? 64 : 256;
    constexpr uint32_t RPB = 256 / GROUP;
    uint64_t blocks = phk_div_up(n, RPB);
    if (blocks > PHK_FOLD_BLOCKS_MAX) blocks = PHK_FOLD_BLOCKS_MAX;
    const size_t lds = (size_t)RPB * phk_pow4(K) * sizeof(uint32_t);   // 64 KiB at most (k = 6: four rows; k = 7: one)
    PHK_LAUNCH(ctx, "phk_fold_strands_kernel",
               phk_fold_strands_kernel<K, GROUP><<<dim3((unsigned)blocks), dim3(256), lds, ctx->stream>>>(d_counts, d_nwin, n));
    return PHK_OK;
}

extern "C" int phk_batch_fold_strands(phk_ctx *ctx, phk_batch *b) {
    PHK_ENTER(ctx, "phk_batch_fold_strands");
    PHK_REQUIRE(b, "phk_batch_fold_strands: NULL batch");
    PHK_REQUIRE(!b->folded, "phk_batch_fold_strands: the batch is folded already");
    PHK_REQUIRE(b->k >= 1 && b->k <= PHK_MAX_K && b->D == phk_pow4(b->k), "phk_batch_fold_strands: not a batch of 4^k columns");
    if (b->n == 0) {
        b->folded = true;
        return PHK_OK;
    }
    void *d_over;
    PHK_TRY(phk_ws(ctx, WS_FLAGS, 64, &d_over));
    PHK_HIP(hipMemsetAsync(d_over, 0, 4, ctx->stream));
    uint64_t blocks = phk_div_up(b->n, 256);
    if (blocks > (uint64_t)ctx->num_cus * 16) blocks = (uint64_t)ctx->num_cus * 16;
    PHK_LAUNCH(ctx, "phk_fold_check_kernel",
               phk_fold_check_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(b->d_nwin, b->n, (uint32_t *)d_over));
    uint32_t over = 0;
    PHK_HIP(hipMemcpyAsync(&over, d_over, 4, hipMemcpyDeviceToHost, ctx->stream));
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    if (over) {   // nothing has been written
        phk_set_error("phk_batch_fold_strands: the sum of %u row(s) is 2^31 or more and cannot be doubled in 32 bits", over);
        return PHK_ERR_UNSUPPORTED;
    }
    switch (b->k) {
        case 1: PHK_TRY(fold_launch<1>(ctx, b->d_counts, b->d_nwin, b->n)); break;
        case 2: PHK_TRY(fold_launch<2>(ctx, b->d_counts, b->d_nwin, b->n)); break;
        case 3: PHK_TRY(fold_launch<3>(ctx, b->d_counts, b->d_nwin, b->n)); break;
        case 4: PHK_TRY(fold_launch<4>(ctx, b->d_counts, b->d_nwin, b->n)); break;
        case 5: PHK_TRY(fold_launch<5>(ctx, b->d_counts, b->d_nwin, b->n)); break;
        case 6: PHK_TRY(fold_launch<6>(ctx, b->d_counts, b->d_nwin, b->n)); break;
        default: PHK_TRY(fold_launch<7>(ctx, b->d_counts, b->d_nwin, b->n)); break;
    }
    PHK_HIP(hipStreamSynchronize(ctx->stream));
    b->folded = true;
    return PHK_OK;
}

extern "C" int phk_batch_strands(const phk_batch *b, int *folded) {
    PHK_REQUIRE(b && folded, "phk_batch_strands: NULL");
    *folded = b->folded ? 1 : 0;
    return PHK_OK;
}

// ---- the same transform for an int64 matrix of the host (beside phk_permute_columns_i64): no 32-bit limit ----
__global__ __launch_bounds__(256) void phk_fold_i64_kernel(const int64_t *__restrict__ in, uint64_t n, int K,
                                                           int64_t *__restrict__ out) {
    const uint64_t total = n << (2 * K);
    const uint32_t dmask = (1u << (2 * K)) - 1u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = (uint32_t)i & dmask;
        out[i] = (int64_t)((uint64_t)in[i] + (uint64_t)in[i - c + fold_rc(c, K)]);
    }
}

extern "C" int phk_fold_strands_i64(phk_ctx *ctx, const int64_t *counts, uint64_t n, uint64_t D, int64_t *out) {
    PHK_ENTER(ctx, "phk_fold_strands_i64");
    int k = 0;
    while (k <= PHK_MAX_K && phk_pow4(k) != D) ++k;
    if (k < 1 || k > PHK_MAX_K) {
        phk_set_error("phk_fold_strands_i64: %llu columns is not 4^k for 1 <= k <= %d", (unsigned long long)D, PHK_MAX_K);
        return PHK_ERR_UNSUPPORTED;
    }
    if (n == 0) return PHK_OK;
    PHK_REQUIRE(counts && out, "phk_fold_strands_i64: NULL pointer");
    void *d_in, *d_out;
    PHK_TRY(phk_ws(ctx, WS_WIDE, n * D * 8, &d_in));
    PHK_TRY(phk_ws(ctx, WS_Q64, n * D * 8, &d_out));
    PHK_TRY(phk_copy_to_device(ctx, d_in, counts, n * D * 8));
    uint64_t blocks = phk_div_up(n * D, 256);
    if (blocks > (uint64_t)ctx->num_cus * 16) blocks = (uint64_t)ctx->num_cus * 16;
    PHK_LAUNCH(ctx, "phk_fold_i64_kernel",
               phk_fold_i64_kernel<<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>((const int64_t *)d_in, n, k, (int64_t *)d_out));
    return phk_copy_to_host(ctx, out, d_out, n * D * 8);
}
