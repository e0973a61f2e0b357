// probe_mfma_f64.hip -- the sustained rate of v_mfma_f64_16x16x4_f64 on this device, and its C/D layout.
// Build: hipcc --offload-arch=gfx950 -O2 -Wno-unused-value tools/probe_mfma_f64.hip -o tools/probe_mfma_f64 ; run on the GPU box.
// Rate: every wave issues chains of back-to-back MFMAs into 8 independent accumulators (no memory traffic in the loop);
// grid = CUs x 4 SIMDs x waves per SIMD; FLOP = waves x iterations x 8 x (16 x 16 x 4 x 2).
// Layout: A[i][k] = i + 1 at k = 0 only, B[k][j] = 100 (j + 1) at k = 0 only, so D[i][j] = 100 (i + 1)(j + 1) -- asymmetric, and
// each lane's four results name their own row and column.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void rate(double *out, int iters, double a0, double b0) {
    const int lane = threadIdx.x & 63;
    double a = a0 + lane * 1e-3, b = b0 - lane * 1e-3;
    f64x4 c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = (f64x4){0, 0, 0, 0};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c[j], 0, 0, 0);
    }
    f64x4 s = c[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) s += c[j];
    if (s[0] == 12345.678) out[blockIdx.x] = s[1] + s[2] + s[3];   // keeps the chains live; never true for these inputs
}

__global__ void layout(double *D) {
    const int lane = threadIdx.x, i = lane & 15, k = lane >> 4;
    const double a = k == 0 ? i + 1.0 : 0.0, b = k == 0 ? 100.0 * (i + 1) : 0.0;   // A[i][k] / B[k][j = i]
    f64x4 c = {0, 0, 0, 0};
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    for (int r = 0; r < 4; ++r) D[lane * 4 + r] = c[r];
}

int main() {   // (return codes unchecked: a failed call shows as a wrong layout count or an absurd rate)
    int dev = 0, cus = 0, clk = 0;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, dev);
    double *d_out, *d_lay;
    hipMalloc(&d_out, 1 << 20);
    hipMalloc(&d_lay, 256 * sizeof(double));
    layout<<<1, 64>>>(d_lay);
    double h[256];
    hipMemcpy(h, d_lay, sizeof(h), hipMemcpyDeviceToHost);
    int ok_doc = 0;   // C/D: col = lane & 15, row = (lane >> 4) + 4 reg
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) ok_doc += h[l * 4 + r] == 100.0 * ((l >> 4) + 4 * r + 1) * ((l & 15) + 1);
    printf("{\"layout_col_lane15_row_lane4_plus_4reg\": \"%d/256\"", ok_doc);
    const int iters = 20000;
    for (int wps = 1; wps <= 4; wps *= 2) {
        const int blocks = cus * wps;   // 256 threads = 4 waves = one per SIMD
        rate<<<blocks, 256>>>(d_out, 100, 1.0, 2.0);
        hipDeviceSynchronize();
        hipEvent_t e0, e1;
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        hipEventRecord(e0);
        rate<<<blocks, 256>>>(d_out, iters, 1.0, 2.0);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        const double flop = (double)blocks * 4 * iters * 8 * (16.0 * 16 * 4 * 2);
        const double cyc_per_mfma = (ms * 1e-3) * (clk * 1e3) / ((double)iters * 8 * wps);
        printf(", \"waves_per_simd_%d\": {\"ms\": %.3f, \"tflops\": %.2f, \"cycles_per_mfma_per_simd\": %.1f}", wps, ms,
               flop / (ms * 1e-3) / 1e12, cyc_per_mfma);
    }
    printf(", \"cus\": %d, \"clock_khz\": %d}\n", cus, clk);
    return 0;
}
