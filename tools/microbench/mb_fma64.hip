// Micro-benchmark: what does THIS MI355X sustain on dependent-free float64 FMAs (v_fma_f64), and how much is left when every FMA takes one
// operand from LDS?  The denominators for the metrics kernels' float64 rate (EXPERIMENTS.md, metrics entry; tools/metrics_bench.py).
//   regs   16 independent accumulators per lane, operands in registers
//   lds    the same, one multiplicand per FMA read from LDS (ds_read_b64, conflict-free), as moments_kernel's vertical pass
// Build: hipcc --offload-arch=gfx950 -O3 mb_fma64.hip -o mb_fma64      Output: one JSON object per line.
#include <hip/hip_runtime.h>

#include <cstdio>

#define CHECK(x)                                                    \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) {                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            return 1;                                               \
        }                                                           \
    } while (0)

constexpr int ACC = 16, ITERS = 4096;

template <bool LDS> __global__ __launch_bounds__(256) void fma_kernel(double* out, double a, double b) {
    __shared__ double sh[ACC * 256];
    for (int k = 0; k < ACC; ++k) sh[k * 256 + threadIdx.x] = b + k;
    __syncthreads();
    double acc[ACC];
#pragma unroll
    for (int k = 0; k < ACC; ++k) acc[k] = threadIdx.x + k;
    for (int i = 0; i < ITERS; ++i) {
#pragma unroll
        for (int k = 0; k < ACC; ++k) {
            if constexpr (LDS) acc[k] = fma(a, ((volatile double*)sh)[k * 256 + threadIdx.x], acc[k]);
            else acc[k] = fma(a, acc[k], b);
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < ACC; ++k) s += acc[k];
    out[(long long)blockIdx.x * 256 + threadIdx.x] = s;
}

template <bool LDS> static int run(const char* name, double* out, int blocks) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(fma_kernel<LDS>, dim3(blocks), dim3(256), 0, 0, out, 1.0000001, 1e-9);
    CHECK(hipDeviceSynchronize());
    const int reps = 10;
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(fma_kernel<LDS>, dim3(blocks), dim3(256), 0, 0, out, 1.0000001, 1e-9);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    const double fmas = (double)reps * blocks * 256.0 * ITERS * ACC;
    printf("{\"bench\": \"fma64_%s\", \"blocks\": %d, \"ms\": %.4f, \"tfma_per_s\": %.3f}\n", name, blocks, ms / reps, fmas / (ms * 1e-3) / 1e12);
    return 0;
}

int main() {
    int cus = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const int blocks = cus * 8;  // eight workgroups of four waves per CU: every SIMD full
    double* out = nullptr;
    CHECK(hipMalloc(&out, (size_t)blocks * 256 * sizeof(double)));
    if (run<false>("regs", out, blocks)) return 1;
    if (run<true>("lds", out, blocks)) return 1;
    CHECK(hipFree(out));
    return 0;
}
