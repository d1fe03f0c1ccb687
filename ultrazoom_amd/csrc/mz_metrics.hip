// gfx950 (MI355X / CDNA4): the image-quality metrics family (mz_metrics.h) -- instantiations and the launcher of one mz_metrics() call.
#define MZ_METRICS_KERNELS
#include "mz_metrics.h"

namespace mz {

// grid B: the partials of image b in a fixed order (thread i: partials i, i + 256; then the tree)
__global__ __launch_bounds__(kMetricsThreads) void psnr_reduce_kernel(const double* part, int blocks, double numel, double* out) {
    __shared__ double sh[kMetricsThreads];
    const long long b = blockIdx.x;
    double sq = 0.0, pmin = __builtin_inf(), pmax = -__builtin_inf(), tmin = __builtin_inf(), tmax = -__builtin_inf();
    for (int i = threadIdx.x; i < blocks; i += kMetricsThreads) {
        const double* q = part + (b * blocks + i) * 5;
        sq += q[0];
        pmin = OpMin::f(pmin, q[1]);
        pmax = OpMax::f(pmax, q[2]);
        tmin = OpMin::f(tmin, q[3]);
        tmax = OpMax::f(tmax, q[4]);
    }
    sq = block_reduce<OpSum>(sq, sh);
    pmin = block_reduce<OpMin>(pmin, sh);
    pmax = block_reduce<OpMax>(pmax, sh);
    tmin = block_reduce<OpMin>(tmin, sh);
    tmax = block_reduce<OpMax>(tmax, sh);
    if (threadIdx.x == 0) {
        double* o = out + b * kMetricSlots;
        o[MS_SQ_ERR] = sq;
        o[MS_NUMEL] = numel;
        o[MS_P_MIN] = pmin;
        o[MS_P_MAX] = pmax;
        o[MS_T_MIN] = tmin;
        o[MS_T_MAX] = tmax;
    }
}

// one thread: max(p.max() - p.min(), t.max() - t.min()) over the whole batch, as ssim_per_image's data_range=None
__global__ void range_kernel(const double* out, int B, double* range) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double pmin = __builtin_inf(), pmax = -__builtin_inf(), tmin = __builtin_inf(), tmax = -__builtin_inf();
    for (int b = 0; b < B; ++b) {
        const double* o = out + (long long)b * kMetricSlots;
        pmin = OpMin::f(pmin, o[MS_P_MIN]);
        pmax = OpMax::f(pmax, o[MS_P_MAX]);
        tmin = OpMin::f(tmin, o[MS_T_MIN]);
        tmax = OpMax::f(tmax, o[MS_T_MAX]);
    }
    *range = OpMax::f(pmax - pmin, tmax - tmin);
}

hipError_t launch_psnr_reduce(const double* part, int blocks, double numel, double* out, int B, hipStream_t s) {
    hipLaunchKernelGGL(psnr_reduce_kernel, dim3(B), dim3(kMetricsThreads), 0, s, part, blocks, numel, out);
    return hipGetLastError();
}
hipError_t launch_range(const double* out, int B, double* range, hipStream_t s) {
    hipLaunchKernelGGL(range_kernel, dim3(1), dim3(64), 0, s, out, B, range);
    return hipGetLastError();
}

hipError_t launch_metrics(const MetricsArgs& a, hipStream_t s) {
    return for_elem(a.elem, [&](auto e) { return launch_metrics_e<decltype(e)::value, 3>(a, s); });
}

}  // namespace mz
