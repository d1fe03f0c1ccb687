// gfx950 (MI355X / CDNA4): luma of an RGB image view (mz_color.h) -- the streaming kernel and the launcher of one mz_luma() call, and
// the luma metrics (mz_metrics.h with C = 1): the plane kernel, the one-plane instantiations of the metrics kernels, their launcher.
#include <hip/hip_runtime.h>

#define MZ_METRICS_KERNELS
#include "mz_color.h"
#include "mz_metrics.h"

namespace mz {

constexpr int kLumaThreads = 256;
static_assert(kLumaThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");

// Work item i of B * H * chunks: one run of kVec<E> output elements (16 bytes) along a row, run fastest, then the row, then the image.
// vec: both views have a column stride of 1 and 16-byte aligned rows (the launcher's finding): three 16-byte loads, one store16; a row's
// last, partial run and every run of other views go element by element.  No LDS, no scratch; 64-bit signed addresses throughout.
template <int E>
__global__ __launch_bounds__(kLumaThreads) void luma_kernel(const StridedView x, const StridedView out, int H, int W, int chunks, long long items,
                                                             const LumaCoeffs k, int clamp, int vec) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long item = (long long)blockIdx.x * kLumaThreads + threadIdx.x;
    if (item >= items) return;
    long long b;
    int y, j;
    if (items <= 0x7fffffffLL) {  // (uniform) the usual case: 32-bit divisions
        const uint32_t it = (uint32_t)item, row = it / (uint32_t)chunks;
        j = (int)(it - row * (uint32_t)chunks) * V;
        b = row / (uint32_t)H;
        y = (int)(row - (uint32_t)b * (uint32_t)H);
    } else {
        const long long row = item / chunks;
        j = (int)(item - row * chunks) * V;
        b = row / H;
        y = (int)(row - b * H);
    }
    const long long xb = b * x.s[0] + (long long)y * x.s[2], ob = b * out.s[0] + (long long)y * out.s[2];
    if (vec && j + V <= W) {  // (x.s[3] == out.s[3] == 1; j is a multiple of the run: aligned once base and strides are)
        const char* p = (const char*)x.data + (xb + j) * EB;
        const u32x4 r = *(const u32x4*)p, g = *(const u32x4*)(p + x.s[1] * EB), bl = *(const u32x4*)(p + 2 * x.s[1] * EB);
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const double yv = luma_of(k, f64_of_raw<E>(vec_get<E>(r, e)), f64_of_raw<E>(vec_get<E>(g, e)), f64_of_raw<E>(vec_get<E>(bl, e)));
            vec_put<E>(v, e, luma_round_raw<E>(yv, clamp));
        }
        store16((char*)out.data + (ob + j) * EB, v);
    } else {
        for (int e = 0; e < V && j + e < W; ++e)
            st_raw<E>((void*)out.data, ob + (long long)(j + e) * out.s[3], luma_round_raw<E>(luma_at<E>(x, xb + (long long)(j + e) * x.s[3], k), clamp));
    }
}

int launch_luma(const LumaArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        const int chunks = (int)(((long long)a.W + kVec<E> - 1) / kVec<E>);
        const __int128 items = (__int128)a.B * a.H * chunks, blocks = (items + kLumaThreads - 1) / kLumaThreads;
        if (items < 1 || blocks > kGridRowMax) return hipErrorInvalidValue;
        StridedView o = a.out;
        o.s[1] = 0;  // one channel: its stride names nothing
        const bool vec = a.x.s[3] == 1 && o.s[3] == 1 && rows_aligned(a.x, a.B, a.H, kElemBytes<E>, 16) && rows_aligned(o, a.B, a.H, kElemBytes<E>, 16);
        hipLaunchKernelGGL((luma_kernel<E>), dim3((unsigned)blocks), dim3(kLumaThreads), 0, (hipStream_t)hip_stream, a.x, a.out, a.H, a.W, chunks,
                           (long long)items, luma_coeffs(a.standard), a.clamp, vec ? 1 : 0);
        return hipGetLastError();
    });
}

// mz_metrics_luma: the Y planes of both views into the workspace, then the C = 1 call on them
template <int E> static hipError_t launch_metrics_luma_e(const MetricsArgs& a, hipStream_t s) {
    const long long hw = (long long)a.H * a.W, blocks = (hw + kMetricsThreads - 1) / kMetricsThreads;
    if (!grid_ok(blocks, a.B)) return hipErrorInvalidValue;
    double* yp = (double*)(a.ws + a.plan.off_luma);
    double* yt = yp + (size_t)a.B * hw;
    hipLaunchKernelGGL((luma_planes_kernel<E>), dim3((unsigned)(blocks * a.B)), dim3(kMetricsThreads), 0, s, a.pred, a.target, a.H, a.W, blocks,
                       luma_coeffs(a.standard), yp, yt);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    MetricsArgs y = a;
    y.pred = dense_view(yp, a.H, a.W, 1);
    y.target = dense_view(yt, a.H, a.W, 1);
    return launch_metrics_e<EL_F64, 1>(y, s);
}

hipError_t launch_metrics_luma(const MetricsArgs& a, hipStream_t s) {
    return for_elem(a.elem, [&](auto e) { return launch_metrics_luma_e<decltype(e)::value>(a, s); });
}

}  // namespace mz
