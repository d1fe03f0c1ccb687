// gfx950 (MI355X / CDNA4): the image-quality metrics family (mz_metrics.h) -- instantiations and the launcher of one mz_metrics() call.
#define MZ_METRICS_KERNELS
#include "mz_metrics.h"

#include <cassert>
#include <cmath>

namespace mz {

// g / g.sum() of evaluate.py's _gaussian_window, in double (the 2-D VIF window normalised in 2-D is its outer product)
static MetricsTaps gaussian_taps(int n, double sigma) {
    MetricsTaps t = {};
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) / 2.0;
        t.w[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
        sum += t.w[i];
    }
    for (int i = 0; i < n; ++i) t.w[i] /= sum;
    return t;
}

template <int E, int T, int EPI>
static hipError_t launch_moments(const StridedView& p, const StridedView& t, int B, int H, int W, long long tiles, const MetricsTaps& taps,
                                 double param, const double* range_dev, double* part, hipStream_t s) {
    TileGrid g;  // of the (H - T + 1) x (W - T + 1) map; `tiles` is the plan's count (the workspace is laid out by it)
    if (!plane_tile_grid(H - T + 1, W - T + 1, kMetricsTileH, kMetricsTileW, B, &g)) return hipErrorInvalidValue;
    assert(g.tiles == tiles);
    hipLaunchKernelGGL((moments_kernel<E, T, EPI>), dim3((unsigned)g.wgs), dim3(kMetricsThreads), 0, s, p, t, H, W, tiles, g.tiles_x, taps, param,
                       range_dev, part);
    return hipGetLastError();
}

template <int E, int T>
static hipError_t launch_down(const StridedView& p, const StridedView& t, int B, int Ho, int Wo, double* outp, double* outt, hipStream_t s) {
    const long long blocks = ((long long)Ho * Wo + kMetricsThreads - 1) / kMetricsThreads;
    if (!grid_ok(blocks, 3LL * B)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((down_kernel<E, T>), dim3((unsigned)(blocks * 3 * B)), dim3(kMetricsThreads), 0, s, p, t, Ho, Wo, blocks,
                       gaussian_taps(T, T / 5.0), outp, outt);
    return hipGetLastError();
}

template <int E> static hipError_t launch_metrics_e(const MetricsArgs& a, hipStream_t s) {
    const MetricsPlan& pl = a.plan;
    hipError_t e = hipSuccess;
    double* range_dev = (double*)(a.ws + pl.off_range);
    const bool batch_range = (a.which & MET_SSIM) && !(a.data_range > 0.0);
    if ((a.which & MET_PSNR) || batch_range) {
        double* part = (double*)(a.ws + pl.off_psnr);
        if (a.B > 65535) return hipErrorInvalidValue;
        hipLaunchKernelGGL((psnr_kernel<E>), dim3(pl.psnr_blocks, a.B), dim3(kMetricsThreads), 0, s, a.pred, a.target, a.H, a.W, part);
        hipLaunchKernelGGL(psnr_reduce_kernel, dim3(a.B), dim3(kMetricsThreads), 0, s, (const double*)part, pl.psnr_blocks,
                           3.0 * (double)a.H * (double)a.W, a.out);
        if (batch_range) hipLaunchKernelGGL(range_kernel, dim3(1), dim3(64), 0, s, (const double*)a.out, a.B, range_dev);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.which & MET_SSIM) {
        e = launch_moments<E, 11, EPI_SSIM>(a.pred, a.target, a.B, a.H, a.W, pl.ssim_tiles, gaussian_taps(11, 1.5), a.data_range, range_dev,
                                            (double*)(a.ws + pl.off_ssim), s);
        if (e != hipSuccess) return e;
    }
    if (a.which & MET_VIF) {
        e = launch_moments<E, 17, EPI_VIF>(a.pred, a.target, a.B, a.H, a.W, pl.vif_tiles[0], gaussian_taps(17, 17 / 5.0), a.sigma_n_sq,
                                           nullptr, (double*)(a.ws + pl.off_vif[0]), s);
        if (e != hipSuccess) return e;
        double* pyr[4][2] = {};
        for (int k = 1; k < 4; ++k) {
            pyr[k][0] = (double*)(a.ws + pl.off_pyr[k]);
            pyr[k][1] = pyr[k][0] + (size_t)a.B * 3 * pl.vif_h[k] * pl.vif_w[k];
        }
        const StridedView p1 = dense_view(pyr[1][0], pl.vif_h[1], pl.vif_w[1]), t1 = dense_view(pyr[1][1], pl.vif_h[1], pl.vif_w[1]);
        const StridedView p2 = dense_view(pyr[2][0], pl.vif_h[2], pl.vif_w[2]), t2 = dense_view(pyr[2][1], pl.vif_h[2], pl.vif_w[2]);
        const StridedView p3 = dense_view(pyr[3][0], pl.vif_h[3], pl.vif_w[3]), t3 = dense_view(pyr[3][1], pl.vif_h[3], pl.vif_w[3]);
        if ((e = launch_down<E, 9>(a.pred, a.target, a.B, pl.vif_h[1], pl.vif_w[1], pyr[1][0], pyr[1][1], s)) != hipSuccess) return e;
        if ((e = launch_moments<EL_F64, 9, EPI_VIF>(p1, t1, a.B, pl.vif_h[1], pl.vif_w[1], pl.vif_tiles[1], gaussian_taps(9, 9 / 5.0), a.sigma_n_sq,
                                                    nullptr, (double*)(a.ws + pl.off_vif[1]), s)) != hipSuccess) return e;
        if ((e = launch_down<EL_F64, 5>(p1, t1, a.B, pl.vif_h[2], pl.vif_w[2], pyr[2][0], pyr[2][1], s)) != hipSuccess) return e;
        if ((e = launch_moments<EL_F64, 5, EPI_VIF>(p2, t2, a.B, pl.vif_h[2], pl.vif_w[2], pl.vif_tiles[2], gaussian_taps(5, 5 / 5.0), a.sigma_n_sq,
                                                    nullptr, (double*)(a.ws + pl.off_vif[2]), s)) != hipSuccess) return e;
        if ((e = launch_down<EL_F64, 3>(p2, t2, a.B, pl.vif_h[3], pl.vif_w[3], pyr[3][0], pyr[3][1], s)) != hipSuccess) return e;
        if ((e = launch_moments<EL_F64, 3, EPI_VIF>(p3, t3, a.B, pl.vif_h[3], pl.vif_w[3], pl.vif_tiles[3], gaussian_taps(3, 3 / 5.0), a.sigma_n_sq,
                                                    nullptr, (double*)(a.ws + pl.off_vif[3]), s)) != hipSuccess) return e;
    }
    if (a.which & (MET_SSIM | MET_VIF)) {
        MetricsFinishArgs f = {};
        f.which = a.which;
        f.ssim_part = (const double*)(a.ws + pl.off_ssim);
        f.ssim_tiles = pl.ssim_tiles;
        f.ssim_count = 3.0 * (double)(a.H - 10) * (double)(a.W - 10);
        f.fixed_range = a.data_range;
        f.range_dev = range_dev;
        for (int k = 0; k < 4; ++k) {
            f.vif_part[k] = (const double*)(a.ws + pl.off_vif[k]);
            f.vif_tiles[k] = pl.vif_tiles[k];
        }
        hipLaunchKernelGGL(finish_kernel, dim3(a.B), dim3(kMetricsThreads), 0, s, f, a.out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_metrics(const MetricsArgs& a, hipStream_t s) {
    return for_elem(a.elem, [&](auto e) { return launch_metrics_e<decltype(e)::value>(a, s); });
}

}  // namespace mz
