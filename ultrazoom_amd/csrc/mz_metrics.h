// Image-quality metrics of two image views: PSNR's squared error, SSIM and pixel-domain VIF (mz_metrics(), include/mewzoom_hip.h) --
// the arithmetic of ultrazoom_amd/evaluate.py (PSNR / ssim_per_image / vif_per_image) as gfx950 kernels.  No reference counterpart in
// model.py: the reference takes the three metrics from torchmetrics (pretrain.py:209-211, 301-329).
//
// Everything is float64: the inputs (f32, bf16, f16, uint8 / 255) are exact in it, and sigma = E[x^2] - mu^2 cancels against constants
// as small as (0.03 * range)^2 -- in float32 SSIM of a nearly flat pair collapses (EXPERIMENTS.md, metrics entry).
//
//   psnr_kernel        per image: sum (p - t)^2, min / max of p and of t         -> partials per workgroup
//   psnr_reduce_kernel the partials of an image in a fixed order                  -> out slots 0..5
//   range_kernel       SSIM's data_range=None: max(range of p, range of t) of the BATCH, on the device (no host synchronisation)
//   moments_kernel     <element type, taps, epilogue>: one workgroup = one 16 x 32 pixel tile of one channel of one image.  The tile and its
//                      (taps - 1) halo of both images are staged in LDS; a horizontal pass filters p, t, p^2, t^2, p t (four adjacent
//                      outputs per work item, so every product is formed once per staged row element), a vertical pass finishes the five
//                      windowed moments, the epilogue (SSIM map / VIF numerator and denominator logs) follows, then a workgroup sum.
//                      Only windows that lie wholly inside the image exist ("valid" filtering): torchmetrics' reflect-pad-by-5 and
//                      crop-by-5 leaves exactly those.
//   down_kernel        VIF scales 1..3: "valid" Gaussian filter + every second row and column, float64 into the workspace
//   finish_kernel      per image: the tile partials in a fixed order -> out slots 6.. (no floating-point atomics anywhere: two calls
//                      give the same bits, and an image's sums do not depend on the batch it is in)
// All address arithmetic is 64-bit and signed (element strides of a view may be negative and larger than 2^31).
//
// CHANNELS.  The plan, the arguments and the kernels carry a channel count C: 3 for mz_metrics, 1 for mz_metrics_luma, where
// luma_planes_kernel first writes the UNROUNDED float64 Y planes (mz_color.h) of both images, dense [B][1][H][W], into the workspace and
// the kernels above then run on those planes with E = EL_F64.  C is a template argument: the C = 3 kernels are compiled as before, in
// mz_metrics.hip; the C = 1 instantiations and luma_planes_kernel are compiled in mz_color.hip, the luma unit.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mz_color.h"
#include "mz_view.h"

namespace mz {

constexpr int kMetricsTileH = 16;   // output pixels of one moments_kernel workgroup
constexpr int kMetricsTileW = 32;
constexpr int kMetricsThreads = 256;
static_assert(kMetricsThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kMetricsRun = 4;      // adjacent outputs of one horizontal-pass work item
constexpr int kMetricsMaxTaps = 17;
constexpr int kMetricSlots = 16;    // == MZ_METRIC_SLOTS
constexpr int kPsnrBlocksMax = 512; // psnr_kernel workgroups per image (<= 2 * kMetricsThreads: psnr_reduce_kernel)

enum MetricBits : int { MET_PSNR = 1, MET_SSIM = 2, MET_VIF = 4 };
// out[b][slot]
enum MetricSlot : int {
    MS_SQ_ERR = 0, MS_NUMEL = 1, MS_P_MIN = 2, MS_P_MAX = 3, MS_T_MIN = 4, MS_T_MAX = 5, MS_SSIM_SUM = 6, MS_SSIM_COUNT = 7,
    MS_VIF_NUM = 8 /* ..10: per channel */, MS_VIF_DEN = 11 /* ..13 */, MS_SSIM_RANGE = 14
};

struct MetricsTaps {
    double w[kMetricsMaxTaps];  // the normalised 1-D Gaussian window, computed by the host in double
};

inline int vif_taps(int scale) { return (1 << (4 - scale)) + 1; }  // 17, 9, 5, 3
inline long long metrics_tiles(int H, int W, int taps) {
    const long long hv = H - taps + 1, wv = W - taps + 1;
    return ((hv + kMetricsTileH - 1) / kMetricsTileH) * ((wv + kMetricsTileW - 1) / kMetricsTileW);
}

// Workspace layout of one call (bytes from the start, every part 256-byte aligned); depends on B, H, W, which and C only.  C = 1 is the
// plan of mz_metrics_luma: the layout of one plane, and behind it the two Y planes (off_luma: p then t, float64 [B][1][H][W] each) --
// the workspace of a luma call is larger than that of one RGB plane by these 2 * 8 B H W bytes (rounded up to 256).
struct MetricsPlan {
    int C;                     // channels: 3, or 1 (luma)
    int psnr_blocks;           // psnr_kernel workgroups per image: a function of C H alone
    long long ssim_tiles;      // per channel
    int vif_h[4], vif_w[4];    // the image at each VIF scale
    long long vif_tiles[4];    // per channel
    size_t off_psnr, off_range, off_ssim, off_vif[4], off_pyr[4];  // off_pyr[s]: p then t of scale s, float64 [B][C][h][w] each (s = 1..3)
    size_t off_luma;           // C = 1 only
    size_t total;
};
// the two Y planes of a luma call fit a size_t worth allocating (2^62 bytes); every other part of the plan is smaller than they are
inline bool luma_planes_fit(int B, int H, int W) { return (__int128)16 * B * H * W <= ((__int128)1 << 62); }
inline MetricsPlan metrics_plan(int B, int H, int W, int which, int C = 3) {
    MetricsPlan p = {};
    p.C = C;
    auto take = [&](size_t bytes) {
        const size_t at = p.total;
        p.total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t planes = (size_t)B * C;
    p.psnr_blocks = C * (long long)H < kPsnrBlocksMax ? C * H : kPsnrBlocksMax;
    p.off_psnr = take((size_t)B * p.psnr_blocks * 5 * sizeof(double));
    p.off_range = take(sizeof(double));
    if (which & MET_SSIM) {
        p.ssim_tiles = metrics_tiles(H, W, 11);
        p.off_ssim = take(planes * p.ssim_tiles * sizeof(double));
    }
    if (which & MET_VIF) {
        p.vif_h[0] = H;
        p.vif_w[0] = W;
        for (int s = 0; s < 4; ++s) {
            const int n = vif_taps(s);
            if (s > 0) {  // "valid" filter, every second row and column
                p.vif_h[s] = (p.vif_h[s - 1] - n + 2) / 2;
                p.vif_w[s] = (p.vif_w[s - 1] - n + 2) / 2;
                p.off_pyr[s] = take(2 * planes * p.vif_h[s] * p.vif_w[s] * sizeof(double));
            }
            p.vif_tiles[s] = metrics_tiles(p.vif_h[s], p.vif_w[s], n);
            p.off_vif[s] = take(planes * p.vif_tiles[s] * 2 * sizeof(double));
        }
    }
    if (C == 1) p.off_luma = take(2 * planes * H * W * sizeof(double));
    return p;
}

struct MetricsArgs {
    StridedView pred, target;
    int elem;            // Elem 0..3
    int B, H, W;
    int standard;        // LumaStandard (plan.C == 1 only)
    int which;           // MetricBits
    double data_range;   // SSIM: > 0 fixed, <= 0 from the batch
    double sigma_n_sq;   // VIF
    double* out;         // [B][kMetricSlots]
    char* ws;
    MetricsPlan plan;
};
// Enqueues the whole call; hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch.  launch_metrics: mz_metrics (plan.C = 3,
// mz_metrics.hip); launch_metrics_luma: mz_metrics_luma (plan.C = 1; mz_color.hip, which compiles the C = 1 kernels)
hipError_t launch_metrics(const MetricsArgs& a, hipStream_t s);
hipError_t launch_metrics_luma(const MetricsArgs& a, hipStream_t s);

#ifdef MZ_METRICS_KERNELS  // mz_metrics.hip only: the host runtime includes the plan above without the device code

struct OpSum { static __device__ __forceinline__ double f(double a, double b) { return a + b; } };
struct OpMin { static __device__ __forceinline__ double f(double a, double b) { return b < a ? b : a; } };
struct OpMax { static __device__ __forceinline__ double f(double a, double b) { return b > a ? b : a; } };
// value of all kMetricsThreads threads combined in a fixed tree; sh: kMetricsThreads doubles, free again on return
template <class OP> __device__ __forceinline__ double block_reduce(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = kMetricsThreads / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = OP::f(sh[tid], sh[tid + s]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---- PSNR part ----------------------------------------------------------------------------------------------------------------------
// grid (psnr_blocks, B): workgroup i takes rows i, i + psnr_blocks, .. of the C H channel rows of its image
template <int E, int C = 3> __global__ __launch_bounds__(kMetricsThreads) void psnr_kernel(const StridedView p, const StridedView t, int H, int W,
                                                                                  double* part) {
    __shared__ double sh[kMetricsThreads];
    const long long b = blockIdx.y;
    double sq = 0.0, pmin = __builtin_inf(), pmax = -__builtin_inf(), tmin = __builtin_inf(), tmax = -__builtin_inf();
    for (int r = blockIdx.x; r < C * H; r += gridDim.x) {
        const long long c = r / H, y = r - c * H;
        const long long po = b * p.s[0] + c * p.s[1] + y * p.s[2], to = b * t.s[0] + c * t.s[1] + y * t.s[2];
        for (long long x = threadIdx.x; x < W; x += kMetricsThreads) {
            const double pv = ld_f64<E>(p.data, po + x * p.s[3]), tv = ld_f64<E>(t.data, to + x * t.s[3]);
            const double d = pv - tv;
            sq += d * d;
            pmin = OpMin::f(pmin, pv);
            pmax = OpMax::f(pmax, pv);
            tmin = OpMin::f(tmin, tv);
            tmax = OpMax::f(tmax, tv);
        }
    }
    sq = block_reduce<OpSum>(sq, sh);
    pmin = block_reduce<OpMin>(pmin, sh);
    pmax = block_reduce<OpMax>(pmax, sh);
    tmin = block_reduce<OpMin>(tmin, sh);
    tmax = block_reduce<OpMax>(tmax, sh);
    if (threadIdx.x == 0) {
        double* o = part + (b * gridDim.x + blockIdx.x) * 5;
        o[0] = sq;
        o[1] = pmin;
        o[2] = pmax;
        o[3] = tmin;
        o[4] = tmax;
    }
}

// psnr_reduce_kernel (grid B: the partials of image b in a fixed order -> out slots 0..5) and range_kernel (one thread: max(p.max() -
// p.min(), t.max() - t.min()) over the whole batch, as ssim_per_image's data_range=None) are no templates: mz_metrics.hip holds them, and
// these two launch them for every translation unit
hipError_t launch_psnr_reduce(const double* part, int blocks, double numel, double* out, int B, hipStream_t s);
hipError_t launch_range(const double* out, int B, double* range, hipStream_t s);

// ---- windowed moments + epilogue ------------------------------------------------------------------------------------------------------
enum MomentsEpilogue : int { EPI_SSIM = 0, EPI_VIF = 1 };

// SSIM map value of one pixel (ssim_per_image)
__device__ __forceinline__ double ssim_pixel(const double m[5], double c1, double c2) {
    const double mu_p = m[0], mu_t = m[1];
    const double s_pp = m[2] - mu_p * mu_p, s_tt = m[3] - mu_t * mu_t, s_pt = m[4] - mu_p * mu_t;
    return ((2.0 * mu_p * mu_t + c1) * (2.0 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2));
}
// numerator and denominator log of one pixel of one VIF scale (vif_per_image, line for line)
__device__ __forceinline__ void vif_pixel(const double m[5], double sigma_n_sq, double& num, double& den) {
    const double eps = 1e-10;
    const double mu_p = m[0], mu_t = m[1];
    double s_tt = OpMax::f(m[3] - mu_t * mu_t, 0.0);
    const double s_pp = OpMax::f(m[2] - mu_p * mu_p, 0.0);
    const double s_tp = m[4] - mu_t * mu_p;
    double g = s_tp / (s_tt + eps);
    double s_v = s_pp - g * s_tp;
    if (s_tt < eps) {
        g = 0.0;
        s_v = s_pp;
        s_tt = 0.0;
    }
    if (s_pp < eps) {
        g = 0.0;
        s_v = 0.0;
    }
    if (g < 0.0) {
        s_v = s_pp;
        g = 0.0;
    }
    s_v = OpMax::f(s_v, eps);
    num = log10(1.0 + g * g * s_tt / (s_v + sigma_n_sq));
    den = log10(1.0 + s_tt / sigma_n_sq);
}

// grid: tiles * C * B workgroups, tile fastest.  H, W: the image; the map is (H - T + 1) x (W - T + 1).
// param: EPI_SSIM the fixed data range (> 0) or <= 0 = read *range_dev; EPI_VIF sigma_n_sq.
// part: EPI_SSIM [B * C][tiles], EPI_VIF [B * C][tiles][2]
template <int E, int T, int EPI, int C = 3>
__global__ __launch_bounds__(kMetricsThreads) void moments_kernel(const StridedView p, const StridedView t, int H, int W, long long tiles,
                                                                    int tiles_x, const MetricsTaps taps, double param,
                                                                    const double* range_dev, double* part) {
    constexpr int TH = kMetricsTileH, TW = kMetricsTileW, R = kMetricsRun;
    constexpr int SH = TH + T - 1, SW = TW + T - 1;
    static_assert(SH * SW >= kMetricsThreads, "the staging buffer doubles as the reduction buffer");
    __shared__ double sp[SH * SW], st[SH * SW];  // T = 17: 2 x 12 KiB
    __shared__ double hp[5][SH][TW];              // T = 17: 40 KiB -> 64 KiB in all, two workgroups per CU
    const int tid = threadIdx.x;
    const long long wg = blockIdx.x;
    const PlaneTile pt = plane_tile(wg, tiles, tiles_x, C);
    const long long b = pt.b, c = pt.c;
    const int y0 = pt.ty * TH, x0 = pt.tx * TW;
    const int hv = H - T + 1, wv = W - T + 1;

    const long long pb = b * p.s[0] + c * p.s[1], tb = b * t.s[0] + c * t.s[1];
    for (int i = tid; i < SH * SW; i += kMetricsThreads) {
        const int yy = i / SW, xx = i - yy * SW;
        const long long gy = y0 + yy, gx = x0 + xx;
        double pv = 0.0, tv = 0.0;
        if (gy < H && gx < W) {
            pv = ld_f64<E>(p.data, pb + gy * p.s[2] + gx * p.s[3]);
            tv = ld_f64<E>(t.data, tb + gy * t.s[2] + gx * t.s[3]);
        }
        sp[i] = pv;
        st[i] = tv;
    }
    __syncthreads();

    // horizontal pass: R adjacent outputs of one staged row per work item
    for (int item = tid; item < SH * (TW / R); item += kMetricsThreads) {
        const int row = item / (TW / R), x = (item - row * (TW / R)) * R;
        double acc[R][5];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[r][q] = 0.0;
#pragma unroll
        for (int j = 0; j < T + R - 1; ++j) {
            const double pv = sp[row * SW + x + j], tv = st[row * SW + x + j];
            const double v[5] = {pv, tv, pv * pv, tv * tv, pv * tv};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int k = j - r;
                if (k >= 0 && k < T) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) acc[r][q] = fma(taps.w[k], v[q], acc[r][q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int r = 0; r < R; ++r) hp[q][row][x + r] = acc[r][q];
    }
    __syncthreads();

    // vertical pass + epilogue
    double c1 = 0.0, c2 = 0.0;
    if constexpr (EPI == EPI_SSIM) {
        const double range = param > 0.0 ? param : *range_dev;
        c1 = (0.01 * range) * (0.01 * range);
        c2 = (0.03 * range) * (0.03 * range);
    }
    double sum0 = 0.0, sum1 = 0.0;
    for (int o = tid; o < TH * TW; o += kMetricsThreads) {
        const int y = o / TW, x = o - y * TW;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < T; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = fma(taps.w[k], hp[q][y + k][x], m[q]);
        if (y0 + y < hv && x0 + x < wv) {
            if constexpr (EPI == EPI_SSIM) {
                sum0 += ssim_pixel(m, c1, c2);
            } else {
                double num, den;
                vif_pixel(m, param, num, den);
                sum0 += num;
                sum1 += den;
            }
        }
    }
    sum0 = block_reduce<OpSum>(sum0, sp);
    if constexpr (EPI == EPI_SSIM) {
        if (tid == 0) part[wg] = sum0;
    } else {
        sum1 = block_reduce<OpSum>(sum1, sp);
        if (tid == 0) part[wg * 2] = sum0;
        if (tid == 1) part[wg * 2 + 1] = sum1;  // two lanes, two 8-byte stores
    }
}

// ---- VIF: the next scale --------------------------------------------------------------------------------------------------------------
// out[plane][y][x] = sum_ij w[i] w[j] src[plane][2 y + i][2 x + j] for both images; grid: ceil(Ho * Wo / 256) * C * B workgroups
template <int E, int T, int C = 3>
__global__ __launch_bounds__(kMetricsThreads) void down_kernel(const StridedView p, const StridedView t, int Ho, int Wo, long long blocks,
                                                                 const MetricsTaps taps, double* outp, double* outt) {
    const long long wg = blockIdx.x;
    const long long plane = wg / blocks;
    const long long i = (wg - plane * blocks) * kMetricsThreads + threadIdx.x;
    const long long hw = (long long)Ho * Wo;
    if (i >= hw) return;
    const long long b = plane / C, c = plane - b * C;
    const long long y = i / Wo, x = i - y * Wo;
    const long long pb = b * p.s[0] + c * p.s[1] + 2 * y * p.s[2] + 2 * x * p.s[3];
    const long long tb = b * t.s[0] + c * t.s[1] + 2 * y * t.s[2] + 2 * x * t.s[3];
    double ap = 0.0, at = 0.0;
#pragma unroll
    for (int r = 0; r < T; ++r) {
        double hp_ = 0.0, ht_ = 0.0;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            hp_ = fma(taps.w[k], ld_f64<E>(p.data, pb + r * p.s[2] + k * p.s[3]), hp_);
            ht_ = fma(taps.w[k], ld_f64<E>(t.data, tb + r * t.s[2] + k * t.s[3]), ht_);
        }
        ap = fma(taps.w[r], hp_, ap);
        at = fma(taps.w[r], ht_, at);
    }
    outp[plane * hw + i] = ap;
    outt[plane * hw + i] = at;
}

// ---- the last kernel: tile partials -> out ----------------------------------------------------------------------------------------------
// n doubles at q[0], q[stride], .. in a fixed order: thread i takes i, i + 256, .., then the tree
__device__ __forceinline__ double ordered_sum(const double* q, long long n, int stride, double* sh) {
    double v = 0.0;
    for (long long i = threadIdx.x; i < n; i += kMetricsThreads) v += q[i * stride];
    return block_reduce<OpSum>(v, sh);
}
struct MetricsFinishArgs {
    int which;
    const double* ssim_part;
    long long ssim_tiles;
    double ssim_count;
    double fixed_range;
    const double* range_dev;
    const double* vif_part[4];
    long long vif_tiles[4];
};
// grid B
template <int C = 3> __global__ __launch_bounds__(kMetricsThreads) void finish_kernel(const MetricsFinishArgs a, double* out) {
    __shared__ double sh[kMetricsThreads];
    const long long b = blockIdx.x;
    double* o = out + b * kMetricSlots;
    if (a.which & MET_SSIM) {
        const double v = ordered_sum(a.ssim_part + b * C * a.ssim_tiles, C * a.ssim_tiles, 1, sh);
        if (threadIdx.x == 0) {
            o[MS_SSIM_SUM] = v;
            o[MS_SSIM_COUNT] = a.ssim_count;
            o[MS_SSIM_RANGE] = a.fixed_range > 0.0 ? a.fixed_range : *a.range_dev;
        }
    }
    if (a.which & MET_VIF) {
        for (int c = 0; c < C; ++c) {
            double num = 0.0, den = 0.0;
            for (int s = 0; s < 4; ++s) {  // scale by scale, as vif_per_image accumulates
                const double* q = a.vif_part[s] + (b * C + c) * a.vif_tiles[s] * 2;
                num += ordered_sum(q, a.vif_tiles[s], 2, sh);
                den += ordered_sum(q + 1, a.vif_tiles[s], 2, sh);
            }
            if (threadIdx.x == 0) {
                o[MS_VIF_NUM + c] = num;
                o[MS_VIF_DEN + c] = den;
            }
        }
    }
}

// ---- the launchers of one call with C channels (mz_metrics.hip: C = 3; mz_color.hip: C = 1 on the Y planes) ----------------------------
// g / g.sum() of evaluate.py's _gaussian_window, in double (the 2-D VIF window normalised in 2-D is its outer product)
static inline MetricsTaps gaussian_taps(int n, double sigma) {
    MetricsTaps t = {};
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) / 2.0;
        t.w[i] = exp(-(x * x) / (2.0 * sigma * sigma));
        sum += t.w[i];
    }
    for (int i = 0; i < n; ++i) t.w[i] /= sum;
    return t;
}

template <int E, int T, int EPI, int C>
static hipError_t launch_moments(const StridedView& p, const StridedView& t, int B, int H, int W, long long tiles, const MetricsTaps& taps,
                                 double param, const double* range_dev, double* part, hipStream_t s) {
    TileGrid g;  // of the (H - T + 1) x (W - T + 1) map; `tiles` is the plan's count (the workspace is laid out by it)
    if (!plane_tile_grid(H - T + 1, W - T + 1, kMetricsTileH, kMetricsTileW, B, &g, C)) return hipErrorInvalidValue;
    assert(g.tiles == tiles);
    hipLaunchKernelGGL((moments_kernel<E, T, EPI, C>), dim3((unsigned)g.wgs), dim3(kMetricsThreads), 0, s, p, t, H, W, tiles, g.tiles_x, taps, param,
                       range_dev, part);
    return hipGetLastError();
}

template <int E, int T, int C>
static hipError_t launch_down(const StridedView& p, const StridedView& t, int B, int Ho, int Wo, double* outp, double* outt, hipStream_t s) {
    const long long blocks = ((long long)Ho * Wo + kMetricsThreads - 1) / kMetricsThreads;
    if (!grid_ok(blocks, (long long)C * B)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((down_kernel<E, T, C>), dim3((unsigned)(blocks * C * B)), dim3(kMetricsThreads), 0, s, p, t, Ho, Wo, blocks,
                       gaussian_taps(T, T / 5.0), outp, outt);
    return hipGetLastError();
}

template <int E, int C> static hipError_t launch_metrics_e(const MetricsArgs& a, hipStream_t s) {
    const MetricsPlan& pl = a.plan;
    hipError_t e = hipSuccess;
    double* range_dev = (double*)(a.ws + pl.off_range);
    const bool batch_range = (a.which & MET_SSIM) && !(a.data_range > 0.0);
    if ((a.which & MET_PSNR) || batch_range) {
        double* part = (double*)(a.ws + pl.off_psnr);
        if (a.B > 65535) return hipErrorInvalidValue;
        hipLaunchKernelGGL((psnr_kernel<E, C>), dim3(pl.psnr_blocks, a.B), dim3(kMetricsThreads), 0, s, a.pred, a.target, a.H, a.W, part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = launch_psnr_reduce(part, pl.psnr_blocks, (double)C * (double)a.H * (double)a.W, a.out, a.B, s)) != hipSuccess) return e;
        if (batch_range && (e = launch_range(a.out, a.B, range_dev, s)) != hipSuccess) return e;
    }
    if (a.which & MET_SSIM) {
        e = launch_moments<E, 11, EPI_SSIM, C>(a.pred, a.target, a.B, a.H, a.W, pl.ssim_tiles, gaussian_taps(11, 1.5), a.data_range, range_dev,
                                            (double*)(a.ws + pl.off_ssim), s);
        if (e != hipSuccess) return e;
    }
    if (a.which & MET_VIF) {
        e = launch_moments<E, 17, EPI_VIF, C>(a.pred, a.target, a.B, a.H, a.W, pl.vif_tiles[0], gaussian_taps(17, 17 / 5.0), a.sigma_n_sq,
                                           nullptr, (double*)(a.ws + pl.off_vif[0]), s);
        if (e != hipSuccess) return e;
        double* pyr[4][2] = {};
        for (int k = 1; k < 4; ++k) {
            pyr[k][0] = (double*)(a.ws + pl.off_pyr[k]);
            pyr[k][1] = pyr[k][0] + (size_t)a.B * C * pl.vif_h[k] * pl.vif_w[k];
        }
        const StridedView p1 = dense_view(pyr[1][0], pl.vif_h[1], pl.vif_w[1], C), t1 = dense_view(pyr[1][1], pl.vif_h[1], pl.vif_w[1], C);
        const StridedView p2 = dense_view(pyr[2][0], pl.vif_h[2], pl.vif_w[2], C), t2 = dense_view(pyr[2][1], pl.vif_h[2], pl.vif_w[2], C);
        const StridedView p3 = dense_view(pyr[3][0], pl.vif_h[3], pl.vif_w[3], C), t3 = dense_view(pyr[3][1], pl.vif_h[3], pl.vif_w[3], C);
        if ((e = launch_down<E, 9, C>(a.pred, a.target, a.B, pl.vif_h[1], pl.vif_w[1], pyr[1][0], pyr[1][1], s)) != hipSuccess) return e;
        if ((e = launch_moments<EL_F64, 9, EPI_VIF, C>(p1, t1, a.B, pl.vif_h[1], pl.vif_w[1], pl.vif_tiles[1], gaussian_taps(9, 9 / 5.0), a.sigma_n_sq,
                                                    nullptr, (double*)(a.ws + pl.off_vif[1]), s)) != hipSuccess) return e;
        if ((e = launch_down<EL_F64, 5, C>(p1, t1, a.B, pl.vif_h[2], pl.vif_w[2], pyr[2][0], pyr[2][1], s)) != hipSuccess) return e;
        if ((e = launch_moments<EL_F64, 5, EPI_VIF, C>(p2, t2, a.B, pl.vif_h[2], pl.vif_w[2], pl.vif_tiles[2], gaussian_taps(5, 5 / 5.0), a.sigma_n_sq,
                                                    nullptr, (double*)(a.ws + pl.off_vif[2]), s)) != hipSuccess) return e;
        if ((e = launch_down<EL_F64, 3, C>(p2, t2, a.B, pl.vif_h[3], pl.vif_w[3], pyr[3][0], pyr[3][1], s)) != hipSuccess) return e;
        if ((e = launch_moments<EL_F64, 3, EPI_VIF, C>(p3, t3, a.B, pl.vif_h[3], pl.vif_w[3], pl.vif_tiles[3], gaussian_taps(3, 3 / 5.0), a.sigma_n_sq,
                                                    nullptr, (double*)(a.ws + pl.off_vif[3]), s)) != hipSuccess) return e;
    }
    if (a.which & (MET_SSIM | MET_VIF)) {
        MetricsFinishArgs f = {};
        f.which = a.which;
        f.ssim_part = (const double*)(a.ws + pl.off_ssim);
        f.ssim_tiles = pl.ssim_tiles;
        f.ssim_count = (double)C * (double)(a.H - 10) * (double)(a.W - 10);
        f.fixed_range = a.data_range;
        f.range_dev = range_dev;
        for (int k = 0; k < 4; ++k) {
            f.vif_part[k] = (const double*)(a.ws + pl.off_vif[k]);
            f.vif_tiles[k] = pl.vif_tiles[k];
        }
        hipLaunchKernelGGL((finish_kernel<C>), dim3(a.B), dim3(kMetricsThreads), 0, s, f, a.out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- luma: the Y planes of both images --------------------------------------------------------------------------------------------------
// yp[b][y][x], yt[b][y][x] = the unrounded float64 Y (mz_color.h) of p and t; grid: ceil(H * W / 256) * B workgroups, one pixel a thread
template <int E>
__global__ __launch_bounds__(kMetricsThreads) void luma_planes_kernel(const StridedView p, const StridedView t, int H, int W, long long blocks,
                                                                        const LumaCoeffs k, double* yp, double* yt) {
    const long long wg = blockIdx.x;
    const long long b = wg / blocks;
    const long long i = (wg - b * blocks) * kMetricsThreads + threadIdx.x;
    const long long hw = (long long)H * W;
    if (i >= hw) return;
    const long long y = i / W, x = i - y * W;
    yp[b * hw + i] = luma_at<E>(p, b * p.s[0] + y * p.s[2] + x * p.s[3], k);
    yt[b * hw + i] = luma_at<E>(t, b * t.s[0] + y * t.s[2] + x * t.s[3], k);
}

#endif  // MZ_METRICS_KERNELS

}  // namespace mz
