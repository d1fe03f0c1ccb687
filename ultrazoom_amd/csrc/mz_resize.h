// Antialiased resampling of an image view to any size (mz_resize(), include/mewzoom_hip.h): the arithmetic of
// torch's interpolate(..., mode="bicubic" | "bilinear", antialias=True, align_corners=False) as gfx950 kernels.  No reference
// counterpart in model.py: stands in for torchvision's antialiased Resize as the reference's data.py:91-108 uses it.
//
// Per axis, n_in samples -> n_out (resize_taps() below is the one statement of it, for the device's table kernel and the host's
// mz_debug_resize_taps() alike):
//   scale = n_in / n_out (double, from the two sizes);   support = interp / 2 * max(scale, 1);   inv = 1 / max(scale, 1)
//   center = scale (i + 0.5);   first = max((int)(center - support + 0.5), 0);   count = min((int)(center + support + 0.5), n_in) - first
//   w_j = f((j + first - center + 0.5) inv) / sum_j f(..)   in double;   out[i] = sum_j w_j in[first + j]
//   f: bicubic with A = -0.5 (interp 4; the PIL constant of torch's antialiased kernels, NOT the -0.75 of the head's fused skip) or the
//   triangle (interp 2).
// The filter is separable: horizontal pass, then vertical pass.  Both passes accumulate in FLOAT64 with fma in ascending j, from the double
// weights as they are (the inputs are exact in it); the intermediate between the passes is float32 and is never rounded to the storage
// type.  THE LAST STEP: the second sum is rounded to float32, (float)acc, and that float32 goes through st_f32 (mz_view.h): the clamp, then
// nothing more for float32, the cast to a 16-bit type -- a SECOND rounding: float64 -> float32 -> 16 bits, not the one rounding of
// mz_interp.h -- or u8_of_unit.  A uint8 input is read as the float32 quotient v / 255.0f.  tests/test_image_exact_gpu.py holds the
// kernel to this statement bit for bit.  Float32 accumulation (about 1e-7 absolute on [0, 1] images) would meet the float32 bound but not "one ulp of the storage type"
// where a bicubic result of a 16-bit type comes close to zero, the ulp shrinking with the value (EXPERIMENTS.md, resize entry).
//
//   resize_table_kernel  one thread per output column / row: {first, count} and the weights of both axes, into the caller's workspace (no
//                        host table, no copy, no synchronisation)
//   resize_kernel        <element type>: one workgroup of 256 threads = one kResizeTileH x kResizeTileW output tile of one channel plane of
//                        one image.  Every input row of the tile's vertical range [first(y0), first(y1) + count(y1)) is filtered straight
//                        from global memory into LDS ([rows][tile width] float32; neighbouring lanes' overlapping taps are served by the
//                        caches), the vertical pass runs out of LDS, the store follows.  The tiles are laid from the WINDOW's corner and
//                        columns / rows beyond the window have no taps, so a call reads exactly what its window's outputs need; an output's
//                        own arithmetic does not depend on the tile it falls in.
// One kernel serves every layout (one-element loads and stores), so dense and strided views give the same bits.  All address arithmetic is
// 64-bit and signed (element strides of a view may be negative and larger than 2^31).  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mz_view.h"

namespace mz {

constexpr int kResizeTileH = 8;    // output pixels of one resize_kernel workgroup
constexpr int kResizeTileW = 32;
constexpr int kResizeThreads = 256;
static_assert(kResizeThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kResizeMaxRatio = 16;  // n_in / n_out beyond this is refused: bounds count at 66 and the LDS of a workgroup at 43 KiB
constexpr int kResizeMaxTaps = 66;

enum ResizeFilter : int { RF_BICUBIC = 0, RF_BILINEAR = 1 };

// f(u) of the table above
__host__ __device__ inline double resize_filter(int filter, double u) {
#pragma clang fp contract(off)  // the host and the device evaluate the same roundings
    if (u < 0.0) u = -u;
    if (filter == RF_BILINEAR) return u < 1.0 ? 1.0 - u : 0.0;
    const double A = -0.5;
    if (u < 1.0) return ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0;
    if (u < 2.0) return (((u - 5.0) * u + 8.0) * u - 4.0) * A;
    return 0.0;
}

// The table of output index i of one axis: returns count, *first, and hands the normalised weights w_0 .. w_{count-1} (double) to put(j, w)
// in ascending j.  cap >= 0: nothing is put when count exceeds it (the count is still returned).
template <class Put> __host__ __device__ inline int resize_taps(int n_in, int n_out, int filter, int i, int* first, int cap, Put&& put) {
#pragma clang fp contract(off)
    const double scale = (double)n_in / (double)n_out;
    const double half = filter == RF_BILINEAR ? 1.0 : 2.0;  // interp / 2
    const double support = scale >= 1.0 ? half * scale : half;
    const double inv = scale >= 1.0 ? 1.0 / scale : 1.0;
    const double center = scale * ((double)i + 0.5);
    long long lo = (long long)(center - support + 0.5), hi = (long long)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_in) hi = n_in;
    const int count = (int)(hi - lo);
    *first = (int)lo;
    if (cap >= 0 && count > cap) return count;
    double sum = 0.0;
    for (int j = 0; j < count; ++j) sum += resize_filter(filter, ((double)(j + lo) - center + 0.5) * inv);
    for (int j = 0; j < count; ++j) put(j, resize_filter(filter, ((double)(j + lo) - center + 0.5) * inv) / sum);
    return count;
}

// upper bounds from the two sizes alone (host): taps of one output, input rows under kResizeTileH output rows
inline int resize_taps_cap(int n_in, int n_out, int filter) {
    const double scale = (double)n_in / (double)n_out, half = filter == RF_BILINEAR ? 1.0 : 2.0;
    const double support = scale >= 1.0 ? half * scale : half;
    const int cap = (int)(2.0 * support) + 2;  // (int)(c + s + 0.5) - (int)(c - s + 0.5) <= 2 s + 1
    return cap < kResizeMaxTaps ? cap : kResizeMaxTaps;
}
inline int resize_rows_cap(int n_in, int n_out, int filter) {
    const double scale = (double)n_in / (double)n_out;
    return (int)((kResizeTileH - 1) * scale) + 1 + resize_taps_cap(n_in, n_out, filter);
}

// Workspace layout of one call (bytes from the start, every part 256-byte aligned); depends on the four sizes and the filter only
struct ResizePlan {
    int taps_x, taps_y;  // weights kept per output column / row
    int rows_cap;        // input rows a workgroup may have to stage
    size_t off_span_x, off_w_x, off_span_y, off_w_y;  // int {first, count} [n_out];  double [n_out][taps]
    size_t total;
    size_t lds_bytes;    // dynamic LDS of resize_kernel
};
inline ResizePlan resize_plan(int Hin, int Win, int Hout, int Wout, int filter) {
    ResizePlan p = {};
    auto take = [&](size_t bytes) {
        const size_t at = p.total;
        p.total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    p.taps_x = resize_taps_cap(Win, Wout, filter);
    p.taps_y = resize_taps_cap(Hin, Hout, filter);
    p.rows_cap = resize_rows_cap(Hin, Hout, filter);
    p.off_span_x = take((size_t)Wout * 2 * sizeof(int));
    p.off_w_x = take((size_t)Wout * p.taps_x * sizeof(double));
    p.off_span_y = take((size_t)Hout * 2 * sizeof(int));
    p.off_w_y = take((size_t)Hout * p.taps_y * sizeof(double));
    p.lds_bytes = ((size_t)p.taps_x * kResizeTileW + (size_t)p.taps_y * kResizeTileH) * sizeof(double) + (size_t)p.rows_cap * kResizeTileW * sizeof(float);
    return p;
}

struct ResizeArgs {
    StridedView x, out;
    int elem;                  // Elem 0..3
    int B, Hin, Win, Hout, Wout;
    int filter, clamp;
    int y0, x0, h, w;          // the window of the Hout x Wout result that is computed and stored
    char* ws;
    ResizePlan plan;
};
// Enqueues the whole call (the table kernel, then resize_kernel); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch
hipError_t launch_resize(const ResizeArgs& a, hipStream_t s);

#ifdef MZ_RESIZE_KERNELS  // mz_resize.hip only: the host runtime includes the plan above without the device code

// grid: ceil((Wout + Hout) / 256): thread t < Wout is output column t, the next Hout threads are the output rows
__global__ __launch_bounds__(kResizeThreads) void resize_table_kernel(int Hin, int Win, int Hout, int Wout, int filter, int taps_x, int taps_y,
                                                                       int* span_x, double* w_x, int* span_y, double* w_y) {
    const long long t = (long long)blockIdx.x * kResizeThreads + threadIdx.x;
    if (t >= (long long)Wout + Hout) return;
    const bool col = t < Wout;
    const int i = (int)(col ? t : t - Wout);
    const int taps = col ? taps_x : taps_y;
    int* span = col ? span_x : span_y;
    double* w = (col ? w_x : w_y) + (long long)i * taps;
    int first = 0;
    const int count = resize_taps(col ? Win : Hin, col ? Wout : Hout, filter, i, &first, taps, [&](int j, double v) { w[j] = v; });
    span[2 * i] = first;
    span[2 * i + 1] = count <= taps ? count : 0;  // (count <= taps always: resize_taps_cap; an output without taps stores 0)
}

// grid: tiles * 3 * B workgroups, tile fastest (tiles of the window, row by row); dynamic LDS: ResizePlan::lds_bytes
template <int E>
__global__ __launch_bounds__(kResizeThreads) void resize_kernel(const StridedView x, const StridedView out, int y0, int x0, int h, int w,
                                                                  long long tiles, int tiles_x, int clamp, int taps_x, int taps_y, int rows_cap,
                                                                  const int* span_x, const double* w_x, const int* span_y, const double* w_y) {
    constexpr int TH = kResizeTileH, TW = kResizeTileW;
    static_assert(TH * TW == kResizeThreads, "one thread per output of the tile");
    extern __shared__ double lds[];
    double* wxs = lds;                           // [taps_x][TW]: the tile's column weights, tap-major (lane x -> bank pair x)
    double* wys = wxs + (size_t)taps_x * TW;     // [taps_y][TH]
    float* hrow = (float*)(wys + (size_t)taps_y * TH);  // [rows_cap][TW]: the horizontally filtered input rows of the tile
    const int tid = threadIdx.x, tx = tid & (TW - 1), ty = tid / TW;
    const PlaneTile pt = plane_tile(blockIdx.x, tiles, tiles_x);
    const long long b = pt.b, c = pt.c;
    const int tile_y = pt.ty, tile_x = pt.tx;
    const int wy_ = tile_y * TH + ty, wx_ = tile_x * TW + tx;  // inside the window
    const int oy = y0 + wy_, ox = x0 + wx_;                      // inside the Hout x Wout result

    // this thread's column and row: {first, count}, count = 0 beyond the window
    int fx = 0, cx = 0, fy = 0, cy = 0;
    if (wx_ < w) {
        fx = span_x[2 * (long long)ox];
        cx = span_x[2 * (long long)ox + 1];
    }
    if (wy_ < h) {
        fy = span_y[2 * (long long)oy];
        cy = span_y[2 * (long long)oy + 1];
    }
    for (int j = ty; j < cx; j += TH) wxs[j * TW + tx] = w_x[(long long)ox * taps_x + j];
    for (int j = tx; j < cy; j += TW) wys[j * TH + ty] = w_y[(long long)oy * taps_y + j];
    // the tile's input rows [row0, row0 + rows): first and count grow with the output index
    const int ya = y0 + tile_y * TH, yb = min(ya + TH, y0 + h) - 1;
    const int row0 = span_y[2 * (long long)ya];
    const int rows = min(span_y[2 * (long long)yb] + span_y[2 * (long long)yb + 1] - row0, rows_cap);
    __syncthreads();

    // horizontal pass: thread (ty, tx) filters column tx of rows ty, ty + TH, ..; four rows in flight per step
    const long long xb = b * x.s[0] + c * x.s[1] + (long long)fx * x.s[3];
    for (int r = ty; r < rows; r += 4 * TH) {
        long long at[4];
        double acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            at[k] = xb + (long long)(row0 + min(r + k * TH, rows - 1)) * x.s[2];  // rows past the end repeat the last one and are not kept
            acc[k] = 0.0;
        }
        for (int j = 0; j < cx; ++j) {
            const double wj = wxs[j * TW + tx];
            const long long o = (long long)j * x.s[3];
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = ld_f32<E>(x.data, at[k] + o);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fma(wj, (double)v[k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (r + k * TH < rows) hrow[(r + k * TH) * TW + tx] = (float)acc[k];
    }
    __syncthreads();

    // vertical pass out of LDS, then the store
    if (cx > 0 && cy > 0) {
        const float* col = hrow + (fy - row0) * TW + tx;
        double acc = 0.0;
        for (int j = 0; j < cy; ++j) acc = fma(wys[j * TH + ty], (double)col[j * TW], acc);
        st_f32<E>((void*)out.data, b * out.s[0] + c * out.s[1] + (long long)wy_ * out.s[2] + (long long)wx_ * out.s[3], (float)acc, clamp);
    }
}

#endif  // MZ_RESIZE_KERNELS

}  // namespace mz
