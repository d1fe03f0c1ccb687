// Plain (not antialiased) interpolation of an image view to any size (mz_interpolate(), include/mewzoom_hip.h): the arithmetic of torch's
// interpolate(x, size=(Hout, Wout), mode="nearest" | "bilinear" | "bicubic", align_corners=False) as gfx950 kernels.  Reference
// counterpart: the model's own skip, Upsample(scale_factor=r, mode="bicubic") (model.py:71, 156), and the bicubic baseline its
// validate.py:84-118 measures every result against.  NOT mz_resize.h: that one is antialiased and uses A = -0.5.
//
// THE TAPS of output index i of one axis, n_in samples -> n_out, stated here once (interp_taps() below: the kernels of mz_interp.hip and
// the host's mz_debug_interp_taps() compile this source).  s = n_in / n_out in double, from the two sizes:
//   nearest   idx = i when n_in == n_out, else min((int)floorf((float)i * sf), n_in - 1) with sf = (float)n_in / (float)n_out: float32
//             arithmetic, as torch's legacy "nearest" does it.  One tap of weight 1: elements are moved, never changed.
//   bilinear  src = max(s (i + 0.5) - 0.5, 0);  i0 = (int)src;  i1 = i0 + (i0 < n_in - 1);  w = {1 - (src - i0), src - i0}
//   bicubic   src = s (i + 0.5) - 0.5 (not clamped);  f = floor(src);  t = src - f;  idx_k = clamp(f - 1 + k, 0, n_in - 1);
//             w = {c2(t + 1), c1(t), c1(1 - t), c2(2 - t)},  c1(u) = ((A + 2) u - (A + 3)) u u + 1,  c2(u) = ((A u - 5 A) u + 8 A) u - 4 A,
//             A = -0.75
// With n_out == n_in the weights are exactly {1, 0} / {0, 1, 0, 0}: finite values pass through.
//
// THE EVALUATION of bilinear and bicubic, stated here once (interp_dot() below): every source row an output needs is filtered horizontally,
// h[row] = sum_k wx_k x[row][idx_x_k], then the rows are combined, v = sum_k wy_k h[idx_y_k]; both sums run in FLOAT64 as
// acc = fma(w_k, v_k, acc) from acc = 0 in ascending k, the intermediate h stays float64, and v is rounded ONCE to the stored type
// (the 16-bit types through a round-to-odd float32, which makes the second rounding the only one).  uint8 follows mz_view.h: read as
// v / 255, stored as clamp -> * 255 + 0.5 -> truncate, in float64.  clamp != 0 clamps the float types to [0, 1] before the rounding.
//
// The kernel (mz_interp.hip): one workgroup of kInterpThreads threads = one kInterpTileH x kInterpTileW tile of the WINDOW of one plane.
// It computes the tile's column and row taps once, into LDS.  ENLARGING (n_in <= n_out on both axes) with at most kInterpStageRows
// source rows under the tile -- tile / r + 3 of them at a ratio r -- it runs the SEPARABLE path: the horizontal sums of those rows for the
// tile's columns go to LDS ([rows][tile width + padding] float64), the vertical sums run out of LDS.  Otherwise (shrinking, or a ratio near 1) each
// output GATHERS its 1, 2 or 4 x 4 source elements from global memory.  Both paths call interp_dot() on the same operands in the same
// order: the same bits.  Each lane produces 16 bytes of consecutive output elements of one row and stores them at once where the output
// view is dense and 16-byte aligned (the launcher decides), element by element otherwise.  The source is read one element at a time on
// both paths: it is 1 / r^2 of the traffic, and neighbouring lanes read neighbouring or equal addresses.  All addressing is 64-bit and
// signed.  No atomics, no workspace.  A call reads only source elements its window's outputs name: when enlarging, the rows under a tile
// are contiguous (consecutive outputs' first taps differ by at most one), which is why only enlarging calls take the separable path.
//
// LDS of the bicubic instantiations: taps 4 (8 + 4) (128 + 32) = 7680 bytes, rows 20 * (128 + V) * 8 with V = 4 / 8 / 16 elements of a
// 16-byte chunk (one double of padding behind each element's chunks: mz_interp.hip says why): at most 30720 bytes, five workgroups a CU.
//
// The tap and dot statements need no HIP header: plain g++ compiles them.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mz_view.h"

#ifndef MZ_HD
#ifdef __HIPCC__
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {

constexpr int kInterpTileH = 32;  // output pixels of one interp_kernel workgroup
constexpr int kInterpTileW = 128;
constexpr int kInterpThreads = 256;
static_assert(kInterpThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kInterpStageRows = 20;  // source rows whose horizontal sums a workgroup keeps in LDS: 32 / 2 + 3, and one to spare

enum InterpMode : int { IM_NEAREST = 0, IM_BILINEAR = 1, IM_BICUBIC = 2 };

MZ_HD constexpr int interp_count(int mode) { return mode == IM_BICUBIC ? 4 : mode == IM_BILINEAR ? 2 : 1; }

// The taps of output index i (0 <= i < n_out) of one axis: returns count, idx[0..count) inside [0, n_in), w[0..count)
MZ_HD inline int interp_taps(int n_in, int n_out, int mode, int i, int idx[4], double w[4]) {
#pragma clang fp contract(off)  // the host and the device evaluate the same roundings
    if (mode == IM_NEAREST) {
        int j = i;
        if (n_in != n_out) {
            const float sf = (float)n_in / (float)n_out;
            j = (int)floorf((float)i * sf);
            if (j > n_in - 1) j = n_in - 1;
        }
        idx[0] = j;
        w[0] = 1.0;
        return 1;
    }
    const double s = (double)n_in / (double)n_out;
    if (mode == IM_BILINEAR) {
        double src = s * ((double)i + 0.5) - 0.5;
        if (src < 0.0) src = 0.0;
        int i0 = (int)src;
        if (i0 > n_in - 1) i0 = n_in - 1;
        const double l = src - (double)i0;
        idx[0] = i0;
        idx[1] = i0 + (i0 < n_in - 1 ? 1 : 0);
        w[0] = 1.0 - l;
        w[1] = l;
        return 2;
    }
    const double A = -0.75;
    const double src = s * ((double)i + 0.5) - 0.5;
    const double f = floor(src);
    const double t = src - f;
    const long long base = (long long)f - 1;
    for (int k = 0; k < 4; ++k) {
        long long j = base + k;
        if (j < 0) j = 0;
        if (j > n_in - 1) j = n_in - 1;
        idx[k] = (int)j;
    }
    const double u0 = t + 1.0, u2 = 1.0 - t, u3 = 2.0 - t;
    w[0] = ((A * u0 - 5.0 * A) * u0 + 8.0 * A) * u0 - 4.0 * A;
    w[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
    w[2] = ((A + 2.0) * u2 - (A + 3.0)) * u2 * u2 + 1.0;
    w[3] = ((A * u3 - 5.0 * A) * u3 + 8.0 * A) * u3 - 4.0 * A;
    return 4;
}

// sum_k w_k v_k, the one order of both passes
template <int K> MZ_HD inline double interp_dot(const double* w, const double* v) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) acc = fma(w[k], v[k], acc);
    return acc;
}

struct InterpArgs {
    StridedView x, out;  // out: the window's view
    int elem;            // Elem 0..3
    int B, Hin, Win, Hout, Wout;
    int mode, clamp;
    int y0, x0, h, w;    // the window of the Hout x Wout result that is computed and stored
};
// hipError_t values (kept as int: this header stays free of HIP types); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch.
// MZ_INTERP_GATHER in the environment (read at every call; a debug knob of the tests) sends every tile down the gather path.
int launch_interp(const InterpArgs& a, void* hip_stream);

}  // namespace mz
