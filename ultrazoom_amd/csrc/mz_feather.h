// Feathered tiling (mz_feather_paste(): include/mewzoom_hip.h; ultrazoom_amd/tiling.py: upscale_feathered): one rectangle pasted onto
// another of the same shape with a linear cross-fade along its top and left edges.  The tiles of a small-halo tiling overlap by a band
// around every interior cut; the later tile is pasted onto the earlier one with a ramp as long as the band.  No reference counterpart
// (the reference has no tiling code).
//
// THE ARITHMETIC, stated here once (the kernel of mz_feather.hip and the host compile this source; tests/feather_ref.py restates it in
// numpy).  Float64 with contraction off.
//   ramp     a ramp of n positions, 0 <= n <= 2^20 (kFeatherMaxRamp).  rho(n) = 1.0 / (2 n), a float64 quotient formed ON THE HOST and
//            handed to the kernel;  omega(n, k) = (2 k + 1) * rho(n) for 0 <= k < n, one float64 multiplication;  omega = 1 for k >= n
//            and for n == 0.  The weights are the midpoints of n equal steps from 0 to 1: 1 / (2 n) at k = 0, 1 - 1 / (2 n) at k = n - 1.
//            For every n of the range omega(n, n - 1) < 1 strictly (the largest is 1 - 2^-21) and omega grows with k
//            (tests/feather_main.cpp walks all of them)
//   weight   element (y, x) of a paste with the ramps (ny, nx):  w = omega(ny, y) * omega(nx, x), a float64 product.  w == 1 exactly
//            outside both ramps and nowhere else
//   paste    s the element of src, d the element of dst.  If w == 1, or s and d hold the same bit pattern: dst receives the BIT PATTERN
//            of s -- a select, not arithmetic: a NaN, a -0 or uninitialised bytes in dst under w == 1 change nothing, and two tiles
//            that agree give exactly their common value.  Otherwise
//              f32 / bf16 / f16   v = d + w * (s - d), in exactly that order; v rounded ONCE to the element type (st_f64 of mz_view.h:
//                                 float32 by the cast, a 16-bit type through round-to-odd).  No clamp: a convex combination
//              uint8              s and d are the codes 0..255 as float64 (no division by 255), the same expression; the stored code is
//                                 (int)(v + 0.5)
//
// The host part needs no HIP header: plain g++ compiles it.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>  // (mz_view.h's device part needs it first)
#endif
#include <stdint.h>

#include "mz_color.h"
#include "mz_view.h"

namespace mz {

constexpr int kFeatherThreads = 256;
static_assert(kFeatherThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kFeatherMaxRamp = 1 << 20;
// one workgroup: kFeatherRows rows of kFeatherRuns runs of 16 bytes; a lane takes one run of kFeatherRows / (threads / runs) rows
constexpr int kFeatherRuns = 32, kFeatherRows = 32;
static_assert(kFeatherRows % (kFeatherThreads / kFeatherRuns) == 0, "whole steps of rows");

inline bool feather_ramp_ok(int n) { return n >= 0 && n <= kFeatherMaxRamp; }
// rho(n) on the host; 0 for n == 0, where no weight is formed from it
inline double feather_rho(int n) { return n > 0 ? 1.0 / (2.0 * (double)n) : 0.0; }
// omega(n, k), rho = feather_rho(n); k >= 0
MZ_HD inline double feather_omega(int n, double rho, int k) {
#pragma clang fp contract(off)
    return k < n ? (double)(2 * k + 1) * rho : 1.0;
}
// w of an element: the product of its two axis weights
MZ_HD inline double feather_weight(double wy, double wx) {
#pragma clang fp contract(off)
    return wy * wx;
}
// v of a pair of values that the select has not taken
MZ_HD inline double feather_mix(double s, double d, double w) {
#pragma clang fp contract(off)
    const double t = s - d;
    const double p = w * t;
    return d + p;
}
// the uint8 code of v
MZ_HD inline int feather_code(double v) {
#pragma clang fp contract(off)
    return (int)(v + 0.5);
}

struct FeatherArgs {
    StridedView src, dst;  // [B,3,H,W] both
    int elem;              // Elem 0..3 of both
    int B, H, W;
    int ramp_y, ramp_x;
};
// hipError_t values (kept as int: this header stays free of HIP types); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h)
// can launch -- found before the launch: a refused call writes nothing
int launch_feather_paste(const FeatherArgs& a, void* hip_stream);

}  // namespace mz
