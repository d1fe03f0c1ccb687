// Luma (Y) of an RGB image view: the number every super-resolution paper reports its PSNR / SSIM on (mz_luma(), mz_metrics_luma():
// include/mewzoom_hip.h).  No reference counterpart in model.py or validate.py: the reference measures RGB over the full frame.
//
// THE ARITHMETIC, stated here once (the kernel of mz_color.hip, the plane kernel of mz_metrics.h and the host's mz_debug_luma_coeffs
// compile this source; tests/color_ref.py restates it in Python).  Two standards, for R, G, B in units of [0, 1]:
//     0  "bt601"  studio range, MATLAB's rgb2ycbcr and basicsr's bgr2ycbcr(y_only=True):
//                 Y = 16/255 + (65.481/255) R + (128.553/255) G + (24.966/255) B         white: 235/255, black: 16/255
//     1  "full"   full range, BT.601 / JFIF / Pillow's "L":  Y = 0.299 R + 0.587 G + 0.114 B
// The four constants are the float64 results of the divisions as written (65.481 / 255.0, ..); those of "full" are the literals.  The
// sum is float64, three fused multiply-adds in this order:
//     acc = off;  acc = fma(kr, r, acc);  acc = fma(kg, g, acc);  acc = fma(kb, b, acc)
// on elements read with ld_f64<E> (mz_view.h): a uint8 value v is v / 255.0 by true division, the float types are exact in float64.
// The sum is rounded ONCE on store (luma_round_raw below); mz_metrics_luma keeps it unrounded.
//
// The host part needs no HIP header: plain g++ compiles it.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>  // (mz_view.h's device part needs it first)
#endif
#include <math.h>
#include <stdint.h>

#include "mz_view.h"

#ifdef __HIPCC__
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif

namespace mz {

enum LumaStandard : int { LUMA_BT601 = 0, LUMA_FULL = 1 };
MZ_HD inline bool luma_valid(int standard) { return standard == LUMA_BT601 || standard == LUMA_FULL; }

struct LumaCoeffs { double off, kr, kg, kb; };
MZ_HD inline LumaCoeffs luma_coeffs(int standard) {
    if (standard == LUMA_FULL) return LumaCoeffs{0.0, 0.299, 0.587, 0.114};
    return LumaCoeffs{16.0 / 255.0, 65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0};
}
MZ_HD inline double luma_of(const LumaCoeffs& k, double r, double g, double b) {
    double acc = k.off;
    acc = fma(k.kr, r, acc);
    acc = fma(k.kg, g, acc);
    acc = fma(k.kb, b, acc);
    return acc;
}

struct LumaArgs {
    StridedView x, out;  // [B,3,H,W] and [B,1,H,W] (out.s[1] is never used)
    int elem;            // Elem 0..3 of both
    int B, H, W;
    int standard;        // LumaStandard
    int clamp;
};
// hipError_t values (kept as int: this header stays free of HIP types); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch
int launch_luma(const LumaArgs& a, void* hip_stream);

#ifdef __HIPCC__
// the value ld_f64<E> gives for an element whose bits are `raw` (an element of a 16-byte vector: vec_get)
template <int E> __device__ __forceinline__ double f64_of_raw(uint32_t raw) {
    if constexpr (E == EL_F32) return (double)__builtin_bit_cast(float, raw);
    else if constexpr (E == EL_BF16) return (double)__builtin_bit_cast(float, raw << 16);
    else if constexpr (E == EL_F16) return (double)(float)__builtin_bit_cast(_Float16, (uint16_t)raw);
    else return (double)raw / 255.0;
}
// The one rounding of Y to the stored element, as its raw bits.  Float types: with `clamp` the value is clamped to [0, 1] first (a NaN
// becomes 0), then the casts of st_f64 (mz_view.h): float32 by the cast, a 16-bit type through f32_round_odd.  uint8 always clamps, then
// * 255 + 0.5, then truncates, in float64, the product and the sum rounded separately (contraction off) -- the project's uint8 rule,
// the statement of interp_round_raw (mz_interp.hip).
template <int E> __device__ __forceinline__ uint32_t luma_round_raw(double v, int clamp) {
#pragma clang fp contract(off)
    if constexpr (E == EL_U8) {
        v = fmin(fmax(v, 0.0), 1.0);
        return (uint32_t)(uint8_t)(v * 255.0 + 0.5);
    } else {
        if (clamp) v = fmin(fmax(v, 0.0), 1.0);
        if constexpr (E == EL_F32) return __builtin_bit_cast(uint32_t, (float)v);
        else if constexpr (E == EL_BF16) return __builtin_bit_cast(uint16_t, (__bf16)f32_round_odd(v));
        else return __builtin_bit_cast(uint16_t, (_Float16)f32_round_odd(v));
    }
}
// Y of the pixel whose red element is element i of the view's data: the three reads and the sum
template <int E> __device__ __forceinline__ double luma_at(const StridedView& v, long long i, const LumaCoeffs& k) {
    return luma_of(k, ld_f64<E>(v.data, i), ld_f64<E>(v.data, i + v.s[1]), ld_f64<E>(v.data, i + 2 * v.s[1]));
}
#endif  // __HIPCC__

}  // namespace mz
