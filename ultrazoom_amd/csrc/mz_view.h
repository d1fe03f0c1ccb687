// An image view as the kernels of mz_metrics.h, mz_resize.h and mz_degrade.h take it, the element codes, and every conversion between a
// stored element and the value it stands for -- stated here once (the convolution kernels' view path, ImageViews / StemView, is
// separate; mz_view_check.h holds the host's checks of the public mz_image_view).  A uint8 element v stands for v / 255: read by a
// TRUE division, stored as clamp -> * 255 + 0.5 -> truncate, exactly mz_forward_u8's rule; the float accessors do that in float32,
// the double ones in float64.  The struct and the enum need no HIP header; the accessors exist under hipcc only, for translation
// units that have included <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

namespace mz {

struct StridedView {
    const void* data;  // element (image 0, channel 0, row 0, column 0); of a windowed output: the window's first element
    long long s[4];    // element strides: image, channel, row, column (signed)
};

// the `elem` of the view entries; EL_F64 is internal (the VIF pyramid in mz_metrics' workspace)
enum Elem : int { EL_F32 = 0, EL_BF16 = 1, EL_F16 = 2, EL_U8 = 3, EL_F64 = 4 };

#ifdef __HIPCC__
#include <type_traits>

// the uint8 contract in float32.  v * 255.0f + 0.5f is compiled to one v_fma_f32; a product rounded before the sum (the host's and the
// tests' restatements) gives the same byte for every float32 within 64 ulps of each threshold (k - 0.5) / 255 and for every value the
// exact image tests store: tests/test_image_exact_cpu.py::test_uint8_store_rule_fused_and_unfused_give_the_same_bytes
__device__ __forceinline__ float unit_of_u8(int v) { return (float)v / 255.0f; }
__device__ __forceinline__ uint8_t u8_of_unit(float v) { return (uint8_t)fminf(fmaxf(v * 255.0f + 0.5f, 0.0f), 255.0f); }

template <int E> __device__ __forceinline__ float ld_f32(const void* base, long long i) {
    static_assert(E >= EL_F32 && E <= EL_U8, "float64 data is read by ld_f64");
    if constexpr (E == EL_F32) return ((const float*)base)[i];
    else if constexpr (E == EL_BF16) return __builtin_bit_cast(float, (uint32_t)((const uint16_t*)base)[i] << 16);
    else if constexpr (E == EL_F16) return (float)((const _Float16*)base)[i];
    else return unit_of_u8(((const uint8_t*)base)[i]);
}
template <int E> __device__ __forceinline__ double ld_f64(const void* base, long long i) {
    if constexpr (E == EL_U8) return (double)((const uint8_t*)base)[i] / 255.0;
    else if constexpr (E == EL_F64) return ((const double*)base)[i];
    else return (double)ld_f32<E>(base, i);
}
// clamp: to [0, 1] first (a uint8 store clamps whatever it says)
template <int E> __device__ __forceinline__ void st_f32(void* base, long long i, float v, int clamp) {
    if constexpr (E == EL_U8) {
        ((uint8_t*)base)[i] = u8_of_unit(v);
    } else {
        if (clamp) v = fminf(fmaxf(v, 0.0f), 1.0f);
        if constexpr (E == EL_F32) ((float*)base)[i] = v;
        else if constexpr (E == EL_BF16) ((__bf16*)base)[i] = (__bf16)v;
        else ((_Float16*)base)[i] = (_Float16)v;
    }
}
// float64 -> float32 rounded to ODD (truncate, then set the last bit when inexact): a following round-to-nearest to a 16-bit type is then
// the one rounding of the float64 value
__device__ __forceinline__ float f32_round_odd(double d) {
    const float f = (float)d;
    if ((double)f == d || f != f) return f;
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if (fabs((double)f) > fabs(d)) u -= 1;  // towards zero (|f| > |d| >= 0: f is not a zero)
    return __builtin_bit_cast(float, u | 1u);
}
// A float64 sum to the stored element, no clamp: float32 is (float)v and uint8 is u8_of_unit((float)v); a 16-bit type is v rounded ONCE.
// Written out because the two casts (T16)(float)v do not pin it: behind a clamp that is an argument the compiler rounds twice, as
// written (resize_kernel), and without one it merges them into the one rounding (what blur_kernel, which calls this, always computed)
template <int E> __device__ __forceinline__ void st_f64(void* base, long long i, double v) {
    if constexpr (E == EL_BF16 || E == EL_F16) st_f32<E>(base, i, f32_round_odd(v), 0);
    else st_f32<E>(base, i, (float)v, 0);
}
// v in [0, 1] already
template <int E> __device__ __forceinline__ void st_f64_unit(void* base, long long i, double v) {
    if constexpr (E == EL_U8) ((uint8_t*)base)[i] = (uint8_t)(v * 255.0 + 0.5);
    else if constexpr (E == EL_F32) ((float*)base)[i] = (float)v;
    else if constexpr (E == EL_BF16) ((__bf16*)base)[i] = (__bf16)(float)v;
    else ((_Float16*)base)[i] = (_Float16)v;
}
// an element as the 8-bit sample 0..255 it stands for, and back (the JPEG kernels)
template <int E> __device__ __forceinline__ int ld_8bit(const void* base, long long i) {
    if constexpr (E == EL_U8) return ((const uint8_t*)base)[i];
    else return (int)u8_of_unit(ld_f32<E>(base, i));
}
template <int E> __device__ __forceinline__ void st_8bit(void* base, long long i, int v) {
    if constexpr (E == EL_U8) ((uint8_t*)base)[i] = (uint8_t)v;
    else st_f32<E>(base, i, unit_of_u8(v), 0);
}

// f(std::integral_constant<int, E>()) of an entry's element code E = 0..3: how a launcher picks its kernels' instantiation
template <class F> static hipError_t for_elem(int elem, F&& f) {
    switch (elem) {
        case EL_F32: return f(std::integral_constant<int, EL_F32>());
        case EL_BF16: return f(std::integral_constant<int, EL_BF16>());
        case EL_F16: return f(std::integral_constant<int, EL_F16>());
        case EL_U8: return f(std::integral_constant<int, EL_U8>());
        default: return hipErrorInvalidValue;
    }
}

#endif  // __HIPCC__

}  // namespace mz
