// An image view as the kernels of mz_metrics.h, mz_resize.h, mz_degrade.h, mz_interp.h and mz_dihedral.h take it, the element codes,
// every conversion between a stored element and the value it stands for, and what those kernels and their launchers share below that
// -- stated here once (the convolution kernels' view path, ImageViews / StemView, is separate; mz_view_check.h holds the host's checks
// of the public mz_image_view).  A uint8 element v stands for v / 255: read by a TRUE division, stored as clamp -> * 255 + 0.5 ->
// truncate, exactly mz_forward_u8's rule; the float accessors do that in float32, the double ones in float64.
//   host (no HIP header: plain g++ compiles it, tests/view_check_main.cpp runs it under the sanitizers): the struct, the enum, the grid
//     of a plane-tile launch (plane_tile_grid, grid_ok), rows_aligned, dense_view
//   device (under hipcc only, for translation units that have included <hip/hip_runtime.h>): the accessors, the raw-element and 16-byte
//     vector helpers, store16() -- the ONE place a 16-byte global store of an image kernel is written -- and plane_tile(), the walk that
//     takes a workgroup index apart
#pragma once
#include <stdint.h>

namespace mz {

struct StridedView {
    const void* data;  // element (image 0, channel 0, row 0, column 0); of a windowed output: the window's first element
    long long s[4];    // element strides: image, channel, row, column (signed)
};

// the `elem` of the view entries; EL_F64 is internal (the VIF pyramid in mz_metrics' workspace)
enum Elem : int { EL_F32 = 0, EL_BF16 = 1, EL_F16 = 2, EL_U8 = 3, EL_F64 = 4 };

// ---- the launchers' side --------------------------------------------------------------------------------------------------------
// A grid dimension holds at most 2^32 - 1 WORK-ITEMS: the dispatch packet counts a dimension's work-items in 32 bits, and HIP launches
// a larger grid cut to the count modulo 2^32 WITHOUT an error -- the workgroups past it never run (measured: EXPERIMENTS.md, "Large-index
// tests").  Every image kernel runs workgroups of kImageThreads threads, so one grid dimension holds 2^24 - 1 of them.
constexpr int kImageThreads = 256;
constexpr long long kGridRowMax = 0xffffffffLL / kImageThreads;
// a one-dimensional grid of wgs * per workgroups can be launched: 1 .. 2^24 - 1 (no product is formed here: the caller's fits once this
// says so)
inline bool grid_ok(long long wgs, long long per = 1) { return wgs > 0 && per > 0 && wgs <= kGridRowMax / per; }

// THE GRID CONVENTION of the plane-tile kernels (interp, dihedral, resize, blur, moments): tiles * C * B workgroups, tile fastest -- the
// tile_h x tile_w tiles of an h x w rectangle row by row, then the channel, then the image; plane_tile() below takes an index apart.
// C is 3 everywhere but in the metrics of a luma plane (mz_metrics_luma: C = 1).
struct TileGrid { int tiles_x, tiles_y; long long tiles, wgs; };  // tiles = tiles_x * tiles_y; wgs = tiles * C * B
// false where wgs is not in [1, kGridRowMax] (nothing is multiplied before it is known to fit: sides of 2^28 in 1 x 1 tiles are refused)
inline bool plane_tile_grid(int h, int w, int tile_h, int tile_w, int B, TileGrid* g, int C = 3) {
    if (h < 1 || w < 1 || tile_h < 1 || tile_w < 1 || B < 1 || C < 1) return false;
    g->tiles_x = (int)(((long long)w + tile_w - 1) / tile_w);
    g->tiles_y = (int)(((long long)h + tile_h - 1) / tile_h);
    g->tiles = (long long)g->tiles_x * g->tiles_y;
    if (!grid_ok(g->tiles, (long long)C * B)) return false;
    g->wgs = g->tiles * C * B;
    return true;
}

// every address of a [B,3,H,*] view's rows is a multiple of `bytes`: the base and the strides of the dimensions that have a second step
inline bool rows_aligned(const StridedView& v, int B, int H, int elem_bytes, int bytes) {
    if ((uintptr_t)v.data % bytes) return false;
    const long long per = bytes / elem_bytes;
    return (B == 1 || v.s[0] % per == 0) && v.s[1] % per == 0 && (H == 1 || v.s[2] % per == 0);
}

// a dense [B,C,H,W] array as a view (sides of 2^28: the image stride is C * 2^56)
inline StridedView dense_view(const void* data, int H, int W, int C = 3) {
    return StridedView{data, {(long long)C * H * W, (long long)H * W, W, 1}};
}

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

// ---- raw elements and 16-byte vectors of them (the kernels that move bit patterns: interp's nearest, dihedral) ----------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int E> constexpr int kElemBytes = E == EL_F32 ? 4 : E == EL_U8 ? 1 : 2;
template <int E> constexpr int kVec = 16 / kElemBytes<E>;  // elements of one 16-byte access

// an element as it lies in memory, zero-extended to a dword, and back (nearest moves bit patterns)
template <int E> __device__ __forceinline__ uint32_t ld_raw(const void* base, long long i) {
    if constexpr (E == EL_F32) return ((const uint32_t*)base)[i];
    else if constexpr (E == EL_U8) return ((const uint8_t*)base)[i];
    else return ((const uint16_t*)base)[i];
}
template <int E> __device__ __forceinline__ void st_raw(void* base, long long i, uint32_t v) {
    if constexpr (E == EL_F32) ((uint32_t*)base)[i] = v;
    else if constexpr (E == EL_U8) ((uint8_t*)base)[i] = (uint8_t)v;
    else ((uint16_t*)base)[i] = (uint16_t)v;
}
// element e of a 16-byte vector of kVec<E> elements, and its place in one
template <int E> __device__ __forceinline__ uint32_t vec_get(const u32x4& v, int e) {
    if constexpr (E == EL_F32) return v[e];
    else if constexpr (E == EL_U8) return (v[e >> 2] >> (8 * (e & 3))) & 0xffu;
    else return (v[e >> 1] >> (16 * (e & 1))) & 0xffffu;
}
template <int E> __device__ __forceinline__ void vec_put(u32x4& v, int e, uint32_t raw) {
    if constexpr (E == EL_F32) v[e] = raw;
    else if constexpr (E == EL_U8) v[e >> 2] |= raw << (8 * (e & 3));
    else v[e >> 1] |= raw << (16 * (e & 1));
}

// A 16-byte global store with the wait states gfx950 needs behind it PINNED (the store reads its data registers
// late; hipcc pads one wait state, the probe of tests/test_store_hazard_gpu.py wants two): the store and `s_nop 1` in one statement,
// which the scheduler cannot part.  Every 16-byte store of the image kernels goes through here; tools/asm_store_hazard.py re-checks
// the listings.
__device__ __forceinline__ void store16(void* p, const u32x4& v) {
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// ---- the tile walk: workgroup wg of the grid plane_tile_grid() describes (tiles * C * B workgroups, tile fastest) -------------------
struct PlaneTile { long long b, c; int ty, tx; };  // image, channel, tile row, tile column
__device__ __forceinline__ PlaneTile plane_tile(long long wg, long long tiles, int tiles_x, int C = 3) {
    const long long plane = wg / tiles;  // b * C + c
    const int tile = (int)(wg - plane * tiles);
    const long long b = plane / C, c = plane - b * C;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    return PlaneTile{b, c, ty, tx};
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
