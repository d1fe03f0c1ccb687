// gfx950 (MI355X / CDNA4): images with an alpha channel (mz_alpha.h) -- the push-pull fill of the colour under a == 0 and the merge of
// the enlarged alpha plane.  The kernels of one mz_alpha_fill() call, in launch order: alpha_push0_kernel (the views -> level 1),
// alpha_push_kernel (level l -> l + 1, once a level), alpha_pull_kernel (level l from the pulled level l + 1, in place, coarsest first),
// alpha_pull0_kernel (the views and the pulled level 1 -> the result view).  mz_alpha_merge() is alpha_merge_kernel (the alpha plane) and,
// with premultiply, alpha_premultiply_kernel behind it.
// A texel is one 16-byte load or store; every 16-byte store is store16 (mz_view.h); no atomics, no scratch; 64-bit signed addressing.
#include <hip/hip_runtime.h>

#include "mz_alpha.h"
#include "mz_color.h"

namespace mz {

// work item `item` of B * rows * cols, the column fastest, then the row, then the image
struct AlphaItem { long long b; int y, x; };
__device__ __forceinline__ AlphaItem alpha_item(long long item, long long items, int rows, int cols) {
    AlphaItem w;
    if (items <= 0x7fffffffLL) {  // (uniform) the usual case: 32-bit divisions
        const uint32_t it = (uint32_t)item, r = it / (uint32_t)cols;
        w.x = (int)(it - r * (uint32_t)cols);
        w.b = r / (uint32_t)rows;
        w.y = (int)(r - (uint32_t)w.b * (uint32_t)rows);
    } else {
        const long long r = item / cols;
        w.x = (int)(item - r * cols);
        w.b = r / rows;
        w.y = (int)(r - w.b * rows);
    }
    return w;
}

// ---- texels in memory: [B][h][w] of 16 bytes ---------------------------------------------------------------------------------------------
// (an element of the vector is copied into a scalar first: __builtin_bit_cast applied to `v[k]` itself reads element 0 for every k)
__device__ __forceinline__ double texel_component(uint32_t bits) { return (double)__builtin_bit_cast(float, bits); }
__device__ __forceinline__ AlphaTexel texel_ld(const char* level, long long i) {
    const u32x4 v = *(const u32x4*)(level + i * 16);
    return AlphaTexel{texel_component(v[0]), texel_component(v[1]), texel_component(v[2]), texel_component(v[3])};
}
// (the components are float32 values already: alpha_f32)
__device__ __forceinline__ void texel_st(char* level, long long i, const AlphaTexel& t) {
    const u32x4 v = {__builtin_bit_cast(uint32_t, (float)t.w), __builtin_bit_cast(uint32_t, (float)t.r), __builtin_bit_cast(uint32_t, (float)t.g),
                     __builtin_bit_cast(uint32_t, (float)t.b)};
    store16(level + i * 16, v);
}
// U of texel (y, x) of the finer level of image b, from the pulled coarser level `up` of hu x wu
__device__ __forceinline__ AlphaTexel alpha_up_at(const char* up, long long b, int y, int x, int hu, int wu) {
    const int py = y >> 1, px = x >> 1, ny = alpha_neighbour(y, hu), nx = alpha_neighbour(x, wu);
    const long long rp = (b * hu + py) * wu, rn = (b * hu + ny) * wu;
    return alpha_up(texel_ld(up, rp + px), texel_ld(up, rp + nx), texel_ld(up, rn + px), texel_ld(up, rn + nx));
}

// ---- a run of kVec<E> pixels of one row of the views: the raw elements of the three colour planes and of the alpha plane, as 16-byte
// vectors.  `wide`: the run is whole and both views are dense with 16-byte aligned rows -- four 16-byte loads; otherwise the elements
// that exist, one by one, and zeros behind the row's end (a zero alpha element: a == 0, the zero texel)
template <int E>
__device__ __forceinline__ void alpha_load_run(const StridedView& rgb, const StridedView& al, long long b, int y, int x0, int W, bool wide,
                                               u32x4 (&p)[4]) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long cb = b * rgb.s[0] + (long long)y * rgb.s[2], ab = b * al.s[0] + (long long)y * al.s[2];
    if (wide) {
        const char* q = (const char*)rgb.data + (cb + x0) * EB;
        p[0] = *(const u32x4*)q;
        p[1] = *(const u32x4*)(q + rgb.s[1] * EB);
        p[2] = *(const u32x4*)(q + 2 * rgb.s[1] * EB);
        p[3] = *(const u32x4*)((const char*)al.data + (ab + x0) * EB);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (x0 + e < W) {
                const long long at = cb + (long long)(x0 + e) * rgb.s[3];
                vec_put<E>(p[0], e, ld_raw<E>(rgb.data, at));
                vec_put<E>(p[1], e, ld_raw<E>(rgb.data, at + rgb.s[1]));
                vec_put<E>(p[2], e, ld_raw<E>(rgb.data, at + 2 * rgb.s[1]));
                vec_put<E>(p[3], e, ld_raw<E>(al.data, ab + (long long)(x0 + e) * al.s[3]));
            }
        }
    }
}
// the level-0 texel of pixel e of a run
template <int E> __device__ __forceinline__ AlphaTexel alpha_run_texel(const u32x4 (&p)[4], int e, int premultiplied) {
    const double a = alpha_clamp01(f64_of_raw<E>(vec_get<E>(p[3], e)));
    return alpha_texel0(a, alpha_straight(f64_of_raw<E>(vec_get<E>(p[0], e)), a, premultiplied),
                        alpha_straight(f64_of_raw<E>(vec_get<E>(p[1], e)), a, premultiplied),
                        alpha_straight(f64_of_raw<E>(vec_get<E>(p[2], e)), a, premultiplied));
}

// The views -> level 1.  Work item: one run of kVec<E> columns of the rows 2j and 2j + 1, the kVec<E> / 2 texels of row j of level 1 they
// make.  A row or column past the image's end contributes zero texels.
template <int E>
__global__ __launch_bounds__(kAlphaThreads) void alpha_push0_kernel(const StridedView rgb, const StridedView al, char* l1, int H, int W, int H1, int W1,
                                                                    int chunks, long long items, int premultiplied, int xvec) {
    constexpr int V = kVec<E>;
    const long long item = (long long)blockIdx.x * kAlphaThreads + threadIdx.x;
    if (item >= items) return;
    const AlphaItem w = alpha_item(item, items, H1, chunks);
    const int j = w.y, x0 = w.x * V;
    const bool wide = xvec && x0 + V <= W;
    u32x4 p[2][4];
    alpha_load_run<E>(rgb, al, w.b, 2 * j, x0, W, wide, p[0]);
    if (2 * j + 1 < H) {
        alpha_load_run<E>(rgb, al, w.b, 2 * j + 1, x0, W, wide, p[1]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) p[1][c] = u32x4{0u, 0u, 0u, 0u};
    }
    const long long row = (w.b * H1 + j) * W1;
#pragma unroll
    for (int t = 0; t < V / 2; ++t) {
        const int x1 = (x0 >> 1) + t;
        if (x1 < W1)
            texel_st(l1, row + x1,
                     alpha_push(alpha_run_texel<E>(p[0], 2 * t, premultiplied), alpha_run_texel<E>(p[0], 2 * t + 1, premultiplied),
                                alpha_run_texel<E>(p[1], 2 * t, premultiplied), alpha_run_texel<E>(p[1], 2 * t + 1, premultiplied)));
    }
}

// Level l (h x w) -> level l + 1 (hu x wu).  Work item: one texel of level l + 1
__global__ __launch_bounds__(kAlphaThreads) void alpha_push_kernel(const char* lo, char* hi, int h, int w, int hu, int wu, long long items) {
    const long long item = (long long)blockIdx.x * kAlphaThreads + threadIdx.x;
    if (item >= items) return;
    const AlphaItem it = alpha_item(item, items, hu, wu);
    const int y = 2 * it.y, x = 2 * it.x;
    const bool right = x + 1 < w, below = y + 1 < h;
    const long long r0 = (it.b * h + y) * w + x, r1 = r0 + w;
    const AlphaTexel zero = {0.0, 0.0, 0.0, 0.0};
    const AlphaTexel c00 = texel_ld(lo, r0), c01 = right ? texel_ld(lo, r0 + 1) : zero, c10 = below ? texel_ld(lo, r1) : zero,
                     c11 = right && below ? texel_ld(lo, r1 + 1) : zero;
    texel_st(hi, item, alpha_push(c00, c01, c10, c11));
}

// Level l (h x w), in place, from the pulled level l + 1 (hu x wu).  Work item: one texel of level l
__global__ __launch_bounds__(kAlphaThreads) void alpha_pull_kernel(char* lo, const char* hi, int h, int w, int hu, int wu, long long items) {
    const long long item = (long long)blockIdx.x * kAlphaThreads + threadIdx.x;
    if (item >= items) return;
    const AlphaItem it = alpha_item(item, items, h, w);
    texel_st(lo, item, alpha_pull(texel_ld(lo, item), alpha_up_at(hi, it.b, it.y, it.x, hu, wu)));
}

// The pull of level 0 and the result.  Work item: one run of kVec<E> pixels of one row.  A pixel with a > 0 is moved (straight input) or
// un-premultiplied; one with a == 0 reads its four texels of the pulled level 1 (l1 == nullptr: a 1 x 1 image, the result is 0).
// ovec: the result view is dense with 16-byte aligned rows -- whole runs are stored by three store16
template <int E>
__global__ __launch_bounds__(kAlphaThreads) void alpha_pull0_kernel(const StridedView rgb, const StridedView al, const StridedView out, const char* l1,
                                                                    int H, int W, int H1, int W1, int chunks, long long items, int premultiplied,
                                                                    int xvec, int ovec) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long item = (long long)blockIdx.x * kAlphaThreads + threadIdx.x;
    if (item >= items) return;
    const AlphaItem w = alpha_item(item, items, H, chunks);
    const int y = w.y, x0 = w.x * V;
    const bool full = x0 + V <= W, wide_out = ovec && full;
    u32x4 p[4];
    alpha_load_run<E>(rgb, al, w.b, y, x0, W, xvec && full, p);
    const long long ob = w.b * out.s[0] + (long long)y * out.s[2];
    u32x4 o[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int e = 0; e < V; ++e) {
        if (x0 + e >= W) continue;
        const double a = alpha_clamp01(f64_of_raw<E>(vec_get<E>(p[3], e)));
        uint32_t r[3];
        if (a > 0.0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t raw = vec_get<E>(p[c], e);
                r[c] = premultiplied ? luma_round_raw<E>(alpha_straight(f64_of_raw<E>(raw), a, 1), 0) : raw;
            }
        } else {
            AlphaTexel U = {0.0, 0.0, 0.0, 0.0};
            if (l1 != nullptr) U = alpha_up_at(l1, w.b, y, x0 + e, H1, W1);
            r[0] = luma_round_raw<E>(alpha_fill_value(U.w, U.r), 0);
            r[1] = luma_round_raw<E>(alpha_fill_value(U.w, U.g), 0);
            r[2] = luma_round_raw<E>(alpha_fill_value(U.w, U.b), 0);
        }
        if (wide_out) {
#pragma unroll
            for (int c = 0; c < 3; ++c) vec_put<E>(o[c], e, r[c]);
        } else {
            const long long at = ob + (long long)(x0 + e) * out.s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) st_raw<E>((void*)out.data, at + c * out.s[1], r[c]);
        }
    }
    if (wide_out) {
        char* q = (char*)out.data + (ob + x0) * EB;
#pragma unroll
        for (int c = 0; c < 3; ++c) store16(q + c * out.s[1] * EB, o[c]);
    }
}

// The merge's alpha plane.  One workgroup = one kAlphaTileH x kAlphaTileW tile of the Hout x Wout plane of one image; the tile's column
// and row taps go to LDS once (interp_taps), every output gathers its 1, 2 or 4 x 4 source elements and sums them by interp_dot in the
// order of mz_interp.h.  A lane takes 16 bytes of consecutive outputs of one row.  avec: out_alpha is dense with 16-byte aligned rows.
template <int E, int MODE>
__global__ __launch_bounds__(kAlphaThreads) void alpha_merge_kernel(const StridedView al, const StridedView oa, int Hin, int Win, int Hout, int Wout,
                                                                    long long tiles, int tiles_x, int avec) {
    constexpr int TH = kAlphaTileH, TW = kAlphaTileW, NT = kAlphaThreads;
    constexpr int K = interp_count(MODE), V = kVec<E>, CPR = TW / V, EB = kElemBytes<E>;
    constexpr bool kFilter = MODE != IM_NEAREST;
    static_assert(TW % 16 == 0, "a tile row is whole 16-byte chunks of every element type");
    __shared__ int ci[K * TW], ri[K * TH];
    __shared__ double cw[kFilter ? K * TW : 1], rw[kFilter ? K * TH : 1];
    const int tid = threadIdx.x;
    const PlaneTile pt = plane_tile(blockIdx.x, tiles, tiles_x, 1);
    const long long b = pt.b;
    const int i0 = pt.ty * TH, j0 = pt.tx * TW;
    const int th = min(TH, Hout - i0), tw = min(TW, Wout - j0);

    for (int t = tid; t < TW + TH; t += NT) {
        const bool col = t < TW;
        const int l = col ? t : t - TW;
        if (l >= (col ? tw : th)) continue;
        int idx[4];
        double wt[4];
        interp_taps(col ? Win : Hin, col ? Wout : Hout, MODE, (col ? j0 : i0) + l, idx, wt);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (col) ci[k * TW + l] = idx[k];
            else ri[k * TH + l] = idx[k];
            if constexpr (kFilter) {
                if (col) cw[k * TW + l] = wt[k];
                else rw[k * TH + l] = wt[k];
            }
        }
    }
    __syncthreads();

    const long long sbase = b * al.s[0];
    auto hsum = [&](int row, int cc) -> double {  // the horizontal sum of one source row for tile column cc
        double wk[K], vk[K];
        const long long at = sbase + (long long)row * al.s[2];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            wk[k] = cw[k * TW + cc];
            vk[k] = ld_f64<E>(al.data, at + (long long)ci[k * TW + cc] * al.s[3]);
        }
        return interp_dot<K>(wk, vk);
    };

    for (int ch = tid; ch < TH * CPR; ch += NT) {
        const int di = ch / CPR, dj = (ch - di * CPR) * V;
        if (di >= th || dj >= tw) continue;
        int rows[K];
        [[maybe_unused]] double wk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            rows[k] = ri[k * TH + di];
            if constexpr (kFilter) wk[k] = rw[k * TH + di];
        }
        auto value = [&](int cc) -> uint32_t {  // the stored bits of the tile's alpha (di, cc)
            if constexpr (!kFilter) {
                return ld_raw<E>(al.data, sbase + (long long)rows[0] * al.s[2] + (long long)ci[cc] * al.s[3]);
            } else {
                double hk[K];
#pragma unroll
                for (int k = 0; k < K; ++k) hk[k] = hsum(rows[k], cc);
                return luma_round_raw<E>(interp_dot<K>(wk, hk), 1);
            }
        };
        const bool whole = dj + V <= tw;
        const long long aat = b * oa.s[0] + (long long)(i0 + di) * oa.s[2] + (long long)(j0 + dj) * oa.s[3];
        u32x4 va = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < V; ++e) vec_put<E>(va, e, value(min(dj + e, tw - 1)));  // (behind the tile's end: its last column again, not stored)
        if (avec && whole) {
            store16((char*)oa.data + aat * EB, va);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (dj + e < tw) st_raw<E>((void*)oa.data, aat + (long long)e * oa.s[3], vec_get<E>(va, e));
        }
    }
}

// The merge's colour (premultiply only), behind alpha_merge_kernel on the same stream: rgb_out = c A with A read back from out_alpha, the
// value AS STORED.  Work item: one run of kVec<E> pixels of one row; a pixel's colour is read before it is written, by the lane that
// writes it: out_rgb may be the rgb view itself.  wide: the three views are dense with 16-byte aligned rows
template <int E>
__global__ __launch_bounds__(kAlphaThreads) void alpha_premultiply_kernel(const StridedView rgb, const StridedView oa, const StridedView orgb, int H, int W,
                                                                          int chunks, long long items, int vec) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long item = (long long)blockIdx.x * kAlphaThreads + threadIdx.x;
    if (item >= items) return;
    const AlphaItem w = alpha_item(item, items, H, chunks);
    const int y = w.y, x0 = w.x * V;
    const bool wide = vec && x0 + V <= W;
    u32x4 p[4];
    alpha_load_run<E>(rgb, oa, w.b, y, x0, W, wide, p);
    const long long ob = w.b * orgb.s[0] + (long long)y * orgb.s[2];
    u32x4 o[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const double A = f64_of_raw<E>(vec_get<E>(p[3], e));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t r = luma_round_raw<E>(alpha_premultiply(f64_of_raw<E>(vec_get<E>(p[c], e)), A), 0);
            if (wide) vec_put<E>(o[c], e, r);
            else if (x0 + e < W) st_raw<E>((void*)orgb.data, ob + (long long)(x0 + e) * orgb.s[3] + c * orgb.s[1], r);
        }
    }
    if (wide) {
        char* q = (char*)orgb.data + (ob + x0) * EB;
#pragma unroll
        for (int c = 0; c < 3; ++c) store16(q + c * orgb.s[1] * EB, o[c]);
    }
}

// ---- the launchers -----------------------------------------------------------------------------------------------------------------------
// the workgroups of `items` work items, 0 where one grid does not hold them
static unsigned alpha_blocks(__int128 items) {
    const __int128 blocks = (items + kAlphaThreads - 1) / kAlphaThreads;
    return items >= 1 && blocks <= kGridRowMax && grid_ok((long long)blocks) ? (unsigned)blocks : 0u;
}

template <int E> static hipError_t alpha_fill_go(const AlphaFillArgs& a, hipStream_t s) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const AlphaPlan& p = a.plan;
    StridedView al = a.alpha;
    al.s[1] = 0;  // one channel: its stride names nothing
    const int chunks = (int)(((long long)a.W + V - 1) / V);
    const int xvec = a.rgb.s[3] == 1 && al.s[3] == 1 && rows_aligned(a.rgb, a.B, a.H, EB, 16) && rows_aligned(al, a.B, a.H, EB, 16) ? 1 : 0;
    const int ovec = a.out.s[3] == 1 && rows_aligned(a.out, a.B, a.H, EB, 16) ? 1 : 0;
    // every grid before the first launch: a refused call writes nothing
    const __int128 items0 = (__int128)a.B * a.H * chunks;
    if (!alpha_blocks(items0)) return hipErrorInvalidValue;
    for (int l = 1; l < p.n; ++l)
        if (!alpha_blocks((__int128)a.B * p.h[l] * p.w[l])) return hipErrorInvalidValue;
    auto level = [&](int l) { return a.ws + p.off[l]; };
    auto texels = [&](int l) { return (long long)a.B * p.h[l] * p.w[l]; };
    if (p.n > 1) {
        const long long items = (long long)a.B * p.h[1] * chunks;
        hipLaunchKernelGGL((alpha_push0_kernel<E>), dim3(alpha_blocks(items)), dim3(kAlphaThreads), 0, s, a.rgb, al, level(1), a.H, a.W, p.h[1], p.w[1],
                           chunks, items, a.premultiplied, xvec);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        for (int l = 1; l + 1 < p.n; ++l) {
            hipLaunchKernelGGL(alpha_push_kernel, dim3(alpha_blocks(texels(l + 1))), dim3(kAlphaThreads), 0, s, (const char*)level(l), level(l + 1), p.h[l],
                               p.w[l], p.h[l + 1], p.w[l + 1], texels(l + 1));
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
        for (int l = p.n - 2; l >= 1; --l) {
            hipLaunchKernelGGL(alpha_pull_kernel, dim3(alpha_blocks(texels(l))), dim3(kAlphaThreads), 0, s, level(l), (const char*)level(l + 1), p.h[l],
                               p.w[l], p.h[l + 1], p.w[l + 1], texels(l));
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL((alpha_pull0_kernel<E>), dim3(alpha_blocks(items0)), dim3(kAlphaThreads), 0, s, a.rgb, al, a.out,
                       p.n > 1 ? (const char*)level(1) : (const char*)nullptr, a.H, a.W, p.n > 1 ? p.h[1] : 1, p.n > 1 ? p.w[1] : 1, chunks,
                       (long long)items0, a.premultiplied, xvec, ovec);
    return hipGetLastError();
}

int launch_alpha_fill(const AlphaFillArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) { return alpha_fill_go<decltype(e)::value>(a, (hipStream_t)hip_stream); });
}

template <int E, int MODE> static hipError_t alpha_merge_go(const AlphaMergeArgs& a, hipStream_t s) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    TileGrid g;
    if (!plane_tile_grid(a.Hout, a.Wout, kAlphaTileH, kAlphaTileW, a.B, &g, 1)) return hipErrorInvalidValue;
    const int chunks = (int)(((long long)a.Wout + V - 1) / V);
    const __int128 items = (__int128)a.B * a.Hout * chunks;
    if (a.premultiply && !alpha_blocks(items)) return hipErrorInvalidValue;  // both grids before the first launch
    StridedView al = a.alpha, oa = a.out_alpha;
    al.s[1] = oa.s[1] = 0;  // one channel: its stride names nothing
    const int avec = oa.s[3] == 1 && rows_aligned(oa, a.B, a.Hout, EB, 16) ? 1 : 0;
    hipLaunchKernelGGL((alpha_merge_kernel<E, MODE>), dim3((unsigned)g.wgs), dim3(kAlphaThreads), 0, s, al, oa, a.Hin, a.Win, a.Hout, a.Wout, g.tiles,
                       g.tiles_x, avec);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || !a.premultiply) return e;
    const int vec = avec && a.rgb.s[3] == 1 && a.out_rgb.s[3] == 1 && rows_aligned(a.rgb, a.B, a.Hout, EB, 16) &&
                            rows_aligned(a.out_rgb, a.B, a.Hout, EB, 16) ? 1 : 0;
    hipLaunchKernelGGL((alpha_premultiply_kernel<E>), dim3(alpha_blocks(items)), dim3(kAlphaThreads), 0, s, a.rgb, oa, a.out_rgb, a.Hout, a.Wout, chunks,
                       (long long)items, vec);
    return hipGetLastError();
}

int launch_alpha_merge(const AlphaMergeArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        const hipStream_t s = (hipStream_t)hip_stream;
        switch (a.mode) {
            case IM_NEAREST: return alpha_merge_go<E, IM_NEAREST>(a, s);
            case IM_BILINEAR: return alpha_merge_go<E, IM_BILINEAR>(a, s);
            case IM_BICUBIC: return alpha_merge_go<E, IM_BICUBIC>(a, s);
            default: return hipErrorInvalidValue;
        }
    });
}

}  // namespace mz
