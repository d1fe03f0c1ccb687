// gfx950 (MI355X / CDNA4): plain interpolation of image views (mz_interp.h) -- the tile kernel and the launcher of one mz_interpolate() call.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "mz_interp.h"

namespace mz {

// the one rounding of a result to the stored element, as its raw bits (f32_round_odd: mz_view.h)
template <int E> __device__ __forceinline__ uint32_t interp_round_raw(double v, int clamp) {
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

// grid: tiles * 3 * B workgroups, tile fastest (tiles of the WINDOW, row by row).  vec: the output view is dense with 16-byte aligned
// rows (the launcher's finding); stage: the separable path is allowed (enlarging on both axes, no debug knob)
template <int E, int MODE>
__global__ __launch_bounds__(kInterpThreads) void interp_kernel(const StridedView x, const StridedView out, int Hin, int Win, int Hout, int Wout,
                                                                 int y0, int x0, int h, int w, long long tiles, int tiles_x, int clamp, int vec,
                                                                 int stage) {
    constexpr int TH = kInterpTileH, TW = kInterpTileW, NT = kInterpThreads, SR = kInterpStageRows;
    constexpr int K = interp_count(MODE), V = kVec<E>, CPR = TW / V;  // taps an axis; elements and chunks of 16 bytes a tile row
    constexpr bool kFilter = MODE != IM_NEAREST;
    static_assert((TW & (TW - 1)) == 0 && TW % 16 == 0, "a tile row is whole 16-byte chunks of every element type");
    __shared__ int ci[K * TW], ri[K * TH];                                // the tile's taps, tap-major
    __shared__ double cw[kFilter ? K * TW : 1], rw[kFilter ? K * TH : 1];
    // the horizontal sums, [source row - rmin][element of a chunk][chunk] with one double of padding behind every element's chunks: the
    // lanes of the output phase, one chunk each, read neighbouring doubles (no bank conflict), and the lanes of the horizontal phase, along
    // the columns, write at a pitch that is odd
    constexpr int HP = CPR + 1, ROWP = V * HP;
    __shared__ double hrow[kFilter ? SR * ROWP : 1];
    auto hslot = [](int r, int cc) { return r * ROWP + (cc % V) * HP + cc / V; };
    const int tid = threadIdx.x;
    const PlaneTile pt = plane_tile(blockIdx.x, tiles, tiles_x);
    const long long b = pt.b, c = pt.c;
    const int i0 = pt.ty * TH, j0 = pt.tx * TW;  // inside the window
    const int th = min(TH, h - i0), tw = min(TW, w - j0);

    // ---- the taps of the tile's columns and rows ----
    for (int t = tid; t < TW + TH; t += NT) {
        const bool col = t < TW;
        const int l = col ? t : t - TW;
        if (l >= (col ? tw : th)) continue;
        int idx[4];
        double wt[4];
        interp_taps(col ? Win : Hin, col ? Wout : Hout, MODE, (col ? x0 + j0 : y0 + i0) + l, idx, wt);
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

    const long long sbase = b * x.s[0] + c * x.s[1];
    // h[row] of tile column cc: the horizontal sum of one source row
    auto hsum = [&](int row, int cc) -> double {
        double wk[K], vk[K];
        const long long at = sbase + (long long)row * x.s[2];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            wk[k] = cw[k * TW + cc];
            vk[k] = ld_f64<E>(x.data, at + (long long)ci[k * TW + cc] * x.s[3]);
        }
        return interp_dot<K>(wk, vk);
    };

    // ---- the separable path: the horizontal sums of the source rows [rmin, rmin + nr) under the tile, into LDS ----
    bool staged = false;
    int rmin = 0;
    if constexpr (kFilter) {
        rmin = ri[0];                                   // taps grow with the output index: the first row's first, the last row's last
        const int nr = ri[(K - 1) * TH + th - 1] - rmin + 1;
        staged = stage != 0 && nr <= SR;                // the same for every thread of the workgroup
        if (staged) {
#pragma unroll 2
            for (int it = tid; it < nr * TW; it += NT) {
                const int r = it / TW, cc = it & (TW - 1);
                if (cc < tw) hrow[hslot(r, cc)] = hsum(rmin + r, cc);
            }
        }
        __syncthreads();
    }

    // ---- the outputs: a lane takes 16 bytes of consecutive elements of one row ----
    const long long obase = b * out.s[0] + c * out.s[1];
    for (int ch = tid; ch < TH * CPR; ch += NT) {
        const int di = ch / CPR, dj = (ch - di * CPR) * V;
        if (di >= th || dj >= tw) continue;
        int rows[K];   // the row's taps, once for the chunk
        [[maybe_unused]] double wk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            rows[k] = ri[k * TH + di];
            if constexpr (kFilter) wk[k] = rw[k * TH + di];
        }
        auto value = [&](int cc) -> uint32_t {  // the stored bits of the tile's output (di, cc)
            if constexpr (!kFilter) {
                return ld_raw<E>(x.data, sbase + (long long)rows[0] * x.s[2] + (long long)ci[cc] * x.s[3]);
            } else {
                double hk[K];
#pragma unroll
                for (int k = 0; k < K; ++k) hk[k] = staged ? hrow[hslot(rows[k] - rmin, cc)] : hsum(rows[k], cc);
                return interp_round_raw<E>(interp_dot<K>(wk, hk), clamp);
            }
        };
        const long long at = obase + (long long)(i0 + di) * out.s[2] + (long long)(j0 + dj) * out.s[3];  // (out.data: the window's corner)
        if (vec && dj + V <= tw) {  // (out.s[3] == 1; j0 and dj are multiples of the chunk: aligned once base and strides are)
            u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < V; ++e) vec_put<E>(v, e, value(dj + e));
            store16((char*)out.data + at * kElemBytes<E>, v);
        } else {
            for (int e = 0; e < V && dj + e < tw; ++e) st_raw<E>((void*)out.data, at + (long long)e * out.s[3], value(dj + e));
        }
    }
}

template <int E, int MODE> static hipError_t launch_interp_em(const InterpArgs& a, hipStream_t s) {
    TileGrid g;
    if (!plane_tile_grid(a.h, a.w, kInterpTileH, kInterpTileW, a.B, &g)) return hipErrorInvalidValue;
    const int vec = a.out.s[3] == 1 && rows_aligned(a.out, a.B, a.h, kElemBytes<E>, 16) ? 1 : 0;
    const int stage = a.Hin <= a.Hout && a.Win <= a.Wout && getenv("MZ_INTERP_GATHER") == nullptr ? 1 : 0;
    hipLaunchKernelGGL((interp_kernel<E, MODE>), dim3((unsigned)g.wgs), dim3(kInterpThreads), 0, s, a.x, a.out, a.Hin, a.Win, a.Hout, a.Wout, a.y0,
                       a.x0, a.h, a.w, g.tiles, g.tiles_x, a.clamp, vec, stage);
    return hipGetLastError();
}

int launch_interp(const InterpArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        const hipStream_t s = (hipStream_t)hip_stream;
        switch (a.mode) {
            case IM_NEAREST: return launch_interp_em<E, IM_NEAREST>(a, s);
            case IM_BILINEAR: return launch_interp_em<E, IM_BILINEAR>(a, s);
            case IM_BICUBIC: return launch_interp_em<E, IM_BICUBIC>(a, s);
            default: return hipErrorInvalidValue;
        }
    });
}

}  // namespace mz
