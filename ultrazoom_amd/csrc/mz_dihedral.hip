// gfx950 (MI355X / CDNA4): the dihedral transforms and the self-ensemble accumulator (mz_dihedral.h) -- the tile skeleton, the finish
// kernel and the launchers of mz_dihedral(), mz_ensemble_add() and mz_ensemble_finish().
#include <hip/hip_runtime.h>

#include "mz_dihedral.h"

namespace mz {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// how the lanes of a workgroup walk one side of a tile
enum Walk : int { WALK_COLS = 0, WALK_ROWS = 1, WALK_VEC = 2 };  // one element a lane along columns / along rows; 16 bytes a lane along columns

// the `value` of the ensemble: the element as float32 (uint8: the raw sample 0..255, not v / 255 -- sums of eight stay exact integers)
template <int E> __device__ __forceinline__ float value_of(uint32_t raw) {
    if constexpr (E == EL_F32) return __builtin_bit_cast(float, raw);
    else if constexpr (E == EL_BF16) return __builtin_bit_cast(float, raw << 16);
    else if constexpr (E == EL_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)raw);
    else return (float)raw;
}

// grid: tiles * 3 * B workgroups, tile fastest (the tiles of the DESTINATION, row by row).  mz_dihedral.h describes the skeleton and
// the LDS arithmetic.  src_walk / dst_walk: Walk, chosen by the launcher from the strides and alignments of each side.
template <int E, int MODE>
__global__ __launch_bounds__(kDihedralThreads) void dihedral_kernel(const StridedView src, const StridedView dst, int Hs, int Ws, int k, int first,
                                                                     long long tiles, int tiles_x, int src_walk, int dst_walk) {
    constexpr int T = kDihedralTile, P = kDihedralPitch, NT = kDihedralThreads;
    constexpr int DE = MODE == DM_ACC ? (int)EL_F32 : E;  // the destination's element type
    constexpr int VS = kVec<E>, VD = kVec<DE>;
    static_assert(NT % (T / VS) == 0 && NT % (T / VD) == 0 && NT % T == 0, "whole rows of lanes");
    __shared__ uint32_t lds[T * P];
    const int tid = threadIdx.x;
    int Hd, Wd;
    dihedral_shape(k, Hs, Ws, &Hd, &Wd);
    const PlaneTile pt = plane_tile(blockIdx.x, tiles, tiles_x);
    const long long b = pt.b, c = pt.c;
    const int i0 = pt.ty * T, j0 = pt.tx * T;
    const int th = min(T, Hd - i0), tw = min(T, Wd - j0);
    // the source rectangle that lands on this tile: [r0, r0 + nr) x [c0, c0 + nc), from the tile's two corners
    int ra, ca, rb, cb;
    dihedral_source(k, Hs, Ws, i0, j0, &ra, &ca);
    dihedral_source(k, Hs, Ws, i0 + th - 1, j0 + tw - 1, &rb, &cb);
    const int r0 = min(ra, rb), c0 = min(ca, cb);
    const int nr = abs(ra - rb) + 1, nc = abs(ca - cb) + 1;
    const long long sbase = b * src.s[0] + c * src.s[1] + (long long)r0 * src.s[2] + (long long)c0 * src.s[3];
    auto staged = [](uint32_t raw) -> uint32_t {  // what LDS holds of an element
        if constexpr (MODE == DM_ACC) return __builtin_bit_cast(uint32_t, value_of<E>(raw));
        else return raw;
    };

    // ---- accumulate, 16-byte path: this thread's old sums are asked for before the tile is staged, so that their way from HBM
    // overlaps the source's ----
    const long long dbase = b * dst.s[0] + c * dst.s[1] + (long long)i0 * dst.s[2] + (long long)j0 * dst.s[3];
    constexpr int DN = T / VD, DRP = NT / DN;  // the store side's 16-byte walk: chunks a row, rows a step
    const int vdj = (tid % DN) * VD, vrr = tid / DN;
    [[maybe_unused]] f32x4 old[T / DRP];
    if constexpr (MODE == DM_ACC) {
        if (dst_walk == WALK_VEC && !first) {
#pragma unroll
            for (int it = 0; it < T / DRP; ++it) {
                const int di = vrr + it * DRP;
                if (di < th && vdj + VD <= tw) old[it] = *(const f32x4*)((const float*)dst.data + dbase + (long long)di * dst.s[2] + vdj);
            }
        }
    }

    // ---- load: the rectangle, row by row of the source ----
    if (src_walk == WALK_VEC && c0 % VS == 0) {  // (the launcher has checked base and strides: 16-byte alignment then hangs on c0 alone)
        constexpr int N = T / VS, RP = NT / N;
        const int cc = (tid % N) * VS, rr = tid / N;
#pragma unroll
        for (int it = 0; it < T / RP; ++it) {
            const int r = rr + it * RP;
            if (r >= nr) continue;
            const long long at = sbase + (long long)r * src.s[2] + cc;
            if (cc + VS <= nc) {
                const u32x4 v = *(const u32x4*)((const char*)src.data + at * kElemBytes<E>);
#pragma unroll
                for (int e = 0; e < VS; ++e) lds[r * P + cc + e] = staged(vec_get<E>(v, e));
            } else {
                for (int e = 0; cc + e < nc; ++e) lds[r * P + cc + e] = staged(ld_raw<E>(src.data, at + e));
            }
        }
    } else {
        const int fast = tid % T, slow = tid / T;
#pragma unroll 4
        for (int it = 0; it < T / (NT / T); ++it) {
            const int other = slow + it * (NT / T);
            const int r = src_walk == WALK_ROWS ? fast : other, cc = src_walk == WALK_ROWS ? other : fast;
            if (r < nr && cc < nc) lds[r * P + cc] = staged(ld_raw<E>(src.data, sbase + (long long)r * src.s[2] + (long long)cc * src.s[3]));
        }
    }
    __syncthreads();

    // ---- store: the tile, row by row of the destination; element (di, dj) from the LDS slot dihedral_source names ----
    auto slot = [&](int di, int dj) {
        int si, sj;
        dihedral_source(k, Hs, Ws, i0 + di, j0 + dj, &si, &sj);
        return (si - r0) * P + (sj - c0);
    };
    auto put = [&](long long at, uint32_t w) {  // one element
        if constexpr (MODE == DM_ACC) {
            float* p = (float*)dst.data + at;
            const float v = __builtin_bit_cast(float, w);
            *p = first ? v : *p + v;
        } else {
            st_raw<E>((void*)dst.data, at, w);
        }
    };
    if (dst_walk == WALK_VEC) {  // (j0 is a multiple of the tile: every chunk of the tile is aligned once base and strides are)
        const int dj = vdj;
#pragma unroll
        for (int it = 0; it < T / DRP; ++it) {
            const int di = vrr + it * DRP;
            if (di >= th) continue;
            const long long at = dbase + (long long)di * dst.s[2] + dj;
            if (dj + VD <= tw) {
                char* p = (char*)dst.data + at * kElemBytes<DE>;
                u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < VD; ++e) vec_put<DE>(v, e, lds[slot(di, dj + e)]);
                if constexpr (MODE == DM_ACC) {
                    if (!first) v = __builtin_bit_cast(u32x4, old[it] + __builtin_bit_cast(f32x4, v));
                }
                store16(p, v);
            } else {
                for (int e = 0; dj + e < tw; ++e) put(at + e, lds[slot(di, dj + e)]);
            }
        }
    } else {
        const int fast = tid % T, slow = tid / T;
#pragma unroll 4
        for (int it = 0; it < T / (NT / T); ++it) {
            const int other = slow + it * (NT / T);
            const int di = dst_walk == WALK_ROWS ? fast : other, dj = dst_walk == WALK_ROWS ? other : fast;
            if (di < th && dj < tw) put(dbase + (long long)di * dst.s[2] + (long long)dj * dst.s[3], lds[slot(di, dj)]);
        }
    }
}

// The finish of one accumulator element as the stored element's raw bits.  Float types: acc * (1 / n) (exact: n is a power of two), the
// clamp, one rounding to the stored type -- the casts of st_f32 (mz_view.h).  uint8: (2 sum + n) / (2 n) in integers: round half up.
template <int E> __device__ __forceinline__ uint32_t ensemble_mean_raw(float a, float inv_n, int n, int log2n, int clamp) {
    if constexpr (E == EL_U8) {
        return (uint32_t)(2 * (int)a + n) >> (log2n + 1);
    } else {
        float v = a * inv_n;
        if (clamp) v = fminf(fmaxf(v, 0.0f), 1.0f);
        if constexpr (E == EL_F32) return __builtin_bit_cast(uint32_t, v);
        else if constexpr (E == EL_BF16) return __builtin_bit_cast(uint16_t, (__bf16)v);
        else return __builtin_bit_cast(uint16_t, (_Float16)v);
    }
}

constexpr int kFinishSpan = 4 * kDihedralThreads;  // pixels of a row one workgroup finishes

// grid: segs * h * 3 * B workgroups, segment fastest: one workgroup = kFinishSpan pixels of one row of the window of one plane.
// vec: four pixels a lane (a 16-byte read of the accumulator, one 16- / 8- / 4-byte store); else one pixel a lane, four times.
template <int E>
__global__ __launch_bounds__(kDihedralThreads) void ensemble_finish_kernel(const float* acc, const StridedView out, int H, int W, int y0, int x0,
                                                                            int h, int w, int segs, int n, int log2n, int clamp, int vec) {
    const int tid = threadIdx.x;
    const long long wg = blockIdx.x;
    const long long row = wg / segs;  // (b * 3 + c) * h + y
    const int seg = (int)(wg - row * segs);
    const long long plane = row / h;
    const int y = (int)(row - plane * h);
    const long long b = plane / 3, c = plane - b * 3;
    const float* arow = acc + ((plane * H + y0 + y) * (long long)W + x0);
    const long long obase = b * out.s[0] + c * out.s[1] + (long long)y * out.s[2];
    const float inv_n = 1.0f / (float)n;
    auto put = [&](int x) {
        if constexpr (E == EL_U8) st_raw<E>((void*)out.data, obase + (long long)x * out.s[3], ensemble_mean_raw<E>(arow[x], inv_n, n, log2n, clamp));
        else st_f32<E>((void*)out.data, obase + (long long)x * out.s[3], arow[x] * inv_n, clamp);
    };
    const int xs = seg * kFinishSpan;
    if (vec) {
        const int x = xs + 4 * tid;
        if (x + 4 <= w) {
            const f32x4 a = *(const f32x4*)(arow + x);
            uint32_t r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = ensemble_mean_raw<E>(a[e], inv_n, n, log2n, clamp);
            char* p = (char*)out.data + (obase + x) * kElemBytes<E>;
            if constexpr (E == EL_F32) store16(p, u32x4{r[0], r[1], r[2], r[3]});
            else if constexpr (E == EL_U8) *(uint32_t*)p = r[0] | r[1] << 8 | r[2] << 16 | r[3] << 24;
            else *(u32x2*)p = u32x2{r[0] | r[1] << 16, r[2] | r[3] << 16};
        } else {
            for (int e = 0; x + e < w; ++e) put(x + e);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = xs + e * kDihedralThreads + tid;
            if (x < w) put(x);
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
static int walk_of(const StridedView& v, int B, int H, int W, int elem_bytes) {
    if (v.s[3] == 1 || W == 1) return v.s[3] == 1 && rows_aligned(v, B, H, elem_bytes, 16) ? WALK_VEC : WALK_COLS;
    return (v.s[2] == 1 || v.s[2] == -1) && H > 1 ? WALK_ROWS : WALK_COLS;
}

template <int E, int MODE> static hipError_t launch_dihedral_em(const DihedralArgs& a, hipStream_t s) {
    int Hd, Wd;
    dihedral_shape(a.k, a.Hs, a.Ws, &Hd, &Wd);
    TileGrid g;
    if (!plane_tile_grid(Hd, Wd, kDihedralTile, kDihedralTile, a.B, &g)) return hipErrorInvalidValue;
    const int src_walk = walk_of(a.src, a.B, a.Hs, a.Ws, kElemBytes<E>);
    const int dst_walk = walk_of(a.dst, a.B, Hd, Wd, MODE == DM_ACC ? 4 : kElemBytes<E>);
    hipLaunchKernelGGL((dihedral_kernel<E, MODE>), dim3((unsigned)g.wgs), dim3(kDihedralThreads), 0, s, a.src, a.dst, a.Hs, a.Ws, a.k, a.first,
                       g.tiles, g.tiles_x, src_walk, dst_walk);
    return hipGetLastError();
}

int launch_dihedral(const DihedralArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        return a.mode == DM_ACC ? launch_dihedral_em<E, DM_ACC>(a, (hipStream_t)hip_stream) : launch_dihedral_em<E, DM_COPY>(a, (hipStream_t)hip_stream);
    });
}

int launch_ensemble_finish(const EnsembleFinishArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        const int segs = (a.w + kFinishSpan - 1) / kFinishSpan;
        const long long rows = 3LL * a.B * a.h;
        if (!grid_ok(rows, segs)) return hipErrorInvalidValue;
        int log2n = 0;
        while ((1 << log2n) < a.n) ++log2n;
        const bool vec = a.out.s[3] == 1 && rows_aligned(a.out, a.B, a.h, kElemBytes<E>, 4 * kElemBytes<E>) && (uintptr_t)a.acc % 16 == 0 &&
                         a.W % 4 == 0 && a.x0 % 4 == 0;
        hipLaunchKernelGGL((ensemble_finish_kernel<E>), dim3((unsigned)(rows * segs)), dim3(kDihedralThreads), 0, (hipStream_t)hip_stream, a.acc,
                           a.out, a.H, a.W, a.y0, a.x0, a.h, a.w, segs, a.n, log2n, a.clamp, vec ? 1 : 0);
        return hipGetLastError();
    });
}

}  // namespace mz
