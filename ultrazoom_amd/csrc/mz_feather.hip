// gfx950 (MI355X / CDNA4): the paste of feathered tiling (mz_feather.h) -- feather_paste_kernel and its launcher.  One pass over the
// rectangle: outside both ramps src is moved onto dst (one read, one write; dst is not read), inside them the two are blended in
// float64.  Every 16-byte store is store16 (mz_view.h); no LDS, no atomics, no workspace, no scratch; 64-bit signed addressing.
#include <hip/hip_runtime.h>

#include "mz_feather.h"

namespace mz {

// the value the blend takes an element for: the float types as ld_f64 reads them, uint8 the code 0..255 itself
template <int E> __device__ __forceinline__ double feather_value(uint32_t raw) {
    if constexpr (E == EL_U8) return (double)raw;
    else return f64_of_raw<E>(raw);
}
// the one rounding of v to the stored element, as its raw bits (no clamp)
template <int E> __device__ __forceinline__ uint32_t feather_round_raw(double v) {
    if constexpr (E == EL_U8) return (uint32_t)feather_code(v);
    else return luma_round_raw<E>(v, 0);
}
// the raw bits dst receives: s and d the raw bits of the two elements, w their weight
template <int E> __device__ __forceinline__ uint32_t feather_element(uint32_t s, uint32_t d, double w) {
    if (w == 1.0 || s == d) return s;  // the select
    return feather_round_raw<E>(feather_mix(feather_value<E>(s), feather_value<E>(d), w));
}

// grid: tiles * 3 * B workgroups, tile fastest: one workgroup = kFeatherRows rows of kFeatherRuns runs of kVec<E> columns of one plane.
// vec: both views have a column stride of 1 and 16-byte aligned rows -- a lane takes one run of every eighth row, 16 bytes a load and a
// store; a run wholly outside both ramps (y >= ny and its first column >= nx) is moved without a look at dst and without float64.
// Otherwise a lane takes single elements, neighbouring lanes neighbouring columns.
template <int E>
__global__ __launch_bounds__(kFeatherThreads) void feather_paste_kernel(const StridedView src, const StridedView dst, int H, int W, int ny, int nx,
                                                                        double rho_y, double rho_x, long long tiles, int tiles_x, int vec) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>, TW = kFeatherRuns * V, RP = kFeatherThreads / kFeatherRuns;
    const int tid = threadIdx.x;
    const PlaneTile pt = plane_tile(blockIdx.x, tiles, tiles_x);
    const int i0 = pt.ty * kFeatherRows, j0 = pt.tx * TW;
    const int run = tid % kFeatherRuns, rr = tid / kFeatherRuns;
    const long long sb = pt.b * src.s[0] + pt.c * src.s[1], db = pt.b * dst.s[0] + pt.c * dst.s[1];

    auto one = [&](int y, int x, double wy) {  // one element
        const long long so = sb + (long long)y * src.s[2] + (long long)x * src.s[3];
        const long long dd = db + (long long)y * dst.s[2] + (long long)x * dst.s[3];
        const uint32_t s = ld_raw<E>(src.data, so);
        if (y >= ny && x >= nx) {
            st_raw<E>((void*)dst.data, dd, s);
            return;
        }
        const uint32_t d = ld_raw<E>(dst.data, dd);
        st_raw<E>((void*)dst.data, dd, feather_element<E>(s, d, feather_weight(wy, feather_omega(nx, rho_x, x))));
    };

    if (vec) {
        const int x0 = j0 + run * V;
        if (x0 >= W) return;
        const bool whole = x0 + V <= W;
#pragma unroll
        for (int it = 0; it < kFeatherRows / RP; ++it) {
            const int y = i0 + rr + it * RP;
            if (y >= H) continue;
            const double wy = feather_omega(ny, rho_y, y);
            if (!whole) {
                for (int e = 0; x0 + e < W; ++e) one(y, x0 + e, wy);
                continue;
            }
            const u32x4 s = *(const u32x4*)((const char*)src.data + (sb + (long long)y * src.s[2] + x0) * EB);
            char* q = (char*)dst.data + (db + (long long)y * dst.s[2] + x0) * EB;
            if (y >= ny && x0 >= nx) {
                store16(q, s);
                continue;
            }
            const u32x4 d = *(const u32x4*)q;
            u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < V; ++e)
                vec_put<E>(o, e, feather_element<E>(vec_get<E>(s, e), vec_get<E>(d, e), feather_weight(wy, feather_omega(nx, rho_x, x0 + e))));
            store16(q, o);
        }
    } else {
#pragma unroll 1
        for (int it = 0; it < kFeatherRows / RP; ++it) {
            const int y = i0 + rr + it * RP;
            if (y >= H) break;
            const double wy = feather_omega(ny, rho_y, y);
#pragma unroll 4
            for (int e = 0; e < V; ++e) {
                const int x = j0 + e * kFeatherRuns + run;
                if (x < W) one(y, x, wy);
            }
        }
    }
}

template <int E> static hipError_t feather_go(const FeatherArgs& a, hipStream_t s) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    TileGrid g;
    if (!plane_tile_grid(a.H, a.W, kFeatherRows, kFeatherRuns * V, a.B, &g)) return hipErrorInvalidValue;
    const int vec = a.src.s[3] == 1 && a.dst.s[3] == 1 && rows_aligned(a.src, a.B, a.H, EB, 16) && rows_aligned(a.dst, a.B, a.H, EB, 16) ? 1 : 0;
    hipLaunchKernelGGL((feather_paste_kernel<E>), dim3((unsigned)g.wgs), dim3(kFeatherThreads), 0, s, a.src, a.dst, a.H, a.W, a.ramp_y, a.ramp_x,
                       feather_rho(a.ramp_y), feather_rho(a.ramp_x), g.tiles, g.tiles_x, vec);
    return hipGetLastError();
}

int launch_feather_paste(const FeatherArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) { return feather_go<decltype(e)::value>(a, (hipStream_t)hip_stream); });
}

}  // namespace mz
