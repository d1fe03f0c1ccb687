// gfx950 (MI355X / CDNA4): the degradation family (mz_degrade.h) -- instantiations and the launchers of mz_blur(), mz_noise(), mz_jpeg().
#define MZ_DEGRADE_KERNELS
#include "mz_degrade.h"

namespace mz {

template <int E> static hipError_t launch_blur_e(const DegradeArgs& a, const BlurWeights& bw, hipStream_t s) {
    TileGrid g;
    if (!plane_tile_grid(a.H, a.W, kBlurTile, kBlurTile, a.B, &g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((blur_kernel<E>), dim3((unsigned)g.wgs), dim3(kDegradeThreads), 0, s, a.x, a.out, a.H, a.W, g.tiles, g.tiles_x, bw);
    return hipGetLastError();
}

template <int E> static hipError_t launch_noise_e(const DegradeArgs& a, double sigma, unsigned long long seed, unsigned long long offset, hipStream_t s) {
    // One workgroup a chunk of 256 elements: from 2^32 elements a call on, more than one grid holds (grid_ok), so the call is up to
    // kNoiseLaunches launches of at most kGridRowMax workgroups each -- 2^42 elements a call; the usual call is one launch
    constexpr long long kNoiseLaunches = 1024;
    const long long chunks = (3LL * a.H * a.W + kDegradeThreads - 1) / kDegradeThreads;  // (H, W <= 2^28: below 2^50)
    if (a.B < 1 || chunks < 1 || chunks > kNoiseLaunches * kGridRowMax / a.B) return hipErrorInvalidValue;
    const long long wgs = chunks * a.B;
    for (long long wg0 = 0; wg0 < wgs; wg0 += kGridRowMax) {
        const long long n = wgs - wg0 < kGridRowMax ? wgs - wg0 : kGridRowMax;
        hipLaunchKernelGGL((noise_kernel<E>), dim3((unsigned)n), dim3(kDegradeThreads), 0, s, a.x, a.out, a.H, a.W, chunks, wg0, sigma, seed, offset);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int E> static hipError_t launch_jpeg_e(const DegradeArgs& a, const JpegTables& t, const JpegPlan& pl, char* ws, hipStream_t s) {
    uint8_t* ws_y = (uint8_t*)(ws + pl.off_y);
    uint8_t* ws_c = (uint8_t*)(ws + pl.off_c);
    const int tiles_x = (pl.Wp / 16 + kJpegMcus - 1) / kJpegMcus;
    const long long tiles = (long long)tiles_x * (pl.Hp / 16);
    const long long chunks = ((long long)a.H * a.W + kDegradeThreads - 1) / kDegradeThreads;
    if (!grid_ok(tiles, a.B) || !grid_ok(chunks, a.B)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((jpeg_code_kernel<E>), dim3((unsigned)(tiles * a.B)), dim3(kDegradeThreads), 0, s, a.x, a.H, a.W, pl.Hp, pl.Wp, tiles, tiles_x, t,
                       ws_y, ws_c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((jpeg_image_kernel<E>), dim3((unsigned)(chunks * a.B)), dim3(kDegradeThreads), 0, s, a.out, a.H, a.W, pl.Hp, pl.Wp, chunks,
                       (const uint8_t*)ws_y, (const uint8_t*)ws_c);
    return hipGetLastError();
}

hipError_t launch_blur(const DegradeArgs& a, const BlurWeights& bw, hipStream_t s) {
    return for_elem(a.elem, [&](auto e) { return launch_blur_e<decltype(e)::value>(a, bw, s); });
}

hipError_t launch_noise(const DegradeArgs& a, double sigma, unsigned long long seed, unsigned long long offset, hipStream_t s) {
    return for_elem(a.elem, [&](auto e) { return launch_noise_e<decltype(e)::value>(a, sigma, seed, offset, s); });
}

hipError_t launch_jpeg(const DegradeArgs& a, const JpegTables& t, const JpegPlan& plan, char* ws, hipStream_t s) {
    return for_elem(a.elem, [&](auto e) { return launch_jpeg_e<decltype(e)::value>(a, t, plan, ws, s); });
}

}  // namespace mz
