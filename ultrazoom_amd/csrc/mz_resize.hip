// gfx950 (MI355X / CDNA4): the antialiased resampling family (mz_resize.h) -- instantiations and the launcher of one mz_resize() call.
#define MZ_RESIZE_KERNELS
#include "mz_resize.h"

namespace mz {

template <int E> static hipError_t launch_resize_e(const ResizeArgs& a, hipStream_t s) {
    const ResizePlan& pl = a.plan;
    int* span_x = (int*)(a.ws + pl.off_span_x);
    int* span_y = (int*)(a.ws + pl.off_span_y);
    double* w_x = (double*)(a.ws + pl.off_w_x);
    double* w_y = (double*)(a.ws + pl.off_w_y);
    TileGrid g;
    if (!plane_tile_grid(a.h, a.w, kResizeTileH, kResizeTileW, a.B, &g) || pl.lds_bytes > 64 * 1024) return hipErrorInvalidValue;
    const long long table_wgs = ((long long)a.Wout + a.Hout + kResizeThreads - 1) / kResizeThreads;
    hipLaunchKernelGGL(resize_table_kernel, dim3((unsigned)table_wgs), dim3(kResizeThreads), 0, s, a.Hin, a.Win, a.Hout, a.Wout, a.filter,
                       pl.taps_x, pl.taps_y, span_x, w_x, span_y, w_y);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((resize_kernel<E>), dim3((unsigned)g.wgs), dim3(kResizeThreads), pl.lds_bytes, s, a.x, a.out, a.y0, a.x0, a.h, a.w, g.tiles,
                       g.tiles_x, a.clamp, pl.taps_x, pl.taps_y, pl.rows_cap, (const int*)span_x, (const double*)w_x, (const int*)span_y,
                       (const double*)w_y);
    return hipGetLastError();
}

hipError_t launch_resize(const ResizeArgs& a, hipStream_t s) {
    return for_elem(a.elem, [&](auto e) { return launch_resize_e<decltype(e)::value>(a, s); });
}

}  // namespace mz
