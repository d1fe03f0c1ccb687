// gfx950 (MI355X / CDNA4): 8-bit 4:2:0 YCbCr planes to an RGB image view and back (mz_yuv.h) -- the two streaming kernels and their
// launchers, one instantiation per element type of the RGB side.  NV12, NV21, I420 and YV12 are views of the same three planes.
#include <hip/hip_runtime.h>

#include "mz_yuv.h"

namespace mz {

constexpr int kYuvThreads = 256;
static_assert(kYuvThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kYuvRun = 16;  // luma columns of a work item: one 16-byte run of Y, 8 samples of each chroma plane

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// work item `item` of B * rows * chunks, the run fastest, then the row, then the image (the walk of luma_kernel, mz_color.hip)
struct YuvItem { long long b; int row, x0; };
__device__ __forceinline__ YuvItem yuv_item(long long item, long long items, int rows, int chunks) {
    YuvItem w;
    if (items <= 0x7fffffffLL) {  // (uniform) the usual case: 32-bit divisions
        const uint32_t it = (uint32_t)item, r = it / (uint32_t)chunks;
        w.x0 = (int)(it - r * (uint32_t)chunks) * kYuvRun;
        w.b = r / (uint32_t)rows;
        w.row = (int)(r - (uint32_t)w.b * (uint32_t)rows);
    } else {
        const long long r = item / chunks;
        w.x0 = (int)(item - r * chunks) * kYuvRun;
        w.b = r / rows;
        w.row = (int)(r - w.b * rows);
    }
    return w;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ uint32_t byte_of(const uint32_t* words, int e) { return (words[e >> 2] >> (8 * (e & 3))) & 0xffu; }

// Ten samples of one row of both chroma planes: sample i0 - 1 + k for k = 0..9, the index clamped to [0, Wc - 1].  `fast`: the eight in
// the middle exist and lie as `cmode` says -- one 8-byte load a plane, or one 16-byte load of the pairs; the two at the ends, and every
// sample otherwise, are element loads.  `at` is the element offset of the row in both views (image and row strides applied)
__device__ __forceinline__ void chroma_row(const StridedView& cb, const StridedView& cr, long long at_b, long long at_r, int i0, int Wc, int cmode,
                                           bool fast, int (&ob)[10], int (&orr)[10]) {
    const uint8_t* pb = (const uint8_t*)cb.data;
    const uint8_t* pr = (const uint8_t*)cr.data;
    if (fast && cmode == CHROMA_PLANAR) {
        const u32x2 vb = *(const u32x2*)(pb + at_b + i0), vr = *(const u32x2*)(pr + at_r + i0);
        const uint32_t wb[2] = {vb[0], vb[1]}, wr[2] = {vr[0], vr[1]};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ob[k + 1] = (int)byte_of(wb, k);
            orr[k + 1] = (int)byte_of(wr, k);
        }
    } else if (fast && cmode != CHROMA_ELEMENTS) {
        const bool cb_first = cmode == CHROMA_PAIRS_CB_FIRST;
        const u32x4 v = *(const u32x4*)(cb_first ? pb + at_b + 2LL * i0 : pr + at_r + 2LL * i0);
        const uint32_t w[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int lo = (int)byte_of(w, 2 * k), hi = (int)byte_of(w, 2 * k + 1);
            ob[k + 1] = cb_first ? lo : hi;
            orr[k + 1] = cb_first ? hi : lo;
        }
    } else {
#pragma unroll
        for (int k = 1; k < 9; ++k) {
            const int i = clampi(i0 - 1 + k, 0, Wc - 1);
            ob[k] = pb[at_b + (long long)i * cb.s[3]];
            orr[k] = pr[at_r + (long long)i * cr.s[3]];
        }
    }
    const int il = max(i0 - 1, 0), ir = min(i0 + 8, Wc - 1);
    ob[0] = pb[at_b + (long long)il * cb.s[3]];
    orr[0] = pr[at_r + (long long)il * cr.s[3]];
    ob[9] = pb[at_b + (long long)ir * cb.s[3]];
    orr[9] = pr[at_r + (long long)ir * cr.s[3]];
}

// YCbCr -> RGB.  Work item: one run of 16 pixels of one output row.  yvec / ovec: Y, and the RGB view, have a column stride of 1 and
// 16-byte aligned rows (the launcher's finding): one 16-byte load of Y, 16-byte stores through store16; cmode: ChromaMode.  A row's
// last, partial run and every access of other views go element by element.  No workspace, no LDS, no scratch; 64-bit signed addresses.
template <int E>
__global__ __launch_bounds__(kYuvThreads) void yuv420_to_rgb_kernel(const StridedView yv, const StridedView cb, const StridedView cr, const StridedView out,
                                                                    int H, int W, int chunks, long long items, const YuvCoeffs k, int siting, int clamp,
                                                                    int yvec, int cmode, int ovec) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long item = (long long)blockIdx.x * kYuvThreads + threadIdx.x;
    if (item >= items) return;
    const YuvItem w = yuv_item(item, items, H, chunks);
    const int y = w.row, x0 = w.x0, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1, i0 = x0 >> 1;
    const bool full = x0 + kYuvRun <= W;
    const int j = y >> 1, jn = clampi((y & 1) ? j + 1 : j - 1, 0, Hc - 1);

    // 4 times the vertically filtered chroma of samples i0 - 1 .. i0 + 8
    int vb[10], vr[10];
    {
        int b0[10], r0[10], b1[10], r1[10];
        chroma_row(cb, cr, w.b * cb.s[0] + (long long)j * cb.s[2], w.b * cr.s[0] + (long long)j * cr.s[2], i0, Wc, cmode, full, b0, r0);
        chroma_row(cb, cr, w.b * cb.s[0] + (long long)jn * cb.s[2], w.b * cr.s[0] + (long long)jn * cr.s[2], i0, Wc, cmode, full, b1, r1);
#pragma unroll
        for (int t = 0; t < 10; ++t) {
            vb[t] = chroma_v4(b0[t], b1[t]);
            vr[t] = chroma_v4(r0[t], r1[t]);
        }
    }
    const long long yb = w.b * yv.s[0] + (long long)y * yv.s[2], ob = w.b * out.s[0] + (long long)y * out.s[2];
    uint32_t yw[4];
    if (full && yvec) {
        const u32x4 v = *(const u32x4*)((const uint8_t*)yv.data + yb + x0);
        yw[0] = v[0]; yw[1] = v[1]; yw[2] = v[2]; yw[3] = v[3];
    } else {
        yw[0] = yw[1] = yw[2] = yw[3] = 0u;
#pragma unroll
        for (int e = 0; e < kYuvRun; ++e)
            if (x0 + e < W) yw[e >> 2] |= (uint32_t)((const uint8_t*)yv.data)[yb + (long long)(x0 + e) * yv.s[3]] << (8 * (e & 3));
    }
    const bool wide = full && ovec;
#pragma unroll
    for (int q = 0; q < kYuvRun / V; ++q) {  // one 16-byte run of each output channel
        u32x4 pr = {0u, 0u, 0u, 0u}, pg = pr, pbl = pr;
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const int e = q * V + t, i = e >> 1, nb = (e & 1) ? i + 2 : i;  // (sample i0 + i is index i + 1 of vb, vr)
            const int cb16 = chroma_h16(vb[i + 1], vb[nb], siting, e & 1), cr16 = chroma_h16(vr[i + 1], vr[nb], siting, e & 1);
            const YuvRgb c = yuv_to_rgb_pixel(k, (int)byte_of(yw, e), cb16, cr16);
            const uint32_t rr = luma_round_raw<E>(c.r, clamp), rg = luma_round_raw<E>(c.g, clamp), rb = luma_round_raw<E>(c.b, clamp);
            if (wide) {
                vec_put<E>(pr, t, rr);
                vec_put<E>(pg, t, rg);
                vec_put<E>(pbl, t, rb);
            } else if (x0 + e < W) {
                const long long o = ob + (long long)(x0 + e) * out.s[3];
                st_raw<E>((void*)out.data, o, rr);
                st_raw<E>((void*)out.data, o + out.s[1], rg);
                st_raw<E>((void*)out.data, o + 2 * out.s[1], rb);
            }
        }
        if (wide) {
            char* p = (char*)out.data + (ob + x0 + q * V) * EB;
            store16(p, pr);
            store16(p + out.s[1] * EB, pg);
            store16(p + 2 * out.s[1] * EB, pbl);
        }
    }
}

// RGB -> YCbCr.  Work item: the two luma rows 2j and 2j + 1 of one run of 16 columns, and the 8 samples of chroma row j above them -- every
// Y and chroma sample is written by exactly one work item, no atomics.  A column past the row's end is read at W - 1 and a row past the
// image's at H - 1 (the clamps of the filters); "left" siting also reads column x0 - 1.  xvec / yvec: the RGB view, and Y, have a column
// stride of 1 and 16-byte aligned rows: 16-byte loads, Y stored through store16; cmode: planar chroma is stored 8 bytes a plane,
// interleaved chroma as one store16 of the 8 pairs.  No LDS, no scratch; 64-bit signed addresses.
template <int E>
__global__ __launch_bounds__(kYuvThreads) void rgb_to_yuv420_kernel(const StridedView x, const StridedView yv, const StridedView cb, const StridedView cr,
                                                                    int H, int W, int chunks, long long items, const YuvCoeffs k, int siting, int xvec,
                                                                    int yvec, int cmode) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long item = (long long)blockIdx.x * kYuvThreads + threadIdx.x;
    if (item >= items) return;
    const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const YuvItem w = yuv_item(item, items, Hc, chunks);
    const int j = w.row, x0 = w.x0, i0 = x0 >> 1;
    const bool full = x0 + kYuvRun <= W, two = 2 * j + 1 < H;
    const long long xb = w.b * x.s[0];
    const long long xrow[2] = {xb + (long long)(2 * j) * x.s[2], xb + (long long)min(2 * j + 1, H - 1) * x.s[2]};

    // u of pb and pr, index e + 1 for column x0 + e, index 0 for column x0 - 1 ("left" only)
    double ub[kYuvRun + 1], ur[kYuvRun + 1];
    const auto column = [&](int col, uint32_t (&code)[2], double& sb, double& sr) {  // one column of both rows by element loads
        double p[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long at = xrow[r] + (long long)col * x.s[3];
            const YuvPixel px = rgb_to_yuv_pixel(k, ld_f64<E>(x.data, at), ld_f64<E>(x.data, at + x.s[1]), ld_f64<E>(x.data, at + 2 * x.s[1]));
            code[r] = yuv_code(k.sy, px.y, k.yoff);
            p[r][0] = px.pb;
            p[r][1] = px.pr;
        }
        sb = yuv_half_sum(p[0][0], p[1][0]);
        sr = yuv_half_sum(p[0][1], p[1][1]);
    };
    ub[0] = ur[0] = 0.0;
    if (siting == YUV_LEFT) {
        uint32_t unused[2];
        column(max(x0 - 1, 0), unused, ub[0], ur[0]);
    }
    u32x4 ycodes[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    const bool wide = full && xvec;
#pragma unroll
    for (int q = 0; q < kYuvRun / V; ++q) {  // one 16-byte run of each channel of each row
        u32x4 in[2][3] = {};
        if (wide) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const char* p = (const char*)x.data + (xrow[r] + x0 + q * V) * EB;
                in[r][0] = *(const u32x4*)p;
                in[r][1] = *(const u32x4*)(p + x.s[1] * EB);
                in[r][2] = *(const u32x4*)(p + 2 * x.s[1] * EB);
            }
        }
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const int e = q * V + t;
            uint32_t code[2];
            if (wide) {
                double p[2][2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const YuvPixel px = rgb_to_yuv_pixel(k, f64_of_raw<E>(vec_get<E>(in[r][0], t)), f64_of_raw<E>(vec_get<E>(in[r][1], t)),
                                                         f64_of_raw<E>(vec_get<E>(in[r][2], t)));
                    code[r] = yuv_code(k.sy, px.y, k.yoff);
                    p[r][0] = px.pb;
                    p[r][1] = px.pr;
                }
                ub[e + 1] = yuv_half_sum(p[0][0], p[1][0]);
                ur[e + 1] = yuv_half_sum(p[0][1], p[1][1]);
            } else {
                column(min(x0 + e, W - 1), code, ub[e + 1], ur[e + 1]);
            }
            vec_put<EL_U8>(ycodes[0], e, code[0]);
            vec_put<EL_U8>(ycodes[1], e, code[1]);
        }
    }
    // Y: rows 2j and, where the image has it, 2j + 1
    const long long yb = w.b * yv.s[0] + (long long)(2 * j) * yv.s[2];
    if (full && yvec) {
        store16((uint8_t*)yv.data + yb + x0, ycodes[0]);
        if (two) store16((uint8_t*)yv.data + yb + yv.s[2] + x0, ycodes[1]);
    } else {
#pragma unroll
        for (int e = 0; e < kYuvRun; ++e) {
            if (x0 + e < W) {
                const long long o = yb + (long long)(x0 + e) * yv.s[3];
                ((uint8_t*)yv.data)[o] = (uint8_t)vec_get<EL_U8>(ycodes[0], e);
                if (two) ((uint8_t*)yv.data)[o + yv.s[2]] = (uint8_t)vec_get<EL_U8>(ycodes[1], e);
            }
        }
    }
    // chroma row j: samples i0 .. i0 + 7 that exist
    uint32_t cbc[8], crc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double fb = siting == YUV_CENTER ? yuv_half_sum(ub[2 * i + 1], ub[2 * i + 2]) : yuv_left_sum(ub[2 * i], ub[2 * i + 1], ub[2 * i + 2]);
        const double fr = siting == YUV_CENTER ? yuv_half_sum(ur[2 * i + 1], ur[2 * i + 2]) : yuv_left_sum(ur[2 * i], ur[2 * i + 1], ur[2 * i + 2]);
        cbc[i] = yuv_code(k.sc, fb, 128.0);
        crc[i] = yuv_code(k.sc, fr, 128.0);
    }
    const long long cbb = w.b * cb.s[0] + (long long)j * cb.s[2], crb = w.b * cr.s[0] + (long long)j * cr.s[2];
    if (full && cmode == CHROMA_PLANAR) {
        u32x2 pb = {0u, 0u}, pr = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            pb[i >> 2] |= cbc[i] << (8 * (i & 3));
            pr[i >> 2] |= crc[i] << (8 * (i & 3));
        }
        *(u32x2*)((uint8_t*)cb.data + cbb + i0) = pb;
        *(u32x2*)((uint8_t*)cr.data + crb + i0) = pr;
    } else if (full && cmode != CHROMA_ELEMENTS) {
        const bool cb_first = cmode == CHROMA_PAIRS_CB_FIRST;
        u32x4 pairs = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            vec_put<EL_U8>(pairs, 2 * i, cb_first ? cbc[i] : crc[i]);
            vec_put<EL_U8>(pairs, 2 * i + 1, cb_first ? crc[i] : cbc[i]);
        }
        store16(cb_first ? (uint8_t*)cb.data + cbb + 2LL * i0 : (uint8_t*)cr.data + crb + 2LL * i0, pairs);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i0 + i < Wc) {
                ((uint8_t*)cb.data)[cbb + (long long)(i0 + i) * cb.s[3]] = (uint8_t)cbc[i];
                ((uint8_t*)cr.data)[crb + (long long)(i0 + i) * cr.s[3]] = (uint8_t)crc[i];
            }
        }
    }
}

// what both launchers share: the grid of B * rows * chunks work items, the views with their unused channel strides cleared
struct YuvLaunch { int chunks; long long items; unsigned blocks; StridedView y, cb, cr; int yvec, cmode; };
static bool yuv_launch(const YuvArgs& a, int rows, YuvLaunch* l) {
    l->chunks = (int)(((long long)a.W + kYuvRun - 1) / kYuvRun);
    const __int128 items = (__int128)a.B * rows * l->chunks, blocks = (items + kYuvThreads - 1) / kYuvThreads;
    if (items < 1 || blocks > kGridRowMax || !grid_ok((long long)blocks)) return false;
    l->items = (long long)items;
    l->blocks = (unsigned)blocks;
    l->y = a.y; l->cb = a.cb; l->cr = a.cr;
    l->y.s[1] = l->cb.s[1] = l->cr.s[1] = 0;  // one channel: its stride names nothing
    l->yvec = l->y.s[3] == 1 && rows_aligned(l->y, a.B, a.H, 1, 16);
    l->cmode = chroma_mode(l->cb, l->cr, a.B, (a.H + 1) / 2);
    return true;
}

int launch_yuv420_to_rgb(const YuvArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        YuvLaunch l;
        if (!yuv_launch(a, a.H, &l)) return hipErrorInvalidValue;
        const bool ovec = a.rgb.s[3] == 1 && rows_aligned(a.rgb, a.B, a.H, kElemBytes<E>, 16);
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<E>), dim3(l.blocks), dim3(kYuvThreads), 0, (hipStream_t)hip_stream, l.y, l.cb, l.cr, a.rgb, a.H, a.W,
                           l.chunks, l.items, yuv_coeffs(a.matrix, a.range), a.siting, a.clamp, l.yvec, l.cmode, ovec ? 1 : 0);
        return hipGetLastError();
    });
}

int launch_rgb_to_yuv420(const YuvArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        YuvLaunch l;
        if (!yuv_launch(a, (a.H + 1) / 2, &l)) return hipErrorInvalidValue;
        const bool xvec = a.rgb.s[3] == 1 && rows_aligned(a.rgb, a.B, a.H, kElemBytes<E>, 16);
        hipLaunchKernelGGL((rgb_to_yuv420_kernel<E>), dim3(l.blocks), dim3(kYuvThreads), 0, (hipStream_t)hip_stream, a.rgb, l.y, l.cb, l.cr, a.H, a.W,
                           l.chunks, l.items, yuv_coeffs(a.matrix, a.range), a.siting, xvec ? 1 : 0, l.yvec, l.cmode);
        return hipGetLastError();
    });
}

}  // namespace mz
