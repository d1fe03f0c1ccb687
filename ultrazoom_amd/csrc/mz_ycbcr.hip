// gfx950 (MI355X / CDNA4): YCbCr planes of 8, 10, 12 or 16 bits in 4:2:0, 4:2:2 or 4:4:4 to an RGB image view and back (mz_ycbcr.h) --
// the two streaming kernels and their launchers, one instantiation per element type of the RGB side and per sample type of the planes
// (S = 0: uint8, S = 1: uint16).  Subsampling, siting, depth and alignment are uniform run-time arguments.  The shape of mz_yuv.hip: a
// work item is one run of 16 luma columns.
#include <hip/hip_runtime.h>

#include "mz_ycbcr.h"

namespace mz {

constexpr int kYcThreads = 256;
static_assert(kYcThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kYcRun = 16;  // luma columns of a work item: 16 (uint8) or 2 x 16 (uint16) bytes of Y

typedef uint32_t yc_u32x2 __attribute__((ext_vector_type(2)));

// work item `item` of B * rows * chunks, the run fastest, then the row, then the image (the walk of mz_yuv.hip)
struct YcItem { long long b; int row, x0; };
__device__ __forceinline__ YcItem yc_item(long long item, long long items, int rows, int chunks) {
    YcItem w;
    if (items <= 0x7fffffffLL) {  // (uniform) the usual case: 32-bit divisions
        const uint32_t it = (uint32_t)item, r = it / (uint32_t)chunks;
        w.x0 = (int)(it - r * (uint32_t)chunks) * kYcRun;
        w.b = r / (uint32_t)rows;
        w.row = (int)(r - (uint32_t)w.b * (uint32_t)rows);
    } else {
        const long long r = item / chunks;
        w.x0 = (int)(item - r * chunks) * kYcRun;
        w.b = r / rows;
        w.row = (int)(r - w.b * rows);
    }
    return w;
}

__device__ __forceinline__ int yc_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- samples: one element, and 8 or 16 consecutive ones held in dwords -------------------------------------------------------------------
template <int S> __device__ __forceinline__ uint32_t ld_sample(const void* base, long long i) {
    if constexpr (S) return ((const uint16_t*)base)[i];
    else return ((const uint8_t*)base)[i];
}
template <int S> __device__ __forceinline__ void st_sample(void* base, long long i, uint32_t v) {
    if constexpr (S) ((uint16_t*)base)[i] = (uint16_t)v;
    else ((uint8_t*)base)[i] = (uint8_t)v;
}
template <int S> __device__ __forceinline__ uint32_t sample_of(const uint32_t* w, int e) {
    if constexpr (S) return (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
    else return (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
}
template <int S> __device__ __forceinline__ void sample_put(uint32_t* w, int e, uint32_t v) {
    if constexpr (S) w[e >> 1] |= v << (16 * (e & 1));
    else w[e >> 2] |= v << (8 * (e & 3));
}
// 8 samples at element `at` (a multiple of 8 samples from an aligned row): one 8-byte access of uint8, one 16-byte access of uint16
template <int S> __device__ __forceinline__ void load8(const void* base, long long at, uint32_t (&w)[2 * (S + 1)]) {
    if constexpr (S) {
        const u32x4 v = *(const u32x4*)((const uint16_t*)base + at);
        w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    } else {
        const yc_u32x2 v = *(const yc_u32x2*)((const uint8_t*)base + at);
        w[0] = v[0]; w[1] = v[1];
    }
}
template <int S> __device__ __forceinline__ void store8(void* base, long long at, const uint32_t (&w)[2 * (S + 1)]) {
    if constexpr (S) {
        const u32x4 v = {w[0], w[1], w[2], w[3]};
        store16((uint16_t*)base + at, v);
    } else {
        const yc_u32x2 v = {w[0], w[1]};
        *(yc_u32x2*)((uint8_t*)base + at) = v;
    }
}
// 16 samples (a run of Y; 8 interleaved chroma pairs): one 16-byte access of uint8, two of uint16
template <int S> __device__ __forceinline__ void load16(const void* base, long long at, uint32_t (&w)[4 * (S + 1)]) {
    const char* p = (const char*)base + at * (S + 1);
#pragma unroll
    for (int h = 0; h <= S; ++h) {
        const u32x4 v = *(const u32x4*)(p + 16 * h);
        w[4 * h] = v[0]; w[4 * h + 1] = v[1]; w[4 * h + 2] = v[2]; w[4 * h + 3] = v[3];
    }
}
template <int S> __device__ __forceinline__ void store16s(void* base, long long at, const uint32_t (&w)[4 * (S + 1)]) {
    char* p = (char*)base + at * (S + 1);
#pragma unroll
    for (int h = 0; h <= S; ++h) {
        const u32x4 v = {w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
        store16(p + 16 * h, v);
    }
}

// The codes of samples i_first .. i_first + 7 of one row of both chroma planes.  `fast`: all eight exist and lie as `cmode` says -- one
// load8 a plane, or one load16 of the pairs; otherwise element loads, the index clamped to [0, Wc - 1].  at_b, at_r: the element offset of
// the row in each view (image and row strides applied)
template <int S>
__device__ __forceinline__ void chroma8(const StridedView& cb, const StridedView& cr, long long at_b, long long at_r, int i_first, int Wc, int cmode,
                                        bool fast, const YcbcrWord& wd, int (&ob)[8], int (&orr)[8]) {
    if (fast && cmode == CHROMA_PLANAR) {
        uint32_t wb[2 * (S + 1)], wr[2 * (S + 1)];
        load8<S>(cb.data, at_b + i_first, wb);
        load8<S>(cr.data, at_r + i_first, wr);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ob[k] = ycbcr_read(wd, sample_of<S>(wb, k));
            orr[k] = ycbcr_read(wd, sample_of<S>(wr, k));
        }
    } else if (fast && cmode != CHROMA_ELEMENTS) {
        const bool cb_first = cmode == CHROMA_PAIRS_CB_FIRST;
        uint32_t w[4 * (S + 1)];
        load16<S>(cb_first ? cb.data : cr.data, (cb_first ? at_b : at_r) + 2LL * i_first, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int lo = ycbcr_read(wd, sample_of<S>(w, 2 * k)), hi = ycbcr_read(wd, sample_of<S>(w, 2 * k + 1));
            ob[k] = cb_first ? lo : hi;
            orr[k] = cb_first ? hi : lo;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = yc_clampi(i_first + k, 0, Wc - 1);
            ob[k] = ycbcr_read(wd, ld_sample<S>(cb.data, at_b + (long long)i * cb.s[3]));
            orr[k] = ycbcr_read(wd, ld_sample<S>(cr.data, at_r + (long long)i * cr.s[3]));
        }
    }
}
// samples i0 - 1 + k for k = 0..9 of one row (the ten a run of 16 columns needs under 4:2:0 and 4:2:2): chroma8 and the two at the ends
template <int S>
__device__ __forceinline__ void chroma_row10(const StridedView& cb, const StridedView& cr, long long at_b, long long at_r, int i0, int Wc, int cmode,
                                             bool fast, const YcbcrWord& wd, int (&ob)[10], int (&orr)[10]) {
    int b8[8], r8[8];
    chroma8<S>(cb, cr, at_b, at_r, i0, Wc, cmode, fast, wd, b8, r8);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ob[k + 1] = b8[k];
        orr[k + 1] = r8[k];
    }
    const int il = max(i0 - 1, 0), ir = min(i0 + 8, Wc - 1);
    ob[0] = ycbcr_read(wd, ld_sample<S>(cb.data, at_b + (long long)il * cb.s[3]));
    orr[0] = ycbcr_read(wd, ld_sample<S>(cr.data, at_r + (long long)il * cr.s[3]));
    ob[9] = ycbcr_read(wd, ld_sample<S>(cb.data, at_b + (long long)ir * cb.s[3]));
    orr[9] = ycbcr_read(wd, ld_sample<S>(cr.data, at_r + (long long)ir * cr.s[3]));
}

// YCbCr -> RGB.  Work item: one run of 16 pixels of one output row.  yvec / ovec: Y, and the RGB view, have a column stride of 1 and
// 16-byte aligned rows (the launcher's finding): load16 of Y, 16-byte stores through store16; cmode: ChromaMode.  A row's last, partial
// run and every access of other views go element by element.  No workspace, no LDS, no scratch; 64-bit signed addresses.
template <int E, int S>
__global__ __launch_bounds__(kYcThreads) void ycbcr_to_rgb_kernel(const StridedView yv, const StridedView cb, const StridedView cr, const StridedView out,
                                                                  int H, int W, int chunks, long long items, const YcbcrCoeffs k, int depth, int align,
                                                                  int sub, int siting, int clamp, int yvec, int cmode, int ovec) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long item = (long long)blockIdx.x * kYcThreads + threadIdx.x;
    if (item >= items) return;
    const YcItem w = yc_item(item, items, H, chunks);
    const int y = w.row, x0 = w.x0, Hc = ycbcr_hc(H, sub), Wc = ycbcr_wc(W, sub);
    const bool full = x0 + kYcRun <= W;
    const YcbcrWord wd = ycbcr_word(depth, align);

    // 16 times the upsampled chroma of the 16 pixels
    int cb16[kYcRun], cr16[kYcRun];
    if (sub == YCBCR_444) {  // (uniform)
        const long long ab = w.b * cb.s[0] + (long long)y * cb.s[2], ar = w.b * cr.s[0] + (long long)y * cr.s[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int b8[8], r8[8];
            chroma8<S>(cb, cr, ab, ar, x0 + 8 * h, Wc, cmode, full, wd, b8, r8);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                cb16[8 * h + t] = 16 * b8[t];
                cr16[8 * h + t] = 16 * r8[t];
            }
        }
    } else {
        const int i0 = x0 >> 1, j = sub == YCBCR_420 ? y >> 1 : y;
        int vb[10], vr[10];  // 4 times the vertically filtered chroma of samples i0 - 1 .. i0 + 8
        chroma_row10<S>(cb, cr, w.b * cb.s[0] + (long long)j * cb.s[2], w.b * cr.s[0] + (long long)j * cr.s[2], i0, Wc, cmode, full, wd, vb, vr);
        if (sub == YCBCR_420) {
            const int jn = yc_clampi((y & 1) ? j + 1 : j - 1, 0, Hc - 1);
            int b1[10], r1[10];
            chroma_row10<S>(cb, cr, w.b * cb.s[0] + (long long)jn * cb.s[2], w.b * cr.s[0] + (long long)jn * cr.s[2], i0, Wc, cmode, full, wd, b1, r1);
#pragma unroll
            for (int t = 0; t < 10; ++t) {
                vb[t] = chroma_v4(vb[t], b1[t]);
                vr[t] = chroma_v4(vr[t], r1[t]);
            }
        } else {
#pragma unroll
            for (int t = 0; t < 10; ++t) {
                vb[t] = 4 * vb[t];
                vr[t] = 4 * vr[t];
            }
        }
#pragma unroll
        for (int e = 0; e < kYcRun; ++e) {
            const int i = e >> 1, nb = (e & 1) ? i + 2 : i;  // (sample i0 + i is index i + 1 of vb, vr)
            cb16[e] = chroma_h16(vb[i + 1], vb[nb], siting, e & 1);
            cr16[e] = chroma_h16(vr[i + 1], vr[nb], siting, e & 1);
        }
    }
    const long long yb = w.b * yv.s[0] + (long long)y * yv.s[2], ob = w.b * out.s[0] + (long long)y * out.s[2];
    uint32_t yw[4 * (S + 1)];
    if (full && yvec) {
        load16<S>(yv.data, yb + x0, yw);
    } else {
#pragma unroll
        for (int t = 0; t < 4 * (S + 1); ++t) yw[t] = 0u;
#pragma unroll
        for (int e = 0; e < kYcRun; ++e)
            if (x0 + e < W) sample_put<S>(yw, e, ld_sample<S>(yv.data, yb + (long long)(x0 + e) * yv.s[3]));
    }
    const bool wide = full && ovec;
#pragma unroll
    for (int q = 0; q < kYcRun / V; ++q) {  // one 16-byte run of each output channel
        u32x4 pr = {0u, 0u, 0u, 0u}, pg = pr, pbl = pr;
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const int e = q * V + t;
            const YuvRgb c = ycbcr_to_rgb_pixel(k, ycbcr_read(wd, sample_of<S>(yw, e)), cb16[e], cr16[e]);
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

// The stored words of samples i_first .. i_first + 7 of one row of both chroma planes.  `fast`: all eight exist and lie as `cmode` says:
// planar chroma is one store8 a plane, interleaved chroma one store16s of the 8 pairs; otherwise the samples that exist, one by one
template <int S>
__device__ __forceinline__ void store_chroma8(const StridedView& cb, const StridedView& cr, long long at_b, long long at_r, int i_first, int Wc, int cmode,
                                              bool fast, const uint32_t (&b)[8], const uint32_t (&r)[8]) {
    if (fast && cmode == CHROMA_PLANAR) {
        uint32_t wb[2 * (S + 1)] = {}, wr[2 * (S + 1)] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sample_put<S>(wb, i, b[i]);
            sample_put<S>(wr, i, r[i]);
        }
        store8<S>((void*)cb.data, at_b + i_first, wb);
        store8<S>((void*)cr.data, at_r + i_first, wr);
    } else if (fast && cmode != CHROMA_ELEMENTS) {
        const bool cb_first = cmode == CHROMA_PAIRS_CB_FIRST;
        uint32_t w[4 * (S + 1)] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sample_put<S>(w, 2 * i, cb_first ? b[i] : r[i]);
            sample_put<S>(w, 2 * i + 1, cb_first ? r[i] : b[i]);
        }
        store16s<S>(cb_first ? (void*)cb.data : (void*)cr.data, (cb_first ? at_b : at_r) + 2LL * i_first, w);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i_first + i < Wc) {
                st_sample<S>((void*)cb.data, at_b + (long long)(i_first + i) * cb.s[3], b[i]);
                st_sample<S>((void*)cr.data, at_r + (long long)(i_first + i) * cr.s[3], r[i]);
            }
        }
    }
}

// RGB -> YCbCr.  Work item: one run of 16 columns of the luma rows of one chroma row -- rows 2j and 2j + 1 under 4:2:0, row j otherwise --
// and the 8 (4:4:4: 16) chroma samples they make: every Y and chroma sample is written by exactly one work item, no atomics.  A column past
// the row's end is read at W - 1 and a row past the image's at H - 1 (the clamps of the filters); "left" siting of subsampled chroma also
// reads column x0 - 1.  xvec / yvec: the RGB view, and Y, have a column stride of 1 and 16-byte aligned rows: 16-byte loads, Y stored by
// store16s; cmode: store_chroma8.  No LDS, no scratch; 64-bit signed addresses.
template <int E, int S>
__global__ __launch_bounds__(kYcThreads) void rgb_to_ycbcr_kernel(const StridedView x, const StridedView yv, const StridedView cb, const StridedView cr,
                                                                  int H, int W, int chunks, long long items, const YcbcrCoeffs k, int depth, int align,
                                                                  int sub, int siting, int xvec, int yvec, int cmode) {
    constexpr int V = kVec<E>, EB = kElemBytes<E>;
    const long long item = (long long)blockIdx.x * kYcThreads + threadIdx.x;
    if (item >= items) return;
    const bool v2 = sub == YCBCR_420;  // (uniform) two luma rows a chroma row
    const int Hc = ycbcr_hc(H, sub), Wc = ycbcr_wc(W, sub);
    const YcItem w = yc_item(item, items, Hc, chunks);
    const int j = w.row, x0 = w.x0, y0 = v2 ? 2 * j : j;
    const bool full = x0 + kYcRun <= W, two = v2 && 2 * j + 1 < H;
    const YcbcrWord wd = ycbcr_word(depth, align);
    const YuvCoeffs& kk = k.k;
    const long long xb = w.b * x.s[0];
    const long long xrow[2] = {xb + (long long)y0 * x.s[2], xb + (long long)(v2 ? min(2 * j + 1, H - 1) : y0) * x.s[2]};

    // u of pb and pr, index e + 1 for column x0 + e, index 0 for column x0 - 1 ("left" siting of subsampled chroma only)
    double ub[kYcRun + 1], ur[kYcRun + 1];
    const auto column = [&](int col, uint32_t (&code)[2], double& sb, double& sr) {  // one column of the rows by element loads
        double p[2][2] = {};
        code[1] = 0u;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 0 || v2) {
                const long long at = xrow[r] + (long long)col * x.s[3];
                const YuvPixel px = rgb_to_yuv_pixel(kk, ld_f64<E>(x.data, at), ld_f64<E>(x.data, at + x.s[1]), ld_f64<E>(x.data, at + 2 * x.s[1]));
                code[r] = ycbcr_code(kk.sy, px.y, kk.yoff, k.maxc);
                p[r][0] = px.pb;
                p[r][1] = px.pr;
            }
        }
        sb = v2 ? yuv_half_sum(p[0][0], p[1][0]) : p[0][0];
        sr = v2 ? yuv_half_sum(p[0][1], p[1][1]) : p[0][1];
    };
    ub[0] = ur[0] = 0.0;
    if (siting == YUV_LEFT && sub != YCBCR_444) {
        uint32_t unused[2];
        column(max(x0 - 1, 0), unused, ub[0], ur[0]);
    }
    uint32_t ycodes[2][4 * (S + 1)] = {};
    const bool wide = full && xvec;
#pragma unroll
    for (int q = 0; q < kYcRun / V; ++q) {  // one 16-byte run of each channel of each row
        u32x4 in[2][3] = {};
        if (wide) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (r == 0 || v2) {
                    const char* p = (const char*)x.data + (xrow[r] + x0 + q * V) * EB;
                    in[r][0] = *(const u32x4*)p;
                    in[r][1] = *(const u32x4*)(p + x.s[1] * EB);
                    in[r][2] = *(const u32x4*)(p + 2 * x.s[1] * EB);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < V; ++t) {
            const int e = q * V + t;
            uint32_t code[2] = {0u, 0u};
            if (wide) {
                double p[2][2] = {};
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (r == 0 || v2) {
                        const YuvPixel px = rgb_to_yuv_pixel(kk, f64_of_raw<E>(vec_get<E>(in[r][0], t)), f64_of_raw<E>(vec_get<E>(in[r][1], t)),
                                                             f64_of_raw<E>(vec_get<E>(in[r][2], t)));
                        code[r] = ycbcr_code(kk.sy, px.y, kk.yoff, k.maxc);
                        p[r][0] = px.pb;
                        p[r][1] = px.pr;
                    }
                }
                ub[e + 1] = v2 ? yuv_half_sum(p[0][0], p[1][0]) : p[0][0];
                ur[e + 1] = v2 ? yuv_half_sum(p[0][1], p[1][1]) : p[0][1];
            } else {
                column(min(x0 + e, W - 1), code, ub[e + 1], ur[e + 1]);
            }
            sample_put<S>(ycodes[0], e, ycbcr_write(wd, code[0]));
            sample_put<S>(ycodes[1], e, ycbcr_write(wd, code[1]));
        }
    }
    // Y: row y0 and, under 4:2:0 where the image has it, the row below
    const long long yb = w.b * yv.s[0] + (long long)y0 * yv.s[2];
    if (full && yvec) {
        store16s<S>((void*)yv.data, yb + x0, ycodes[0]);
        if (two) store16s<S>((void*)yv.data, yb + yv.s[2] + x0, ycodes[1]);
    } else {
#pragma unroll
        for (int e = 0; e < kYcRun; ++e) {
            if (x0 + e < W) {
                const long long o = yb + (long long)(x0 + e) * yv.s[3];
                st_sample<S>((void*)yv.data, o, sample_of<S>(ycodes[0], e));
                if (two) st_sample<S>((void*)yv.data, o + yv.s[2], sample_of<S>(ycodes[1], e));
            }
        }
    }
    // chroma row j: the samples of this run that exist
    const long long cbb = w.b * cb.s[0] + (long long)j * cb.s[2], crb = w.b * cr.s[0] + (long long)j * cr.s[2];
    if (sub == YCBCR_444) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t cbc[8], crc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                cbc[i] = ycbcr_write(wd, ycbcr_code(kk.sc, ub[8 * h + i + 1], k.mid, k.maxc));
                crc[i] = ycbcr_write(wd, ycbcr_code(kk.sc, ur[8 * h + i + 1], k.mid, k.maxc));
            }
            store_chroma8<S>(cb, cr, cbb, crb, x0 + 8 * h, Wc, cmode, full, cbc, crc);
        }
    } else {
        uint32_t cbc[8], crc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double fb = siting == YUV_CENTER ? yuv_half_sum(ub[2 * i + 1], ub[2 * i + 2]) : yuv_left_sum(ub[2 * i], ub[2 * i + 1], ub[2 * i + 2]);
            const double fr = siting == YUV_CENTER ? yuv_half_sum(ur[2 * i + 1], ur[2 * i + 2]) : yuv_left_sum(ur[2 * i], ur[2 * i + 1], ur[2 * i + 2]);
            cbc[i] = ycbcr_write(wd, ycbcr_code(kk.sc, fb, k.mid, k.maxc));
            crc[i] = ycbcr_write(wd, ycbcr_code(kk.sc, fr, k.mid, k.maxc));
        }
        store_chroma8<S>(cb, cr, cbb, crb, x0 >> 1, Wc, cmode, full, cbc, crc);
    }
}

// what both launchers share: the grid of B * rows * chunks work items, the views with their unused channel strides cleared
struct YcLaunch { int chunks; long long items; unsigned blocks; StridedView y, cb, cr; int yvec, cmode; };
static bool yc_launch(const YcbcrArgs& a, int rows, YcLaunch* l) {
    const int bytes = a.depth > 8 ? 2 : 1;
    l->chunks = (int)(((long long)a.W + kYcRun - 1) / kYcRun);
    const __int128 items = (__int128)a.B * rows * l->chunks, blocks = (items + kYcThreads - 1) / kYcThreads;
    if (items < 1 || blocks > kGridRowMax || !grid_ok((long long)blocks)) return false;
    l->items = (long long)items;
    l->blocks = (unsigned)blocks;
    l->y = a.y; l->cb = a.cb; l->cr = a.cr;
    l->y.s[1] = l->cb.s[1] = l->cr.s[1] = 0;  // one channel: its stride names nothing
    l->yvec = l->y.s[3] == 1 && rows_aligned(l->y, a.B, a.H, bytes, 16);
    l->cmode = ycbcr_chroma_mode(l->cb, l->cr, a.B, ycbcr_hc(a.H, a.subsampling), bytes);
    return true;
}

template <int E, int S> static hipError_t to_rgb_go(const YcbcrArgs& a, hipStream_t stream) {
    YcLaunch l;
    if (!yc_launch(a, a.H, &l)) return hipErrorInvalidValue;
    const bool ovec = a.rgb.s[3] == 1 && rows_aligned(a.rgb, a.B, a.H, kElemBytes<E>, 16);
    hipLaunchKernelGGL((ycbcr_to_rgb_kernel<E, S>), dim3(l.blocks), dim3(kYcThreads), 0, stream, l.y, l.cb, l.cr, a.rgb, a.H, a.W, l.chunks, l.items,
                       ycbcr_coeffs(a.matrix, a.range, a.depth), a.depth, a.align, a.subsampling, a.siting, a.clamp, l.yvec, l.cmode, ovec ? 1 : 0);
    return hipGetLastError();
}
template <int E, int S> static hipError_t to_ycbcr_go(const YcbcrArgs& a, hipStream_t stream) {
    YcLaunch l;
    if (!yc_launch(a, ycbcr_hc(a.H, a.subsampling), &l)) return hipErrorInvalidValue;
    const bool xvec = a.rgb.s[3] == 1 && rows_aligned(a.rgb, a.B, a.H, kElemBytes<E>, 16);
    hipLaunchKernelGGL((rgb_to_ycbcr_kernel<E, S>), dim3(l.blocks), dim3(kYcThreads), 0, stream, a.rgb, l.y, l.cb, l.cr, a.H, a.W, l.chunks, l.items,
                       ycbcr_coeffs(a.matrix, a.range, a.depth), a.depth, a.align, a.subsampling, a.siting, xvec ? 1 : 0, l.yvec, l.cmode);
    return hipGetLastError();
}

int launch_ycbcr_to_rgb(const YcbcrArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        return a.depth > 8 ? to_rgb_go<E, 1>(a, (hipStream_t)hip_stream) : to_rgb_go<E, 0>(a, (hipStream_t)hip_stream);
    });
}

int launch_rgb_to_ycbcr(const YcbcrArgs& a, void* hip_stream) {
    return (int)for_elem(a.elem, [&](auto e) {
        constexpr int E = decltype(e)::value;
        return a.depth > 8 ? to_ycbcr_go<E, 1>(a, (hipStream_t)hip_stream) : to_ycbcr_go<E, 0>(a, (hipStream_t)hip_stream);
    });
}

}  // namespace mz
