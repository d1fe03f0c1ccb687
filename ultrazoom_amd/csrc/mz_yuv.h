// 8-bit 4:2:0 YCbCr frames to RGB image views and back (mz_yuv420_to_rgb(), mz_rgb_to_yuv420(): include/mewzoom_hip.h): what video
// decoders and encoders exchange.  No reference counterpart in model.py.  NV12, NV21, I420 and YV12 differ only in where Cb and Cr lie
// and with what column stride: the entries take Y, Cb and Cr as three views, one kernel pair (mz_yuv.hip) serves all four.
//
// THE ARITHMETIC, stated here once (the kernels of mz_yuv.hip and the host's mz_debug_yuv_coeffs compile this source; tests/yuv_ref.py
// restates it in Python).  Float64, sums in a fixed order, one rounding on store.
//     matrix   0 "bt601": Kr = 0.299, Kb = 0.114        1 "bt709": Kr = 0.2126, Kb = 0.0722             Kg = (1.0 - Kr) - Kb
//     range    0 "limited": Yoff = 16, Sy = 219, Sc = 224         1 "full": Yoff = 0, Sy = 255, Sc = 255
//     siting   0 "left": chroma sample i sits on luma column 2i, midway between luma rows 2j and 2j + 1 (MPEG-2 / H.264 / HEVC)
//              1 "center": in the middle of its 2 x 2 luma block (JPEG / MPEG-1)
// Planes: Y [B,1,H,W], Cb and Cr [B,1,Hc,Wc] with Hc = ceil(H / 2), Wc = ceil(W / 2), uint8 CODE VALUES 0..255 (not v / 255).  Odd H
// and W are legal; indices clamp at the edges.
//
// YCbCr -> RGB, per output pixel (y, x):
//     chroma is upsampled in code units, vertically then horizontally:
//         vertical      j = y >> 1, jn = clamp(y even ? j - 1 : j + 1, 0, Hc - 1):   v = 0.75 c[j] + 0.25 c[jn]
//         "center"      the same rule in x
//         "left"        i = x >> 1;  x even: v[i];  x odd: 0.5 v[i] + 0.5 v[min(i + 1, Wc - 1)]
//       every weight is dyadic and every input an 8-bit integer: the kernel forms 16 times the value in integers (chroma_v4, chroma_h16), exact
//     yn = (Y - Yoff) * (1.0 / Sy);   cbn = (cb - 128) * (1.0 / Sc), crn likewise       (the constants are the float64 quotients)
//     R = fma(a_r, crn, yn)                      a_r = 2 (1 - Kr)
//     B = fma(a_b, cbn, yn)                      a_b = 2 (1 - Kb)
//     G = fma(g_b, cbn, fma(g_r, crn, yn))       g_r = -(Kr * a_r) / Kg,  g_b = -(Kb * a_b) / Kg
//     stored with luma_round_raw (mz_color.h): float types an optional clamp to [0, 1], then ONE rounding; uint8 the project's rule
// RGB -> YCbCr, elements read with ld_f64 (mz_view.h):
//     y  = fma(Kb, b, fma(Kg, g, fma(Kr, r, 0.0)));    pb = (b - y) * (0.5 / (1 - Kb));    pr = (r - y) * (0.5 / (1 - Kr))
//     Y code = fma(Sy, y, Yoff), clamped to [0, 255] (a NaN becomes 0), + 0.5, truncated      (no 16..235 clamp: super-white survives)
//     chroma sample (j, i), from the UNROUNDED pb and pr, vertically first:
//         u[x] = 0.5 p[2j][x] + 0.5 p[min(2j + 1, H - 1)][x]
//         "center"      0.5 u[2i] + 0.5 u[min(2i + 1, W - 1)]
//         "left"        (0.25 u[max(2i - 1, 0)] + 0.5 u[2i]) + 0.25 u[min(2i + 1, W - 1)]
//     chroma code = fma(Sc, filtered, 128.0), clamped to [0, 255], + 0.5, truncated
//
// The host part needs no HIP header: plain g++ compiles it.
#pragma once
#include "mz_color.h"

namespace mz {

enum YuvMatrix : int { YUV_BT601 = 0, YUV_BT709 = 1 };
enum YuvRange : int { YUV_LIMITED = 0, YUV_FULL = 1 };
enum YuvSiting : int { YUV_LEFT = 0, YUV_CENTER = 1 };
MZ_HD inline bool yuv_code_valid(int code) { return code == 0 || code == 1; }  // each of the three parameters

struct YuvCoeffs {
    double kr, kg, kb;                    // the luma weights
    double yoff, sy, sc;                  // the range, in code values
    double inv_sy, inv_sc;                // 1.0 / Sy, 1.0 / Sc
    double a_r, a_b, g_r, g_b;            // YCbCr -> RGB
    double pb_scale, pr_scale;            // 0.5 / (1 - Kb), 0.5 / (1 - Kr)
};
MZ_HD inline YuvCoeffs yuv_coeffs(int matrix, int range) {
    YuvCoeffs k;
    k.kr = matrix == YUV_BT709 ? 0.2126 : 0.299;
    k.kb = matrix == YUV_BT709 ? 0.0722 : 0.114;
    k.kg = (1.0 - k.kr) - k.kb;
    k.yoff = range == YUV_FULL ? 0.0 : 16.0;
    k.sy = range == YUV_FULL ? 255.0 : 219.0;
    k.sc = range == YUV_FULL ? 255.0 : 224.0;
    k.inv_sy = 1.0 / k.sy;
    k.inv_sc = 1.0 / k.sc;
    k.a_r = 2.0 * (1.0 - k.kr);
    k.a_b = 2.0 * (1.0 - k.kb);
    k.g_r = -(k.kr * k.a_r) / k.kg;
    k.g_b = -(k.kb * k.a_b) / k.kg;
    k.pb_scale = 0.5 / (1.0 - k.kb);
    k.pr_scale = 0.5 / (1.0 - k.kr);
    return k;
}

// 16 times the upsampled chroma of one output pixel, in integers (at most 16 * 255: exact), in the two steps of the rule above.
// chroma_v4: 4 v of one chroma column from its samples in rows j and jn.  chroma_h16: from 4 v[i] and 4 v[in], where `in` is the horizontal
// neighbour (x even: i - 1 under "center"; x odd: i + 1), clamped
MZ_HD inline int chroma_v4(int c_j, int c_jn) { return 3 * c_j + c_jn; }
MZ_HD inline int chroma_h16(int v4, int vn4, int siting, int x_odd) {
    if (siting == YUV_CENTER) return 3 * v4 + vn4;
    return x_odd ? 2 * (v4 + vn4) : 4 * v4;
}
struct YuvRgb { double r, g, b; };
// one pixel from its Y code and 16 times its two upsampled chroma values.  (up16 - 2048) * (inv_sc / 16) is (cb - 128) * (1.0 / Sc):
// the subtraction is exact and a power of two moves through the one rounding of the product
MZ_HD inline YuvRgb yuv_to_rgb_pixel(const YuvCoeffs& k, int ycode, int cb16, int cr16) {
    const double yn = ((double)ycode - k.yoff) * k.inv_sy;
    const double cbn = (double)(cb16 - 2048) * (k.inv_sc * 0.0625), crn = (double)(cr16 - 2048) * (k.inv_sc * 0.0625);
    return YuvRgb{fma(k.a_r, crn, yn), fma(k.g_b, cbn, fma(k.g_r, crn, yn)), fma(k.a_b, cbn, yn)};
}

struct YuvPixel { double y, pb, pr; };
MZ_HD inline YuvPixel rgb_to_yuv_pixel(const YuvCoeffs& k, double r, double g, double b) {
    const double y = fma(k.kb, b, fma(k.kg, g, fma(k.kr, r, 0.0)));
    return YuvPixel{y, (b - y) * k.pb_scale, (r - y) * k.pr_scale};
}
// a code value 0..255 of scale * v + off: the clamp (a NaN becomes 0), + 0.5, the truncation
MZ_HD inline uint32_t yuv_code(double scale, double v, double off) {
    const double c = fmin(fmax(fma(scale, v, off), 0.0), 255.0);
    return (uint32_t)(uint8_t)(c + 0.5);
}
// a + b of two halves, and the three taps of "left" siting, as the header states them (every product is a power of two times its
// operand: exact, so a contraction of product and sum would not change a bit)
MZ_HD inline double yuv_half_sum(double a, double b) { return 0.5 * a + 0.5 * b; }
MZ_HD inline double yuv_left_sum(double l, double m, double r) { return (0.25 * l + 0.5 * m) + 0.25 * r; }

struct YuvArgs {
    StridedView y, cb, cr;  // [B,1,H,W], [B,1,Hc,Wc] twice, uint8 (s[1] is never used)
    StridedView rgb;        // [B,3,H,W] of `elem`: the output of launch_yuv420_to_rgb, the input of launch_rgb_to_yuv420
    int elem;               // Elem 0..3 of rgb
    int B, H, W;
    int matrix, range, siting;
    int clamp;              // YCbCr -> RGB only
};
// hipError_t values (kept as int: this header stays free of HIP types); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch
int launch_yuv420_to_rgb(const YuvArgs& a, void* hip_stream);
int launch_rgb_to_yuv420(const YuvArgs& a, void* hip_stream);

// How the launchers find the two chroma planes (the kernels' `cmode`): element by element; planar, column stride 1 and rows aligned to
// 8 bytes (8 samples of a plane in one access); interleaved, column stride 2 with the other plane one byte ahead or behind and the pair's
// rows aligned to 16 bytes (8 Cb and 8 Cr in one access: NV12, NV21)
enum ChromaMode : int { CHROMA_ELEMENTS = 0, CHROMA_PLANAR = 1, CHROMA_PAIRS_CB_FIRST = 2, CHROMA_PAIRS_CR_FIRST = 3 };
inline int chroma_mode(const StridedView& cb, const StridedView& cr, int B, int Hc) {
    StridedView a = cb, b = cr;
    a.s[1] = b.s[1] = 0;
    if (a.s[3] == 1 && b.s[3] == 1) return rows_aligned(a, B, Hc, 1, 8) && rows_aligned(b, B, Hc, 1, 8) ? CHROMA_PLANAR : CHROMA_ELEMENTS;
    if (a.s[3] != 2 || b.s[3] != 2 || a.s[0] != b.s[0] || a.s[2] != b.s[2]) return CHROMA_ELEMENTS;
    const intptr_t d = (intptr_t)b.data - (intptr_t)a.data;
    if (d == 1) return rows_aligned(a, B, Hc, 1, 16) ? CHROMA_PAIRS_CB_FIRST : CHROMA_ELEMENTS;
    if (d == -1) return rows_aligned(b, B, Hc, 1, 16) ? CHROMA_PAIRS_CR_FIRST : CHROMA_ELEMENTS;
    return CHROMA_ELEMENTS;
}

}  // namespace mz
