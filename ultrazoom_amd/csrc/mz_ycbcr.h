// YCbCr frames of 8, 10, 12 or 16 bits in 4:2:0, 4:2:2 or 4:4:4 to RGB image views and back (mz_ycbcr_to_rgb(), mz_rgb_to_ycbcr():
// include/mewzoom_hip.h): P010 / P012 / P016, yuv420p10le and its kin, NV16 / NV24, I422 / I444, BT.2020.  mz_yuv.h generalised over four
// parameters; where a parameter takes mz_yuv.h's value every operation and its order are the ones stated there -- depth 8, 4:2:0 and
// matrix 0 or 1 give the bits of mz_yuv420_to_rgb / mz_rgb_to_yuv420.  No reference counterpart in model.py.
//
// THE ARITHMETIC, stated here once (the kernels of mz_ycbcr.hip and the host's mz_debug_ycbcr_coeffs compile this source;
// tests/ycbcr_ref.py restates it in Python).  Float64, sums in a fixed order, one rounding on store.  Only what differs from mz_yuv.h:
//     depth    d in {8, 10, 12, 16}: planes hold uint8 code values when d == 8, host-endian uint16 otherwise; strides count elements.
//              s = 2^(d - 8).   "limited": Yoff = 16 s, Sy = 219 s, Sc = 224 s      "full": Yoff = 0, Sy = Sc = 2^d - 1
//              chroma midpoint mid = 2^(d - 1); codes clamp to [0, 2^d - 1]; the reciprocals are the float64 quotients 1.0 / Sy, 1.0 / Sc
//     align    of a 16-bit container, shift = 16 - d:   0 "low": a code is word & (2^d - 1) and is written as it is (yuv420p10le, ..)
//                                                       1 "high": a code is word >> shift and is written as code << shift (P010, P012, P016)
//              with d == 8 or d == 16 both mean the same
//     subsampling   chroma planes [B,1,Hc,Wc]:   0 "420": Hc = ceil(H / 2), Wc = ceil(W / 2), the rules of mz_yuv.h
//              1 "422": Hc = H, Wc = ceil(W / 2).  No vertical filter: upsampling takes 4 c[y] for chroma_v4 (what 0.75 c + 0.25 c is,
//                       exactly), subsampling takes u = p[y]; the horizontal rules of the siting as in mz_yuv.h
//              2 "444": Hc = H, Wc = W.  No filter: 16 times the upsampled chroma is 16 c[y][x], a chroma sample is made of p[y][x]
//     matrix   2 "bt2020": Kr = 0.2627, Kb = 0.0593 (non-constant luminance)
// YCbCr -> RGB:   yn = (Y - Yoff) * (1.0 / Sy);   cbn = (up16 - 16 mid) * ((1.0 / Sc) * 0.0625);  R, G, B by the three fma of mz_yuv.h
//     (up16, 16 times the upsampled chroma, is an integer of at most 16 * 65535: exact)
// RGB -> YCbCr:   rgb_to_yuv_pixel of mz_yuv.h;  Y code = fma(Sy, y, Yoff), chroma code = fma(Sc, filtered, mid), each clamped to
//     [0, 2^d - 1] (a NaN becomes 0), + 0.5, truncated
//
// The host part needs no HIP header: plain g++ compiles it.
#pragma once
#include "mz_yuv.h"

namespace mz {

enum YcbcrMatrix : int { YCBCR_BT2020 = 2 };  // 0 and 1: YuvMatrix
enum YcbcrAlign : int { YCBCR_LOW = 0, YCBCR_HIGH = 1 };
enum YcbcrSubsampling : int { YCBCR_420 = 0, YCBCR_422 = 1, YCBCR_444 = 2 };
MZ_HD inline bool ycbcr_depth_valid(int d) { return d == 8 || d == 10 || d == 12 || d == 16; }
MZ_HD inline bool ycbcr_code3_valid(int code) { return code >= 0 && code <= 2; }  // the matrix, the subsampling

// the chroma plane of an H x W frame
MZ_HD inline int ycbcr_hc(int H, int sub) { return sub == YCBCR_420 ? (H + 1) / 2 : H; }
MZ_HD inline int ycbcr_wc(int W, int sub) { return sub == YCBCR_444 ? W : (W + 1) / 2; }

struct YcbcrCoeffs {
    YuvCoeffs k;       // the matrix, and the range at this depth
    double mid, maxc;  // 2^(d - 1), 2^d - 1
    int mid16;         // 16 mid
};
MZ_HD inline YcbcrCoeffs ycbcr_coeffs(int matrix, int range, int depth) {
    YcbcrCoeffs c;
    YuvCoeffs& k = c.k;
    k.kr = matrix == YCBCR_BT2020 ? 0.2627 : matrix == YUV_BT709 ? 0.2126 : 0.299;
    k.kb = matrix == YCBCR_BT2020 ? 0.0593 : matrix == YUV_BT709 ? 0.0722 : 0.114;
    k.kg = (1.0 - k.kr) - k.kb;
    const double s = (double)(1 << (depth - 8));
    c.maxc = (double)((1 << depth) - 1);
    c.mid = (double)(1 << (depth - 1));
    c.mid16 = 16 << (depth - 1);
    k.yoff = range == YUV_FULL ? 0.0 : 16.0 * s;
    k.sy = range == YUV_FULL ? c.maxc : 219.0 * s;
    k.sc = range == YUV_FULL ? c.maxc : 224.0 * s;
    k.inv_sy = 1.0 / k.sy;
    k.inv_sc = 1.0 / k.sc;
    k.a_r = 2.0 * (1.0 - k.kr);
    k.a_b = 2.0 * (1.0 - k.kb);
    k.g_r = -(k.kr * k.a_r) / k.kg;
    k.g_b = -(k.kb * k.a_b) / k.kg;
    k.pb_scale = 0.5 / (1.0 - k.kb);
    k.pr_scale = 0.5 / (1.0 - k.kr);
    return c;
}

// a code of a stored word and back: (word >> shift) & mask, code << shift
struct YcbcrWord { int shift; uint32_t mask; };
MZ_HD inline YcbcrWord ycbcr_word(int depth, int align) {
    return YcbcrWord{align == YCBCR_HIGH && depth > 8 ? 16 - depth : 0, (1u << depth) - 1u};
}
MZ_HD inline int ycbcr_read(const YcbcrWord& w, uint32_t word) { return (int)((word >> w.shift) & w.mask); }
MZ_HD inline uint32_t ycbcr_write(const YcbcrWord& w, uint32_t code) { return code << w.shift; }

// one pixel from its Y code and 16 times its two upsampled chroma values (yuv_to_rgb_pixel of mz_yuv.h with the midpoint of the depth)
MZ_HD inline YuvRgb ycbcr_to_rgb_pixel(const YcbcrCoeffs& c, int ycode, int cb16, int cr16) {
    const YuvCoeffs& k = c.k;
    const double yn = ((double)ycode - k.yoff) * k.inv_sy;
    const double cbn = (double)(cb16 - c.mid16) * (k.inv_sc * 0.0625), crn = (double)(cr16 - c.mid16) * (k.inv_sc * 0.0625);
    return YuvRgb{fma(k.a_r, crn, yn), fma(k.g_b, cbn, fma(k.g_r, crn, yn)), fma(k.a_b, cbn, yn)};
}
// a code value 0..2^d - 1 of scale * v + off: the clamp (a NaN becomes 0), + 0.5, the truncation
MZ_HD inline uint32_t ycbcr_code(double scale, double v, double off, double maxc) {
    const double c = fmin(fmax(fma(scale, v, off), 0.0), maxc);
    return (uint32_t)(c + 0.5);
}

struct YcbcrArgs {
    StridedView y, cb, cr;  // [B,1,H,W], [B,1,Hc,Wc] twice, uint8 (depth 8) or uint16 (s[1] is never used)
    StridedView rgb;        // [B,3,H,W] of `elem`: the output of launch_ycbcr_to_rgb, the input of launch_rgb_to_ycbcr
    int elem;               // Elem 0..3 of rgb
    int B, H, W;
    int depth, align, subsampling;
    int matrix, range, siting;
    int clamp;              // YCbCr -> RGB only
};
// hipError_t values (kept as int: this header stays free of HIP types); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch
int launch_ycbcr_to_rgb(const YcbcrArgs& a, void* hip_stream);
int launch_rgb_to_ycbcr(const YcbcrArgs& a, void* hip_stream);

// chroma_mode of mz_yuv.h for samples of `bytes` bytes: planar, column stride 1 and rows aligned to 8 samples (one 8- or 16-byte access);
// interleaved, column stride 2 with the other plane one ELEMENT ahead or behind and the pairs' rows aligned to 16 bytes (8 pairs are one
// 16-byte access of bytes, two of 16-bit samples)
inline int ycbcr_chroma_mode(const StridedView& cb, const StridedView& cr, int B, int Hc, int bytes) {
    StridedView a = cb, b = cr;
    a.s[1] = b.s[1] = 0;
    if (a.s[3] == 1 && b.s[3] == 1) return rows_aligned(a, B, Hc, bytes, 8 * bytes) && rows_aligned(b, B, Hc, bytes, 8 * bytes) ? CHROMA_PLANAR : CHROMA_ELEMENTS;
    if (a.s[3] != 2 || b.s[3] != 2 || a.s[0] != b.s[0] || a.s[2] != b.s[2]) return CHROMA_ELEMENTS;
    const intptr_t d = (intptr_t)b.data - (intptr_t)a.data;
    if (d == bytes) return rows_aligned(a, B, Hc, bytes, 16) ? CHROMA_PAIRS_CB_FIRST : CHROMA_ELEMENTS;
    if (d == -bytes) return rows_aligned(b, B, Hc, bytes, 16) ? CHROMA_PAIRS_CR_FIRST : CHROMA_ELEMENTS;
    return CHROMA_ELEMENTS;
}

}  // namespace mz
