// Images with an alpha channel (mz_alpha_fill(), mz_alpha_merge(): include/mewzoom_hip.h): the colour of a straight-alpha image
// extrapolated over its transparent region by a push-pull pyramid, so that the model's receptive field meets no arbitrary colour
// under a == 0, and the alpha plane enlarged with the bits of the model's own skip (mz_interp.h).  No reference counterpart: the
// reference's decode_image(mode="RGB") drops alpha.
//
// THE ARITHMETIC, stated here once (the kernels of mz_alpha.hip and the host's plan compile this source; tests/alpha_ref.py restates
// it in Python).  Float64 with contraction off; every fma below is one; each STORED component is rounded once to float32.
//   alpha    a = the element by the view's rule (uint8: v / 255, a true division), clamped to [0, 1] by fmin(fmax(.)): a NaN reads as 0
//   colour   c = the element's value (straight input);  premultiplied input p:  c = a > 0 ? clamp(p / a, 0, 1) : 0, a true division
//   pyramid  level 0 is H x W, level l + 1 is ceil(H_l / 2) x ceil(W_l / 2), down to 1 x 1 (alpha_plan()).  A texel is four float32
//            (w, r, g, b) in one 16-byte word
//   level 0  (a, a c_r, a c_g, a c_b) where a > 0; exactly (0, 0, 0, 0) where a == 0, by a SELECT and never by a product: the colour
//            elements under a == 0 are never used arithmetically (alpha_texel0())
//   push     texel (y, x) of level l + 1 sums the children (2y + dy, 2x + dx) that exist in the order (0,0), (0,1), (1,0), (1,1), plain
//            adds from 0 per component; if the summed w > 1 every component is divided by it (a true division) and w = 1 (alpha_push())
//   pull     from the coarsest level down; the coarsest stays as pushed.  A texel (y, x) of level l gets U, the bilinear 2x enlargement
//            of the already pulled level l + 1: parent py = y >> 1, neighbour ny = clamp(py + ((y & 1) ? 1 : -1), 0, H_{l+1} - 1), the
//            same in x;  U = the fma chain from 0 over (py,px) 9/16, (py,nx) 3/16, (ny,px) 3/16, (ny,nx) 1/16 per component (alpha_up());
//            texel' = fma(1 - w, U, texel) per component, w included (alpha_pull())
//   result   straight input, a > 0: the input's three elements moved as bit patterns;  premultiplied input, a > 0: c rounded once by the
//            view's store rule;  a == 0:  w0' > 0 ? clamp(rgb0' / w0', 0, 1) : 0, rounded once by the store rule (the 16-bit types through
//            round-to-odd, as st_f64 of mz_view.h).  The level-0 texel' of such a pixel is fma(1, U, 0) = U in float64: it is formed in
//            registers and never rounded to float32.  An image of one pixel has no level 1: its texel' is the level-0 texel itself
//   merge    out alpha = interp_taps / interp_dot of mz_interp.h on the low-resolution alpha plane (nearest, bilinear, bicubic), clamped
//            to [0, 1], rounded once: the bits of mz_interpolate(clamp = 1) on that plane.  With premultiply, rgb_out = c A in float64,
//            rounded once (uint8 by its clamping rule), where A is the value of the alpha element AS STORED: the stored pair is consistent
//
// WHAT IS MATERIALISED.  Level 0 is never written: its texels are consumed once, by the push to level 1, which forms them from the views
// (alpha_push0_kernel), and the pull of level 0 is fused with the store of the result (alpha_pull0_kernel), where only the pixels with
// a == 0 need U.  The workspace holds levels 1 .. n - 1, [B][H_l][W_l] texels each, level 1 first (16 bytes at least: a workspace is
// never empty).  One launch per level and direction covers all B images; no atomics; 64-bit signed addressing.
//
// The host part needs no HIP header: plain g++ compiles it.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>  // (mz_view.h's device part needs it first)
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mz_interp.h"
#include "mz_view.h"

namespace mz {

constexpr int kAlphaThreads = 256;
static_assert(kAlphaThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kAlphaMaxLevels = 32;  // sides of 2^28 have 29
constexpr int kAlphaTileH = 32, kAlphaTileW = 128;  // output pixels of one alpha_merge_kernel workgroup (the tile of mz_interp.h)

// ---- the pyramid ------------------------------------------------------------------------------------------------------------------------
struct AlphaPlan {
    int n;                              // levels, level 0 included
    int h[kAlphaMaxLevels], w[kAlphaMaxLevels];
    size_t off[kAlphaMaxLevels];        // byte offset of level l >= 1 in the workspace (off[0] is unused: level 0 is not materialised)
    size_t total;
};
// false where H or W is outside [1, 2^28], B < 1, or the levels would pass 2^62 bytes
inline bool alpha_plan(int B, int H, int W, AlphaPlan* p) {
    if (B < 1 || H < 1 || W < 1 || H > (1 << 28) || W > (1 << 28)) return false;
    p->n = 0;
    unsigned __int128 total = 0;
    for (int h = H, w = W;; h = (h + 1) / 2, w = (w + 1) / 2) {
        const int l = p->n++;
        p->h[l] = h;
        p->w[l] = w;
        p->off[l] = (size_t)total;
        if (l > 0) total += (unsigned __int128)B * (unsigned long long)h * (unsigned long long)w * 16u;
        if (total > ((unsigned __int128)1 << 62)) return false;
        if (h == 1 && w == 1) break;
    }
    p->total = total < 16 ? 16 : (size_t)total;
    return true;
}

// ---- texels -----------------------------------------------------------------------------------------------------------------------------
struct AlphaTexel { double w, r, g, b; };  // (in memory: four float32)

MZ_HD inline double alpha_clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }  // a NaN becomes 0
MZ_HD inline double alpha_f32(double v) { return (double)(float)v; }             // the one rounding of a stored component

// the straight colour of one element: e the element's value, a the clamped alpha (> 0 where this is used arithmetically)
MZ_HD inline double alpha_straight(double e, double a, int premultiplied) {
#pragma clang fp contract(off)
    if (!premultiplied) return e;
    return a > 0.0 ? alpha_clamp01(e / a) : 0.0;
}
// the level-0 texel of a pixel: a already clamped, (r, g, b) the straight colour
MZ_HD inline AlphaTexel alpha_texel0(double a, double r, double g, double b) {
#pragma clang fp contract(off)
    const bool on = a > 0.0;
    return AlphaTexel{on ? alpha_f32(a) : 0.0, on ? alpha_f32(a * r) : 0.0, on ? alpha_f32(a * g) : 0.0, on ? alpha_f32(a * b) : 0.0};
}
// push: the four children in order, each already a stored texel; a child that does not exist is passed as the zero texel, which changes
// no bit of the sums (they start at +0 and never reach -0)
MZ_HD inline AlphaTexel alpha_push(const AlphaTexel& c00, const AlphaTexel& c01, const AlphaTexel& c10, const AlphaTexel& c11) {
#pragma clang fp contract(off)
    double w = 0.0, r = 0.0, g = 0.0, b = 0.0;
    w = w + c00.w; r = r + c00.r; g = g + c00.g; b = b + c00.b;
    w = w + c01.w; r = r + c01.r; g = g + c01.g; b = b + c01.b;
    w = w + c10.w; r = r + c10.r; g = g + c10.g; b = b + c10.b;
    w = w + c11.w; r = r + c11.r; g = g + c11.g; b = b + c11.b;
    if (w > 1.0) {
        r = r / w;
        g = g / w;
        b = b / w;
        w = 1.0;  // (w / w)
    }
    return AlphaTexel{alpha_f32(w), alpha_f32(r), alpha_f32(g), alpha_f32(b)};
}
// the neighbour of parent p = i >> 1 that texel i of the finer level leans to, n the coarser level's size
MZ_HD inline int alpha_neighbour(int i, int n) {
    const int p = i >> 1, q = (i & 1) ? p + 1 : p - 1;
    return q < 0 ? 0 : q > n - 1 ? n - 1 : q;
}
// U of the four pulled texels (py,px), (py,nx), (ny,px), (ny,nx): unrounded float64
MZ_HD inline AlphaTexel alpha_up(const AlphaTexel& pp, const AlphaTexel& pn, const AlphaTexel& np, const AlphaTexel& nn) {
    const auto up = [](double a, double b, double c, double d) {
        double acc = 0.0;
        acc = fma(0.5625, a, acc);
        acc = fma(0.1875, b, acc);
        acc = fma(0.1875, c, acc);
        acc = fma(0.0625, d, acc);
        return acc;
    };
    return AlphaTexel{up(pp.w, pn.w, np.w, nn.w), up(pp.r, pn.r, np.r, nn.r), up(pp.g, pn.g, np.g, nn.g), up(pp.b, pn.b, np.b, nn.b)};
}
// pull of a stored texel t of a level >= 1
MZ_HD inline AlphaTexel alpha_pull(const AlphaTexel& t, const AlphaTexel& U) {
#pragma clang fp contract(off)
    const double k = 1.0 - t.w;
    return AlphaTexel{alpha_f32(fma(k, U.w, t.w)), alpha_f32(fma(k, U.r, t.r)), alpha_f32(fma(k, U.g, t.g)), alpha_f32(fma(k, U.b, t.b))};
}
// one component of the result of a pixel with a == 0, before the store rule: w the texel' weight, v the component
MZ_HD inline double alpha_fill_value(double w, double v) {
#pragma clang fp contract(off)
    return w > 0.0 ? alpha_clamp01(v / w) : 0.0;
}
// merge with premultiply: the colour value c and A, the value of the alpha element as stored
MZ_HD inline double alpha_premultiply(double c, double A) {
#pragma clang fp contract(off)
    return c * A;
}

// ---- the launches -----------------------------------------------------------------------------------------------------------------------
struct AlphaFillArgs {
    StridedView rgb, alpha, out;  // [B,3,H,W], [B,1,H,W] (s[1] is never used), [B,3,H,W]
    int elem;                     // Elem 0..3 of all three
    int B, H, W;
    int premultiplied;
    AlphaPlan plan;
    char* ws;
};
struct AlphaMergeArgs {
    StridedView rgb, alpha, out_rgb, out_alpha;  // rgb, out_rgb: [B,3,Hout,Wout], used with premultiply only; the planes: [B,1,..]
    int elem;
    int B, Hin, Win, Hout, Wout;
    int mode;                                    // InterpMode
    int premultiply;
};
// hipError_t values (kept as int: this header stays free of HIP types); hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h)
// can launch -- found before the first launch: a refused call writes nothing
int launch_alpha_fill(const AlphaFillArgs& a, void* hip_stream);
int launch_alpha_merge(const AlphaMergeArgs& a, void* hip_stream);

}  // namespace mz
