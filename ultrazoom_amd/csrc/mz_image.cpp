// Stateless image entry points of libmewzoom_hip.so: image-quality metrics (RGB and luma), the luma plane, YCbCr frames (8-bit 4:2:0; any depth and subsampling), antialiased resizing, plain
// interpolation, the degradation chain, the dihedral transforms with the self-ensemble accumulator, images with alpha, the paste of feathered tiling, and the
// host-only mz_debug_* views of what their kernels are handed.  Every check comes before anything touches the GPU.
#include <cstring>

#include "mz_alpha.h"
#include "mz_color.h"
#include "mz_degrade.h"
#include "mz_dihedral.h"
#include "mz_err.h"
#include "mz_feather.h"
#include "mz_interp.h"
#include "mz_metrics.h"
#include "mz_resize.h"
#include "mz_ycbcr.h"
#include "mz_yuv.h"

using namespace mz;

// the tail of every entry here: the device made ready, the launch, its error under the entry's name
template <class Launch> static int launched(const char* what, Launch launch) {
    if (int rc = device_cus(); rc < 0) return rc;
    return hip_rc(launch(), what);
}

// the two byte ranges of a call, each from its own shape (mz_interpolate, mz_dihedral, the ensemble entries; mz_luma: b has Cb = 1 channel)
static int check_ranges_apart(const mz_image_view* a, int elem_a, int Ha, int Wa, const mz_image_view* b, int elem_b, int Hb, int Wb, int B,
                              const char* what, int Cb = 3) {
    long long al, ah, bl, bh;
    if (!view_extent(a, elem_a, B, Ha, Wa, &al, &ah) || !view_extent(b, elem_b, B, Hb, Wb, &bl, &bh, Cb))
        return fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
    if (al < bh && bl < ah) return fail(MZ_ERR_INVALID_ARGUMENT, "%s overlap: this entry does not work in place", what);
    return MZ_OK;
}

// the four sizes of a resampling call (mz_resize, mz_interpolate and their mz_debug_*_taps: behind each entry's filter / mode check)
static int check_sizes(int Hin, int Win, int Hout, int Wout) {
    if (Hin < 1 || Win < 1 || Hout < 1 || Wout < 1)
        return fail(MZ_ERR_INVALID_ARGUMENT, "need sizes >= 1 (got %d x %d -> %d x %d)", Hin, Win, Hout, Wout);
    if (Hin > (1 << 28) || Win > (1 << 28) || Hout > (1 << 28) || Wout > (1 << 28))
        return fail(MZ_ERR_INVALID_ARGUMENT, "at most 2^28 pixels a side (got %d x %d -> %d x %d)", Hin, Win, Hout, Wout);
    return MZ_OK;
}

// the batch of a workspace query that has no views to check (mz_jpeg_workspace_bytes, mz_ensemble_workspace_bytes)
static int check_batch_bounds(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 28) || W > (1 << 28))
        return fail(MZ_ERR_INVALID_ARGUMENT, "need 1 <= B <= 65535 and 1 <= H, W <= 2^28 (got %d, %d, %d)", B, H, W);
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// image-quality metrics (mz_metrics.h): no reference counterpart in model.py; stands in for torchmetrics as the reference's
// pretrain.py:209-211, 301-329 uses it.  Stateless like the mz_op_* entries.
// ------------------------------------------------------------------------------------------------
static int check_metrics_shape(int B, int H, int W, int which) {
    if (which <= 0 || (which & ~(MET_PSNR | MET_SSIM | MET_VIF)))
        return fail(MZ_ERR_INVALID_ARGUMENT, "which must be a non-empty combination of 1 (PSNR), 2 (SSIM), 4 (VIF), got %d", which);
    if (B < 1 || H < 1 || W < 1) return fail(MZ_ERR_INVALID_ARGUMENT, "need B, H, W >= 1 (got %d, %d, %d)", B, H, W);
    if (B > 65535 || H > (1 << 28) || W > (1 << 28))
        return fail(MZ_ERR_INVALID_ARGUMENT, "at most 65535 images of at most 2^28 pixels a side (got %d, %d, %d)", B, H, W);
    if ((which & MET_SSIM) && (H < 11 || W < 11))
        return fail(MZ_ERR_INVALID_ARGUMENT, "SSIM needs images of at least 11 x 11 pixels, got %d x %d", H, W);
    if ((which & MET_VIF) && (H < 41 || W < 41))
        return fail(MZ_ERR_INVALID_ARGUMENT, "VIF needs images of at least 41 x 41 pixels, got %d x %d", H, W);
    return MZ_OK;
}

extern "C" int mz_metrics_workspace_bytes(int B, int H, int W, int which, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_metrics_shape(B, H, W, which)) return rc;
    *bytes = metrics_plan(B, H, W, which).total;
    return MZ_OK;
}

extern "C" int mz_metrics(const mz_image_view* pred, const mz_image_view* target, int elem, int B, int H, int W, int which,
                          double data_range, double sigma_n_sq, double* out_dev, void* workspace, size_t workspace_bytes,
                          void* hip_stream) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ false, /*batch_bound*/ false, /*side_bound*/ false};
    MetricsArgs a = {};
    if (const Refusal r = check_views(pred, target, rules, elem, B, H, W, &a.pred, &a.target)) return fail(r);
    if (int rc = check_metrics_shape(B, H, W, which)) return rc;
    if (!out_dev) return fail(MZ_ERR_INVALID_ARGUMENT, "null out_dev");
    a.plan = metrics_plan(B, H, W, which);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, a.plan.total)) return fail(r);
    a.elem = elem; a.B = B; a.H = H; a.W = W;
    a.which = which;
    a.data_range = data_range;
    a.sigma_n_sq = sigma_n_sq;
    a.out = out_dev;
    a.ws = (char*)workspace;
    return launched("metrics launch", [&] { return launch_metrics(a, (hipStream_t)hip_stream); });
}

// ------------------------------------------------------------------------------------------------
// luma (mz_color.h): the Y plane of an RGB view, and the metrics of the Y planes of two views.  No reference counterpart: the reference's
// validate.py measures RGB over the full frame.  Stateless like mz_metrics.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static int check_standard(int standard) {
    return luma_valid(standard) ? MZ_OK : fail(MZ_ERR_INVALID_ARGUMENT, "standard must be 0 (bt601, studio range) or 1 (full range), got %d", standard);
}

extern "C" int mz_luma(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int standard, int clamp,
                       void* hip_stream) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};
    if (!x || !out) return fail(MZ_ERR_INVALID_ARGUMENT, "null image view");
    mz_image_view y = *out;
    y.stride[1] = 1;  // one channel: its stride is never used, any value is accepted
    LumaArgs a = {};
    if (const Refusal r = check_views(x, &y, rules, elem, B, H, W, &a.x, &a.out)) return fail(r);
    if (int rc = check_standard(standard)) return rc;
    if (int rc = check_ranges_apart(x, elem, H, W, &y, elem, H, W, B, "x and out", 1)) return rc;
    a.elem = elem; a.B = B; a.H = H; a.W = W;
    a.standard = standard;
    a.clamp = clamp != 0;
    return launched("luma launch", [&] { return (hipError_t)launch_luma(a, hip_stream); });
}

// Host only: {off, kr, kg, kb} of a standard, the constants the kernels compile
extern "C" int mz_debug_luma_coeffs(int standard, double out[4]) {
    if (!out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_standard(standard)) return rc;
    const LumaCoeffs k = luma_coeffs(standard);
    out[0] = k.off; out[1] = k.kr; out[2] = k.kg; out[3] = k.kb;
    return MZ_OK;
}

static int check_metrics_luma_shape(int B, int H, int W, int which) {
    if (int rc = check_metrics_shape(B, H, W, which)) return rc;
    if (!luma_planes_fit(B, H, W)) return fail(MZ_ERR_INVALID_ARGUMENT, "two float64 Y planes of %d x %d x %d are beyond 2^62 bytes", B, H, W);
    return MZ_OK;
}

extern "C" int mz_metrics_luma_workspace_bytes(int B, int H, int W, int which, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_metrics_luma_shape(B, H, W, which)) return rc;
    *bytes = metrics_plan(B, H, W, which, 1).total;
    return MZ_OK;
}

extern "C" int mz_metrics_luma(const mz_image_view* pred, const mz_image_view* target, int elem, int B, int H, int W, int which, int standard,
                               double data_range, double sigma_n_sq, double* out_dev, void* workspace, size_t workspace_bytes,
                               void* hip_stream) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ false, /*batch_bound*/ false, /*side_bound*/ false};
    MetricsArgs a = {};
    if (const Refusal r = check_views(pred, target, rules, elem, B, H, W, &a.pred, &a.target)) return fail(r);
    if (int rc = check_metrics_luma_shape(B, H, W, which)) return rc;
    if (int rc = check_standard(standard)) return rc;
    if (!out_dev) return fail(MZ_ERR_INVALID_ARGUMENT, "null out_dev");
    a.plan = metrics_plan(B, H, W, which, 1);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, a.plan.total)) return fail(r);
    a.elem = elem; a.B = B; a.H = H; a.W = W;
    a.standard = standard;
    a.which = which;
    a.data_range = data_range;
    a.sigma_n_sq = sigma_n_sq;
    a.out = out_dev;
    a.ws = (char*)workspace;
    return launched("luma metrics launch", [&] { return launch_metrics_luma(a, (hipStream_t)hip_stream); });
}

// ------------------------------------------------------------------------------------------------
// 8-bit 4:2:0 YCbCr frames (mz_yuv.h): Y, Cb and Cr planes to an RGB view and back.  No reference counterpart.  Stateless like mz_luma,
// no workspace.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
struct YuvPlanes { mz_image_view y, cb, cr; };  // the three views with a channel stride of 1: one channel, its stride names nothing

// the three codes: the LAST check of both entries (a call that arrives here with a bad code has passed every check of its views --
// how tests/test_yuv_cpu.py shows on a machine with a GPU that a layout is accepted, without a launch)
static int check_yuv_codes(int matrix, int range, int siting) {
    if (!yuv_code_valid(matrix)) return fail(MZ_ERR_INVALID_ARGUMENT, "matrix must be 0 (bt601) or 1 (bt709), got %d", matrix);
    if (!yuv_code_valid(range)) return fail(MZ_ERR_INVALID_ARGUMENT, "range must be 0 (limited) or 1 (full), got %d", range);
    if (!yuv_code_valid(siting)) return fail(MZ_ERR_INVALID_ARGUMENT, "siting must be 0 (left) or 1 (center), got %d", siting);
    return MZ_OK;
}

// the views and shapes of both entries; `planes_written`: the planes are the outputs (no stride of 0), else the RGB view is
static int check_yuv_call(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, const mz_image_view* rgb, int elem, int B, int H,
                          int W, int matrix, int range, int siting, bool planes_written, YuvPlanes* p, YuvArgs* a) {
    static const ViewRules written = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};
    static const ViewRules read = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ false, /*batch_bound*/ true, /*side_bound*/ true};
    if (!y || !cb || !cr || !rgb) return fail(MZ_ERR_INVALID_ARGUMENT, "null image view");
    p->y = *y; p->cb = *cb; p->cr = *cr;
    p->y.stride[1] = p->cb.stride[1] = p->cr.stride[1] = 1;
    StridedView unused;
    if (const Refusal r = check_views(planes_written ? rgb : &p->y, planes_written ? &p->y : rgb, written, elem, B, H, W,
                                      planes_written ? &a->rgb : &a->y, planes_written ? &a->y : &a->rgb)) return fail(r);
    const ViewRules& chroma = planes_written ? written : read;
    if (const Refusal r = check_views(&p->cb, &p->cb, chroma, elem, B, H, W, &unused, &a->cb)) return fail(r);
    if (const Refusal r = check_views(&p->cr, &p->cr, chroma, elem, B, H, W, &unused, &a->cr)) return fail(r);
    // the RGB view against each plane: inputs and outputs lie apart
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const mz_image_view* plane[3] = {&p->y, &p->cb, &p->cr};
    for (int i = 0; i < 3; ++i) {
        long long rl, rh, pl, ph;
        if (!view_extent(rgb, elem, B, H, W, &rl, &rh) || !view_extent(plane[i], EL_U8, B, i ? Hc : H, i ? Wc : W, &pl, &ph, 1))
            return fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
        if (rl < ph && pl < rh) return fail(MZ_ERR_INVALID_ARGUMENT, "the RGB view and the %s plane overlap: this entry does not work in place", i == 0 ? "Y" : i == 1 ? "Cb" : "Cr");
    }
    a->elem = elem; a->B = B; a->H = H; a->W = W;
    a->matrix = matrix; a->range = range; a->siting = siting;
    return MZ_OK;
}

// Two planes that are WRITTEN share no byte: the byte range of every image of one against every image of the other.  (The ranges of whole
// batches would not do: the planes of an NV12 or I420 batch alternate in memory.)  With equal image strides image b of one meets image
// b' of the other exactly when the ranges of their images 0, (b - b') image strides apart, do; with different ones the batches' ranges decide.
// (`elem`: a code whose element has the planes' size -- EL_U8, or EL_F16 for 16-bit samples)
static bool planes_apart(const mz_image_view* p, int Hp, int Wp, const mz_image_view* q, int Hq, int Wq, int B, bool* fits, int elem = EL_U8) {
    long long pl, ph, ql, qh;
    *fits = true;
    if (B > 1 && p->stride[0] != q->stride[0]) {
        *fits = view_extent(p, elem, B, Hp, Wp, &pl, &ph, 1) && view_extent(q, elem, B, Hq, Wq, &ql, &qh, 1);
        return *fits && !(pl < qh && ql < ph);
    }
    *fits = view_extent(p, elem, 1, Hp, Wp, &pl, &ph, 1) && view_extent(q, elem, 1, Hq, Wq, &ql, &qh, 1);
    if (!*fits) return false;
    for (long long d = -(long long)(B - 1); d <= B - 1; ++d) {  // (B <= 65535)
        const __int128 shift = (__int128)d * p->stride[0] * (elem == EL_U8 ? 1 : 2);
        if (pl + shift < qh && ql < ph + shift) return false;
    }
    return true;
}

// Cb and Cr interleave, as in NV12: identical strides, a column stride of at least 2, bases a whole number of elements (of `bytes`
// bytes), 1 .. column stride - 1, apart
static bool chroma_interleaved(const mz_image_view* cb, const mz_image_view* cr, int bytes = 1) {
    for (int i = 0; i < 4; ++i)
        if (cb->stride[i] != cr->stride[i]) return false;
    const long long s = cb->stride[3], db = (long long)((intptr_t)cr->data - (intptr_t)cb->data), d = db / bytes;
    return s >= 2 && db % bytes == 0 && d != 0 && d > -s && d < s;
}

extern "C" int mz_yuv420_to_rgb(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, const mz_image_view* out, int elem_out,
                                int B, int H, int W, int matrix, int range, int siting, int clamp, void* hip_stream) {
    YuvPlanes p;
    YuvArgs a = {};
    if (int rc = check_yuv_call(y, cb, cr, out, elem_out, B, H, W, matrix, range, siting, false, &p, &a)) return rc;
    if (int rc = check_yuv_codes(matrix, range, siting)) return rc;
    a.clamp = clamp != 0;
    return launched("yuv420_to_rgb launch", [&] { return (hipError_t)launch_yuv420_to_rgb(a, hip_stream); });
}

extern "C" int mz_rgb_to_yuv420(const mz_image_view* x, int elem, const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr,
                                int B, int H, int W, int matrix, int range, int siting, void* hip_stream) {
    YuvPlanes p;
    YuvArgs a = {};
    if (int rc = check_yuv_call(y, cb, cr, x, elem, B, H, W, matrix, range, siting, true, &p, &a)) return rc;
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    bool fits;
    if (!planes_apart(&p.y, H, W, &p.cb, Hc, Wc, B, &fits) || !planes_apart(&p.y, H, W, &p.cr, Hc, Wc, B, &fits))
        return fits ? fail(MZ_ERR_INVALID_ARGUMENT, "the Y plane and a chroma plane overlap") : fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
    if (!chroma_interleaved(&p.cb, &p.cr) && !planes_apart(&p.cb, Hc, Wc, &p.cr, Hc, Wc, B, &fits))
        return fits ? fail(MZ_ERR_INVALID_ARGUMENT, "the Cb and Cr planes overlap without interleaving (identical strides, a column stride of "
                                                     "at least 2, bases less than that apart)")
                    : fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
    if (int rc = check_yuv_codes(matrix, range, siting)) return rc;
    return launched("rgb_to_yuv420 launch", [&] { return (hipError_t)launch_rgb_to_yuv420(a, hip_stream); });
}

// Host only: {Yoff, 1/Sy, 1/Sc, a_r, a_b, g_r, g_b, Sy, Sc} of a matrix and a range, the constants the kernels compile
extern "C" int mz_debug_yuv_coeffs(int matrix, int range, double out[9]) {
    if (!out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (!yuv_code_valid(matrix) || !yuv_code_valid(range)) return fail(MZ_ERR_INVALID_ARGUMENT, "matrix and range must be 0 or 1, got %d and %d", matrix, range);
    const YuvCoeffs k = yuv_coeffs(matrix, range);
    out[0] = k.yoff; out[1] = k.inv_sy; out[2] = k.inv_sc; out[3] = k.a_r; out[4] = k.a_b; out[5] = k.g_r; out[6] = k.g_b; out[7] = k.sy; out[8] = k.sc;
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// YCbCr frames of 8, 10, 12 or 16 bits in 4:2:0, 4:2:2 or 4:4:4 (mz_ycbcr.h): the entries above generalised over depth, alignment,
// subsampling and a third matrix.  The same checks in the same order, byte ranges with the planes' element size.
// ------------------------------------------------------------------------------------------------
// what decides the planes' shapes and element size: checked once the views are known not to be null, before their ranges are formed
static int check_ycbcr_format(int depth, int align, int subsampling) {
    if (!ycbcr_depth_valid(depth)) return fail(MZ_ERR_INVALID_ARGUMENT, "depth must be 8, 10, 12 or 16, got %d", depth);
    if (align != YCBCR_LOW && align != YCBCR_HIGH) return fail(MZ_ERR_INVALID_ARGUMENT, "align must be 0 (low) or 1 (high), got %d", align);
    if (!ycbcr_code3_valid(subsampling)) return fail(MZ_ERR_INVALID_ARGUMENT, "subsampling must be 0 (420), 1 (422) or 2 (444), got %d", subsampling);
    return MZ_OK;
}
// the LAST check of both entries, as check_yuv_codes
static int check_ycbcr_codes(int matrix, int range, int siting) {
    if (!ycbcr_code3_valid(matrix)) return fail(MZ_ERR_INVALID_ARGUMENT, "matrix must be 0 (bt601), 1 (bt709) or 2 (bt2020), got %d", matrix);
    if (!yuv_code_valid(range)) return fail(MZ_ERR_INVALID_ARGUMENT, "range must be 0 (limited) or 1 (full), got %d", range);
    if (!yuv_code_valid(siting)) return fail(MZ_ERR_INVALID_ARGUMENT, "siting must be 0 (left) or 1 (center), got %d", siting);
    return MZ_OK;
}

// check_yuv_call with the format: `plane_elem` is a code whose element has the planes' size
static int check_ycbcr_call(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, const mz_image_view* rgb, int elem, int B, int H,
                            int W, int depth, int align, int subsampling, bool planes_written, YuvPlanes* p, YcbcrArgs* a, int* plane_elem) {
    static const ViewRules written = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};
    static const ViewRules read = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ false, /*batch_bound*/ true, /*side_bound*/ true};
    if (!y || !cb || !cr || !rgb) return fail(MZ_ERR_INVALID_ARGUMENT, "null image view");
    if (int rc = check_ycbcr_format(depth, align, subsampling)) return rc;
    *plane_elem = depth > 8 ? EL_F16 : EL_U8;  // (view_extent takes an element code: a 16-bit sample has the size of a 16-bit element)
    p->y = *y; p->cb = *cb; p->cr = *cr;
    p->y.stride[1] = p->cb.stride[1] = p->cr.stride[1] = 1;
    StridedView unused;
    if (const Refusal r = check_views(planes_written ? rgb : &p->y, planes_written ? &p->y : rgb, written, elem, B, H, W,
                                      planes_written ? &a->rgb : &a->y, planes_written ? &a->y : &a->rgb)) return fail(r);
    const ViewRules& chroma = planes_written ? written : read;
    if (const Refusal r = check_views(&p->cb, &p->cb, chroma, elem, B, H, W, &unused, &a->cb)) return fail(r);
    if (const Refusal r = check_views(&p->cr, &p->cr, chroma, elem, B, H, W, &unused, &a->cr)) return fail(r);
    const int Hc = ycbcr_hc(H, subsampling), Wc = ycbcr_wc(W, subsampling);
    const mz_image_view* plane[3] = {&p->y, &p->cb, &p->cr};
    static const char* const names[3] = {"Y", "Cb", "Cr"};
    if (depth > 8)
        for (int i = 0; i < 3; ++i)
            if ((uintptr_t)plane[i]->data % 2) return fail(MZ_ERR_INVALID_ARGUMENT, "the %s plane's data is not aligned to 2 bytes (depth %d: uint16 samples)", names[i], depth);
    for (int i = 0; i < 3; ++i) {  // the RGB view against each plane: inputs and outputs lie apart
        long long rl, rh, pl, ph;
        if (!view_extent(rgb, elem, B, H, W, &rl, &rh) || !view_extent(plane[i], *plane_elem, B, i ? Hc : H, i ? Wc : W, &pl, &ph, 1))
            return fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
        if (rl < ph && pl < rh) return fail(MZ_ERR_INVALID_ARGUMENT, "the RGB view and the %s plane overlap: this entry does not work in place", names[i]);
    }
    a->elem = elem; a->B = B; a->H = H; a->W = W;
    a->depth = depth; a->align = align; a->subsampling = subsampling;
    return MZ_OK;
}

extern "C" int mz_ycbcr_to_rgb(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, int depth, int align, int subsampling,
                               const mz_image_view* out, int elem_out, int B, int H, int W, int matrix, int range, int siting, int clamp,
                               void* hip_stream) {
    YuvPlanes p;
    YcbcrArgs a = {};
    int plane_elem;
    if (int rc = check_ycbcr_call(y, cb, cr, out, elem_out, B, H, W, depth, align, subsampling, false, &p, &a, &plane_elem)) return rc;
    if (int rc = check_ycbcr_codes(matrix, range, siting)) return rc;
    a.matrix = matrix; a.range = range; a.siting = siting;
    a.clamp = clamp != 0;
    return launched("ycbcr_to_rgb launch", [&] { return (hipError_t)launch_ycbcr_to_rgb(a, hip_stream); });
}

extern "C" int mz_rgb_to_ycbcr(const mz_image_view* x, int elem, const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr,
                               int depth, int align, int subsampling, int B, int H, int W, int matrix, int range, int siting, void* hip_stream) {
    YuvPlanes p;
    YcbcrArgs a = {};
    int pe;
    if (int rc = check_ycbcr_call(y, cb, cr, x, elem, B, H, W, depth, align, subsampling, true, &p, &a, &pe)) return rc;
    const int Hc = ycbcr_hc(H, subsampling), Wc = ycbcr_wc(W, subsampling);
    bool fits;
    if (!planes_apart(&p.y, H, W, &p.cb, Hc, Wc, B, &fits, pe) || !planes_apart(&p.y, H, W, &p.cr, Hc, Wc, B, &fits, pe))
        return fits ? fail(MZ_ERR_INVALID_ARGUMENT, "the Y plane and a chroma plane overlap") : fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
    if (!chroma_interleaved(&p.cb, &p.cr, depth > 8 ? 2 : 1) && !planes_apart(&p.cb, Hc, Wc, &p.cr, Hc, Wc, B, &fits, pe))
        return fits ? fail(MZ_ERR_INVALID_ARGUMENT, "the Cb and Cr planes overlap without interleaving (identical strides, a column stride of "
                                                     "at least 2 elements, bases at least one element and less than that apart)")
                    : fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
    if (int rc = check_ycbcr_codes(matrix, range, siting)) return rc;
    a.matrix = matrix; a.range = range; a.siting = siting;
    return launched("rgb_to_ycbcr launch", [&] { return (hipError_t)launch_rgb_to_ycbcr(a, hip_stream); });
}

// Host only: the nine values of mz_debug_yuv_coeffs at a depth, then the chroma midpoint and the largest code
extern "C" int mz_debug_ycbcr_coeffs(int matrix, int range, int depth, double out[11]) {
    if (!out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (!ycbcr_code3_valid(matrix) || !yuv_code_valid(range) || !ycbcr_depth_valid(depth))
        return fail(MZ_ERR_INVALID_ARGUMENT, "matrix must be 0..2, range 0 or 1, depth 8, 10, 12 or 16, got %d, %d and %d", matrix, range, depth);
    const YcbcrCoeffs c = ycbcr_coeffs(matrix, range, depth);
    const YuvCoeffs& k = c.k;
    out[0] = k.yoff; out[1] = k.inv_sy; out[2] = k.inv_sc; out[3] = k.a_r; out[4] = k.a_b; out[5] = k.g_r; out[6] = k.g_b; out[7] = k.sy; out[8] = k.sc;
    out[9] = c.mid; out[10] = c.maxc;
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// antialiased resampling to any size (mz_resize.h): no reference counterpart in model.py; stands in for torchvision's Resize as the
// reference's data.py:91-108 uses it.  Stateless like mz_metrics.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static int check_resize_shape(int Hin, int Win, int Hout, int Wout, int filter) {
    if (filter != RF_BICUBIC && filter != RF_BILINEAR)
        return fail(MZ_ERR_INVALID_ARGUMENT, "filter must be 0 (bicubic) or 1 (bilinear), got %d", filter);
    if (int rc = check_sizes(Hin, Win, Hout, Wout)) return rc;
    if ((long long)Hin > (long long)kResizeMaxRatio * Hout || (long long)Win > (long long)kResizeMaxRatio * Wout)
        return fail(MZ_ERR_INVALID_ARGUMENT, "%d x %d -> %d x %d shrinks an axis by more than %d", Hin, Win, Hout, Wout, kResizeMaxRatio);
    return MZ_OK;
}

extern "C" int mz_resize_workspace_bytes(int Hin, int Win, int Hout, int Wout, int filter, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_resize_shape(Hin, Win, Hout, Wout, filter)) return rc;
    *bytes = resize_plan(Hin, Win, Hout, Wout, filter).total;
    return MZ_OK;
}

extern "C" int mz_resize(const mz_image_view* x, const mz_image_view* out, int elem, int B, int Hin, int Win, int Hout, int Wout, int filter,
                         int clamp, const int32_t window[4], void* workspace, size_t workspace_bytes, void* hip_stream) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ false};
    ResizeArgs a = {};
    if (const Refusal r = check_views(x, out, rules, elem, B, Hout, Wout, &a.x, &a.out)) return fail(r);
    if (int rc = check_resize_shape(Hin, Win, Hout, Wout, filter)) return rc;
    if (const Refusal r = check_window(window, Hout, Wout, &a.y0, &a.x0, &a.h, &a.w)) return fail(r);
    a.plan = resize_plan(Hin, Win, Hout, Wout, filter);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, a.plan.total)) return fail(r);
    a.elem = elem;
    a.B = B;
    a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout;
    a.filter = filter;
    a.clamp = clamp != 0;
    a.ws = (char*)workspace;
    return launched("resize launch", [&] { return launch_resize(a, (hipStream_t)hip_stream); });
}

// Host only: resize_taps() (mz_resize.h) of one output index, the source the device's table kernel compiles too
extern "C" int mz_debug_resize_taps(int n_in, int n_out, int filter, int i, int* first, double* w, int cap) {
    if (!first || !w || cap < 0) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument or negative cap");
    if (int rc = check_resize_shape(n_in, 1, n_out, 1, filter)) return rc;
    if (i < 0 || i >= n_out) return fail(MZ_ERR_INVALID_ARGUMENT, "output index %d is not in [0, %d)", i, n_out);
    const int count = resize_taps(n_in, n_out, filter, i, first, cap, [&](int j, double v) { w[j] = v; });
    if (count > cap) return fail(MZ_ERR_INVALID_ARGUMENT, "output %d has %d taps, room for %d", i, count, cap);
    return count;
}

// ------------------------------------------------------------------------------------------------
// plain interpolation to any size (mz_interp.h): the model's own skip (model.py:71, 156) and the bicubic baseline of the reference's
// validate.py:84-118.  Stateless like mz_resize, no workspace.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static int check_interp_shape(int n_in_h, int n_in_w, int n_out_h, int n_out_w, int mode) {
    if (mode != IM_NEAREST && mode != IM_BILINEAR && mode != IM_BICUBIC)
        return fail(MZ_ERR_INVALID_ARGUMENT, "mode must be 0 (nearest), 1 (bilinear) or 2 (bicubic), got %d", mode);
    return check_sizes(n_in_h, n_in_w, n_out_h, n_out_w);
}

extern "C" int mz_interpolate(const mz_image_view* x, const mz_image_view* out, int elem, int B, int Hin, int Win, int Hout, int Wout, int mode,
                              int clamp, const int32_t window[4], void* hip_stream) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ false};
    InterpArgs a = {};
    if (const Refusal r = check_views(x, out, rules, elem, B, Hout, Wout, &a.x, &a.out)) return fail(r);
    if (int rc = check_interp_shape(Hin, Win, Hout, Wout, mode)) return rc;
    if (const Refusal r = check_window(window, Hout, Wout, &a.y0, &a.x0, &a.h, &a.w)) return fail(r);
    if (int rc = check_ranges_apart(x, elem, Hin, Win, out, elem, a.h, a.w, B, "x and out")) return rc;
    if (mode == IM_NEAREST && clamp != 0)  // (the last check: nearest moves bit patterns, a clamp would change them)
        return fail(MZ_ERR_INVALID_ARGUMENT, "clamp with mode 0 (nearest): nearest moves elements and never changes them");
    a.elem = elem;
    a.B = B;
    a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout;
    a.mode = mode;
    a.clamp = clamp != 0;
    return launched("interpolate launch", [&] { return (hipError_t)launch_interp(a, hip_stream); });
}

// Host only: interp_taps() (mz_interp.h) of one output index, the source the kernels compile too
extern "C" int mz_debug_interp_taps(int n_in, int n_out, int mode, int i, int idx[4], double w[4]) {
    if (!idx || !w) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_interp_shape(n_in, 1, n_out, 1, mode)) return rc;
    if (i < 0 || i >= n_out) return fail(MZ_ERR_INVALID_ARGUMENT, "output index %d is not in [0, %d)", i, n_out);
    return interp_taps(n_in, n_out, mode, i, idx, w);
}

// ------------------------------------------------------------------------------------------------
// the degradation chain (mz_degrade.h): no reference counterpart in model.py; stands in for torchvision's gaussian_blur, gaussian_noise
// and jpeg as the reference's transforms.py uses them.  Stateless like mz_resize.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static int check_degrade_views(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int in_place_ok, DegradeArgs* a) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};
    if (const Refusal r = check_views(x, out, rules, elem, B, H, W, &a->x, &a->out)) return fail(r);
    if (const Refusal r = check_overlap(x, out, elem, B, H, W, in_place_ok != 0)) return fail(r);
    a->elem = elem; a->B = B; a->H = H; a->W = W;
    return MZ_OK;
}

extern "C" int mz_blur(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, void* hip_stream) {
    DegradeArgs a = {};
    if (int rc = check_degrade_views(x, out, elem, B, H, W, 0, &a)) return rc;
    BlurWeights bw = {};
    const int half = blur_weights(sigma, &bw);
    if (half < 0) return fail(MZ_ERR_INVALID_ARGUMENT, "sigma %g: need 0 <= sigma and int(3 sigma) <= %d", sigma, kBlurMaxHalf);
    if (half >= (H < W ? H : W))
        return fail(MZ_ERR_INVALID_ARGUMENT, "sigma %g needs %d pixels of reflect padding, a %d x %d image has no such reflection", sigma, half, H, W);
    return launched("blur launch", [&] { return launch_blur(a, bw, (hipStream_t)hip_stream); });
}

extern "C" int mz_noise(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, uint64_t seed,
                        uint64_t offset, void* hip_stream) {
    DegradeArgs a = {};
    if (int rc = check_degrade_views(x, out, elem, B, H, W, 1, &a)) return rc;
    if (!(sigma >= 0.0) || !(sigma <= 1e6)) return fail(MZ_ERR_INVALID_ARGUMENT, "sigma %g: need 0 <= sigma <= 1e6", sigma);
    return launched("noise launch", [&] { return launch_noise(a, sigma, seed, offset, (hipStream_t)hip_stream); });
}

extern "C" int mz_jpeg_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_batch_bounds(B, H, W)) return rc;
    *bytes = jpeg_plan(B, H, W).total;
    return MZ_OK;
}

extern "C" int mz_jpeg(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int quality, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
    DegradeArgs a = {};
    if (int rc = check_degrade_views(x, out, elem, B, H, W, 0, &a)) return rc;
    if (quality < 1 || quality > 100) return fail(MZ_ERR_INVALID_ARGUMENT, "quality must be 1..100, got %d", quality);
    const JpegPlan plan = jpeg_plan(B, H, W);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, plan.total)) return fail(r);
    JpegTables t;
    jpeg_qtable(quality, &t);
    return launched("jpeg launch", [&] { return launch_jpeg(a, t, plan, (char*)workspace, (hipStream_t)hip_stream); });
}

// Host only: what the kernels are handed and compile -- the blur weights of a sigma, the quantisation tables of a quality, one Philox block
extern "C" int mz_debug_blur_weights(double sigma, double* w, int cap) {
    BlurWeights bw = {};
    const int half = blur_weights(sigma, &bw);
    if (!w || half < 0 || 2 * half + 1 > cap) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument, a bad sigma (%g) or room for fewer than k weights", sigma);
    for (int j = 0; j <= 2 * half; ++j) w[j] = bw.w[j];
    return 2 * half + 1;
}
extern "C" int mz_debug_jpeg_qtable(int quality, uint8_t* luma, uint8_t* chroma) {
    if (!luma || !chroma || quality < 1 || quality > 100) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument or quality %d outside 1..100", quality);
    JpegTables t;
    jpeg_qtable(quality, &t);
    memcpy(luma, t.q[0], 64);
    memcpy(chroma, t.q[1], 64);
    return MZ_OK;
}
extern "C" int mz_debug_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    if (!counter || !key || !out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// the dihedral transforms and the self-ensemble accumulator (mz_dihedral.h): no reference counterpart in model.py; the flip is the
// reference's RandomHorizontalFlip (pretrain.py:148).  Stateless like mz_resize.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static const ViewRules kDihedralOut = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};
static const ViewRules kDihedralIn = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ false, /*batch_bound*/ true, /*side_bound*/ true};

static int check_orientation(int k) {
    return dihedral_valid(k) ? MZ_OK : fail(MZ_ERR_INVALID_ARGUMENT, "orientation k must be 0..7, got %d", k);
}

// the accumulator of a B x H x W result as a dense float32 view, after the workspace check: for the kernels and, as the public struct,
// for check_ranges_apart
static int ensemble_accumulator(int B, int H, int W, void* workspace, size_t workspace_bytes, StridedView* dense, mz_image_view* acc) {
    size_t need = 0;
    if (!ensemble_workspace_bytes(B, H, W, &need)) return fail(MZ_ERR_INVALID_ARGUMENT, "an accumulator of %d x 3 x %d x %d float32 is beyond 2^62 bytes", B, H, W);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, need)) return fail(r);
    *dense = dense_view(workspace, H, W);
    acc->data = workspace;
    for (int i = 0; i < 4; ++i) acc->stride[i] = dense->s[i];
    return MZ_OK;
}

extern "C" int mz_dihedral_inverse(int k) { return dihedral_inverse(k); }

extern "C" int mz_dihedral(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int k, void* hip_stream) {
    DihedralArgs a = {};
    if (const Refusal r = check_views(x, out, kDihedralOut, elem, B, H, W, &a.src, &a.dst)) return fail(r);
    if (int rc = check_orientation(k)) return rc;
    int Ho, Wo;
    dihedral_shape(k, H, W, &Ho, &Wo);
    if (int rc = check_ranges_apart(x, elem, H, W, out, elem, Ho, Wo, B, "x and out")) return rc;
    a.elem = elem; a.mode = DM_COPY; a.B = B; a.Hs = H; a.Ws = W; a.k = k;
    return launched("dihedral launch", [&] { return (hipError_t)launch_dihedral(a, hip_stream); });
}

extern "C" int mz_ensemble_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_batch_bounds(B, H, W)) return rc;
    if (!ensemble_workspace_bytes(B, H, W, bytes)) return fail(MZ_ERR_INVALID_ARGUMENT, "an accumulator of %d x 3 x %d x %d float32 is beyond 2^62 bytes", B, H, W);
    return MZ_OK;
}

extern "C" int mz_ensemble_add(const mz_image_view* y, int elem, int B, int H, int W, int k, int first, void* workspace, size_t workspace_bytes,
                               void* hip_stream) {
    DihedralArgs a = {};
    StridedView unused;
    if (const Refusal r = check_views(y, y, kDihedralIn, elem, B, H, W, &a.src, &unused)) return fail(r);
    if (int rc = check_orientation(k)) return rc;
    mz_image_view acc;
    if (int rc = ensemble_accumulator(B, H, W, workspace, workspace_bytes, &a.dst, &acc)) return rc;
    int Hy, Wy;  // y lies in ITS orientation: T(result, k)
    dihedral_shape(k, H, W, &Hy, &Wy);
    if (int rc = check_ranges_apart(y, elem, Hy, Wy, &acc, EL_F32, H, W, B, "y and the workspace")) return rc;
    a.elem = elem; a.mode = DM_ACC; a.B = B; a.Hs = Hy; a.Ws = Wy; a.k = dihedral_inverse(k); a.first = first != 0;
    return launched("ensemble add launch", [&] { return (hipError_t)launch_dihedral(a, hip_stream); });
}

extern "C" int mz_ensemble_finish(const mz_image_view* out, int elem, int B, int H, int W, int n, int clamp, const int32_t window[4],
                                  void* workspace, size_t workspace_bytes, void* hip_stream) {
    EnsembleFinishArgs a = {};
    StridedView unused;
    if (const Refusal r = check_views(out, out, kDihedralOut, elem, B, H, W, &unused, &a.out)) return fail(r);
    if (n != 1 && n != 2 && n != 4 && n != 8) return fail(MZ_ERR_INVALID_ARGUMENT, "n must be 1, 2, 4 or 8 orientations, got %d", n);
    if (const Refusal r = check_window(window, H, W, &a.y0, &a.x0, &a.h, &a.w)) return fail(r);
    mz_image_view acc;
    if (int rc = ensemble_accumulator(B, H, W, workspace, workspace_bytes, &unused, &acc)) return rc;
    if (int rc = check_ranges_apart(out, elem, a.h, a.w, &acc, EL_F32, H, W, B, "out and the workspace")) return rc;
    a.acc = (const float*)workspace;
    a.elem = elem; a.B = B; a.H = H; a.W = W; a.n = n; a.clamp = clamp != 0;
    return launched("ensemble finish launch", [&] { return (hipError_t)launch_ensemble_finish(a, hip_stream); });
}

// ------------------------------------------------------------------------------------------------
// images with an alpha channel (mz_alpha.h): the push-pull fill of the colour under a == 0, the merge of the enlarged alpha plane.  No
// reference counterpart: the reference's decode_image(mode="RGB") drops alpha.  Stateless like mz_resize.  Every check comes before
// anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static const ViewRules kAlphaOut = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};
static const ViewRules kAlphaIn = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ false, /*batch_bound*/ true, /*side_bound*/ true};

// two byte ranges of a call, each from its own channel count and shape
static int alpha_ranges_apart(const mz_image_view* a, int Ca, int Ha, int Wa, const mz_image_view* b, int Cb, int Hb, int Wb, int elem, int B,
                              const char* what) {
    long long al, ah, bl, bh;
    if (!view_extent(a, elem, B, Ha, Wa, &al, &ah, Ca) || !view_extent(b, elem, B, Hb, Wb, &bl, &bh, Cb))
        return fail(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
    if (al < bh && bl < ah) return fail(MZ_ERR_INVALID_ARGUMENT, "%s overlap: this entry does not work in place", what);
    return MZ_OK;
}

static int alpha_fill_plan(int B, int H, int W, AlphaPlan* plan) {
    if (int rc = check_batch_bounds(B, H, W)) return rc;
    if (!alpha_plan(B, H, W, plan)) return fail(MZ_ERR_INVALID_ARGUMENT, "the pyramid of %d images of %d x %d is beyond 2^62 bytes", B, H, W);
    return MZ_OK;
}

extern "C" int mz_alpha_fill_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    AlphaPlan plan;
    if (int rc = alpha_fill_plan(B, H, W, &plan)) return rc;
    *bytes = plan.total;
    return MZ_OK;
}

extern "C" int mz_alpha_fill(const mz_image_view* rgb, const mz_image_view* alpha, const mz_image_view* out, int elem, int B, int H, int W,
                             int premultiplied, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!rgb || !alpha || !out) return fail(MZ_ERR_INVALID_ARGUMENT, "null image view");
    mz_image_view al = *alpha;
    al.stride[1] = 1;  // one channel: its stride is never used, any value is accepted
    AlphaFillArgs a = {};
    StridedView unused;
    if (const Refusal r = check_views(rgb, out, kAlphaOut, elem, B, H, W, &a.rgb, &a.out)) return fail(r);
    if (const Refusal r = check_views(&al, &al, kAlphaIn, elem, B, H, W, &unused, &a.alpha)) return fail(r);
    if (int rc = alpha_ranges_apart(rgb, 3, H, W, out, 3, H, W, elem, B, "rgb and out")) return rc;
    if (int rc = alpha_ranges_apart(&al, 1, H, W, out, 3, H, W, elem, B, "alpha and out")) return rc;
    if (int rc = alpha_fill_plan(B, H, W, &a.plan)) return rc;
    if (const Refusal r = check_workspace(workspace, workspace_bytes, a.plan.total)) return fail(r);
    a.elem = elem; a.B = B; a.H = H; a.W = W;
    a.premultiplied = premultiplied != 0;
    a.ws = (char*)workspace;
    return launched("alpha fill launch", [&] { return (hipError_t)launch_alpha_fill(a, hip_stream); });
}

extern "C" int mz_alpha_merge(const mz_image_view* rgb, const mz_image_view* alpha, const mz_image_view* out_rgb, const mz_image_view* out_alpha,
                              int elem, int B, int Hin, int Win, int Hout, int Wout, int mode, int premultiply, void* hip_stream) {
    static const ViewRules plane = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ false};
    if (!alpha || !out_alpha || (premultiply && (!rgb || !out_rgb))) return fail(MZ_ERR_INVALID_ARGUMENT, "null image view");
    mz_image_view al = *alpha, oa = *out_alpha;
    al.stride[1] = oa.stride[1] = 1;
    AlphaMergeArgs a = {};
    if (const Refusal r = check_views(&al, &oa, plane, elem, B, Hout, Wout, &a.alpha, &a.out_alpha)) return fail(r);
    if (premultiply)
        if (const Refusal r = check_views(rgb, out_rgb, plane, elem, B, Hout, Wout, &a.rgb, &a.out_rgb)) return fail(r);
    if (int rc = check_sizes(Hin, Win, Hout, Wout)) return rc;
    if (int rc = alpha_ranges_apart(&al, 1, Hin, Win, &oa, 1, Hout, Wout, elem, B, "alpha and out_alpha")) return rc;
    if (premultiply)
        if (int rc = alpha_ranges_apart(&al, 1, Hin, Win, out_rgb, 3, Hout, Wout, elem, B, "alpha and out_rgb")) return rc;
    // (the last check: a call that arrives here with a bad mode has passed every check of its views, which is how tests/test_alpha_cpu.py
    // shows without a launch that a layout is accepted; mz_alpha_fill's last check is its workspace)
    if (int rc = check_interp_shape(Hin, Win, Hout, Wout, mode)) return rc;
    a.elem = elem;
    a.B = B;
    a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout;
    a.mode = mode;
    a.premultiply = premultiply != 0;
    return launched("alpha merge launch", [&] { return (hipError_t)launch_alpha_merge(a, hip_stream); });
}

// Host only: the levels of the pyramid of an H x W image, level 0 first
extern "C" int mz_debug_alpha_levels(int H, int W, int* hw, int cap) {
    if (cap < 0 || (!hw && cap > 0)) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument or negative cap");
    AlphaPlan plan;
    if (int rc = alpha_fill_plan(1, H, W, &plan)) return rc;
    for (int l = 0; l < plan.n && l < cap; ++l) {
        hw[2 * l] = plan.h[l];
        hw[2 * l + 1] = plan.w[l];
    }
    return plan.n;
}

// ------------------------------------------------------------------------------------------------
// feathered tiling (mz_feather.h): one rectangle pasted onto another with a linear cross-fade along its top and left edges.  No
// reference counterpart (the reference has no tiling code).  Stateless like mz_resize.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static const ViewRules kFeatherOut = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};

static int check_ramp(const char* name, int n) {
    return feather_ramp_ok(n) ? MZ_OK : fail(MZ_ERR_INVALID_ARGUMENT, "%s must be 0 .. 2^20 positions, got %d", name, n);
}

extern "C" int mz_feather_paste(const mz_image_view* src, const mz_image_view* dst, int elem, int B, int H, int W, int ramp_y, int ramp_x,
                                void* hip_stream) {
    FeatherArgs a = {};
    if (const Refusal r = check_views(src, dst, kFeatherOut, elem, B, H, W, &a.src, &a.dst)) return fail(r);
    if (const Refusal r = check_overlap(src, dst, elem, B, H, W, /*in_place_ok*/ false)) return fail(r);
    if (int rc = check_ramp("ramp_y", ramp_y)) return rc;
    if (int rc = check_ramp("ramp_x", ramp_x)) return rc;
    a.elem = elem; a.B = B; a.H = H; a.W = W; a.ramp_y = ramp_y; a.ramp_x = ramp_x;
    return launched("feather paste launch", [&] { return (hipError_t)launch_feather_paste(a, hip_stream); });
}

// Host only: omega(n, k), from the functions the kernel compiles
extern "C" int mz_debug_feather_weight(int n, int k, double* w) {
    if (!w) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_ramp("n", n)) return rc;
    if (k < 0) return fail(MZ_ERR_INVALID_ARGUMENT, "k must be at least 0, got %d", k);
    *w = feather_omega(n, feather_rho(n), k);
    return MZ_OK;
}
