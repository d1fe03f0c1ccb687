// What every entry that takes mz_image_view refuses (include/mewzoom_hip.h, next to mz_image_view), stated once and called by all of them
// before anything touches the GPU.  Host code without a HIP header (plain g++ compiles it: tests/view_check_main.cpp runs it under
// the sanitizers); a check returns its code and message, the caller hands them to fail() (mz_err.h).
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mewzoom_hip.h"
#include "mz_view.h"

namespace mz {

struct Refusal {
    int code = MZ_OK;
    char msg[256] = "";
    explicit operator bool() const { return code != MZ_OK; }
};
__attribute__((format(printf, 2, 3))) inline Refusal refuse(int code, const char* fmt, ...) {
    Refusal r;
    r.code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof(r.msg), fmt, ap);
    va_end(ap);
    return r;
}

struct ViewRules {
    int elem_max;            // element codes 0..elem_max
    const char* elem_names;  // ".. must be <elem_names>, got .."
    bool second_is_output;   // the second view is written: no stride of 0 (false: both views are read)
    bool batch_bound;        // 1 <= B <= 65535 is checked here (false: the entry states its own bound)
    bool side_bound;         // 1 <= H, W <= 2^28 is checked here (false: the entry states its own bounds; H, W are not looked at)
};
#define MZ_ELEM_NAMES_0_3 "0 (f32), 1 (bf16), 2 (f16) or 3 (uint8)"

// The two views of a call on B images; fills the kernels' structs
inline Refusal check_views(const mz_image_view* first, const mz_image_view* second, const ViewRules& rules, int elem, int B, int H, int W,
                           StridedView* first_out, StridedView* second_out) {
    if (!first || !second) return refuse(MZ_ERR_INVALID_ARGUMENT, "null image view");
    if (!first->data || !second->data) return refuse(MZ_ERR_INVALID_ARGUMENT, "an image view has null data");
    if (elem < 0 || elem > rules.elem_max) return refuse(MZ_ERR_INVALID_ARGUMENT, "elem must be %s, got %d", rules.elem_names, elem);
    if (rules.batch_bound && (B < 1 || B > 65535)) return refuse(MZ_ERR_INVALID_ARGUMENT, "need 1 <= B <= 65535 (got %d)", B);
    if (rules.side_bound) {
        if (H < 1 || W < 1) return refuse(MZ_ERR_INVALID_ARGUMENT, "need H, W >= 1 (got %d x %d)", H, W);
        if (H > (1 << 28) || W > (1 << 28)) return refuse(MZ_ERR_INVALID_ARGUMENT, "at most 2^28 pixels a side (got %d x %d)", H, W);
    }
    static const char* const dim[4] = {"image", "channel", "row", "column"};
    first_out->data = first->data;
    second_out->data = second->data;
    for (int i = 0; i < 4; ++i) {
        first_out->s[i] = first->stride[i];
        second_out->s[i] = second->stride[i];
        if (rules.second_is_output && second->stride[i] == 0 && (i > 0 || B > 1))
            return refuse(MZ_ERR_INVALID_ARGUMENT, "the output view's %s stride is 0: its elements would overlap", dim[i]);
    }
    return Refusal();
}

// window {y0, x0, h, w} of an H x W result, or null for all of it
inline Refusal check_window(const int32_t window[4], int H, int W, int* y0, int* x0, int* h, int* w) {
    *y0 = 0; *x0 = 0; *h = H; *w = W;
    if (!window) return Refusal();
    *y0 = window[0]; *x0 = window[1]; *h = window[2]; *w = window[3];
    if (*h <= 0 || *w <= 0) return refuse(MZ_ERR_INVALID_ARGUMENT, "empty window (%d x %d)", *h, *w);
    if (*y0 < 0 || *x0 < 0 || (long long)*y0 + *h > H || (long long)*x0 + *w > W)
        return refuse(MZ_ERR_INVALID_ARGUMENT, "window {%d, %d, %d, %d} is not inside the %d x %d output", *y0, *x0, *h, *w, H, W);
    return Refusal();
}

// the byte range [lo, hi) the elements of a [B,C,H,W] view lie in (C = 1: mz_luma's output; its channel stride names nothing); false
// where it is no range of signed 64-bit addresses
inline bool view_extent(const mz_image_view* v, int elem, int B, int H, int W, long long* lo, long long* hi, int C = 3) {
    const long long n[4] = {B, C, H, W};
    __int128 a = 0, b = 0;  // |(n - 1) stride| < 2^28 2^63: four of them fit easily
    for (int i = 0; i < 4; ++i) {
        const __int128 span = (__int128)(n[i] - 1) * v->stride[i];
        if (span < 0) a += span; else b += span;
    }
    const __int128 es = elem == EL_F32 ? 4 : elem == EL_U8 ? 1 : 2, at = (long long)(intptr_t)v->data;
    const __int128 l = at + a * es, h = at + (b + 1) * es;
    if (l < INT64_MIN || h > INT64_MAX) return false;
    *lo = (long long)l;
    *hi = (long long)h;
    return true;
}

// x and out of an entry that reads neighbours (in_place_ok false) or one that reads and writes element by element (true: the same view
// twice is accepted): no other overlap of the two byte ranges
inline Refusal check_overlap(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, bool in_place_ok) {
    bool same = x->data == out->data;
    for (int i = 0; i < 4; ++i) same = same && x->stride[i] == out->stride[i];
    if (same && in_place_ok) return Refusal();
    long long xl, xh, ol, oh;
    if (!view_extent(x, elem, B, H, W, &xl, &xh) || !view_extent(out, elem, B, H, W, &ol, &oh))
        return refuse(MZ_ERR_INVALID_ARGUMENT, "a view's byte range does not fit in 63 bits");
    if (xl < oh && ol < xh)
        return refuse(MZ_ERR_INVALID_ARGUMENT, "%s", in_place_ok ? "x and out overlap without being the same view" : "x and out overlap: this entry does not work in place");
    return Refusal();
}

inline Refusal check_workspace(const void* workspace, size_t given, size_t needed) {
    if (!workspace || given < needed)
        return refuse(MZ_ERR_WORKSPACE_TOO_SMALL, "workspace too small: %zu bytes given, %zu needed", workspace ? given : (size_t)0, needed);
    return Refusal();
}

}  // namespace mz
