// Host-only driver of ultrazoom_amd/csrc/mz_view_check.h: extreme strides, sizes, windows and addresses through check_views,
// check_window, view_extent and check_overlap.  tests/test_view_checks_cpu.py compiles it with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=undefined and runs it: exit status 0 and no sanitizer report (a signed overflow in the checks would abort it).
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../ultrazoom_amd/csrc/mz_view_check.h"

using namespace mz;

static int g_failed = 0;
#define EXPECT(cond)                                                \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                             \
        }                                                           \
    } while (0)

static mz_image_view view(uintptr_t data, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
    mz_image_view v;
    v.data = (void*)data;
    v.stride[0] = s0; v.stride[1] = s1; v.stride[2] = s2; v.stride[3] = s3;
    return v;
}

static const ViewRules kOut = {3, MZ_ELEM_NAMES_0_3, true, true, true};     // as mz_blur / mz_noise / mz_jpeg
static const ViewRules kBoth = {3, MZ_ELEM_NAMES_0_3, false, false, false};  // as mz_metrics

int main() {
    const int side = 1 << 28;
    const int64_t extremes[] = {INT64_MAX, INT64_MIN, -1, 1, 0};
    const uintptr_t addresses[] = {0x10000, (uintptr_t)INT64_MAX - 64, UINTPTR_MAX - 64};  // low, the sign change, the top
    StridedView a, b;

    // check_views: the strides are copied as they are, whatever they are; only an output stride of 0 is refused
    for (int64_t s : extremes)
        for (uintptr_t at : addresses) {
            const mz_image_view x = view(at, s, s, s, s), dense = view(0x10000, 3LL * side * side, (int64_t)side * side, side, 1);
            Refusal r = check_views(&x, &dense, kOut, 3, 65535, side, side, &a, &b);
            EXPECT(r.code == MZ_OK && a.s[0] == s && a.s[3] == s && a.data == x.data && b.s[2] == side);
            r = check_views(&dense, &x, kOut, 0, 65535, side, side, &a, &b);
            EXPECT(r.code == (s == 0 ? MZ_ERR_INVALID_ARGUMENT : MZ_OK));
            EXPECT((r.code == MZ_OK) == (r.msg[0] == 0));
            r = check_views(&x, &x, kBoth, 3, INT_MAX, INT_MAX, INT_MIN, &a, &b);  // an entry that states its own bounds
            EXPECT(r.code == MZ_OK);
        }
    {
        const mz_image_view x = view(0x10000, 1, 1, 1, 1);
        EXPECT(check_views(nullptr, &x, kOut, 0, 1, 1, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
        EXPECT(check_views(&x, nullptr, kOut, 0, 1, 1, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
        const mz_image_view null_data = view(0, 1, 1, 1, 1);
        EXPECT(check_views(&null_data, &x, kOut, 0, 1, 1, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
        EXPECT(check_views(&x, &null_data, kOut, 0, 1, 1, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
        for (int elem : {INT_MIN, -1, 4, INT_MAX}) EXPECT(check_views(&x, &x, kOut, elem, 1, 1, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
        for (int batch : {INT_MIN, 0, 65536, INT_MAX}) EXPECT(check_views(&x, &x, kOut, 0, batch, 1, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
        for (int n : {INT_MIN, 0, side + 1, INT_MAX}) {
            EXPECT(check_views(&x, &x, kOut, 0, 1, n, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
            EXPECT(check_views(&x, &x, kOut, 0, 1, 1, n, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
        }
        const mz_image_view one_image = view(0x10000, 0, 1, 1, 1);
        EXPECT(check_views(&x, &one_image, kOut, 0, 1, 1, 1, &a, &b).code == MZ_OK);
        EXPECT(check_views(&x, &one_image, kOut, 0, 2, 1, 1, &a, &b).code == MZ_ERR_INVALID_ARGUMENT);
    }

    // check_window
    {
        int y0, x0, h, w;
        EXPECT(check_window(nullptr, INT_MAX, INT_MAX, &y0, &x0, &h, &w).code == MZ_OK && y0 == 0 && x0 == 0 && h == INT_MAX && w == INT_MAX);
        const int32_t all[4] = {0, 0, INT32_MAX, INT32_MAX}, last[4] = {INT32_MAX - 1, INT32_MAX - 1, 1, 1};
        EXPECT(check_window(all, INT_MAX, INT_MAX, &y0, &x0, &h, &w).code == MZ_OK && h == INT_MAX);
        EXPECT(check_window(last, INT_MAX, INT_MAX, &y0, &x0, &h, &w).code == MZ_OK && y0 == INT_MAX - 1 && w == 1);
        const int32_t bad[][4] = {{INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX}, {1, 0, INT32_MAX, 1}, {0, 1, 1, INT32_MAX}, {INT32_MAX, 0, 1, 1},
                                  {INT32_MIN, 0, 1, 1}, {0, INT32_MIN, INT32_MAX, INT32_MAX}, {0, 0, INT32_MIN, 1}, {0, 0, 1, 0}, {-1, 0, 4, 4}};
        for (const auto& win : bad) EXPECT(check_window(win, INT_MAX, INT_MAX, &y0, &x0, &h, &w).code == MZ_ERR_INVALID_ARGUMENT);
        const int32_t past[4] = {5, 0, 4, 4};
        EXPECT(check_window(past, 8, 8, &y0, &x0, &h, &w).code == MZ_ERR_INVALID_ARGUMENT);
    }

    // view_extent and check_overlap: whatever the strides and the address, a code and no overflow
    for (int64_t s : extremes)
        for (int64_t t : extremes)
            for (uintptr_t at : addresses)
                for (int elem = 0; elem < 4; ++elem) {
                    const mz_image_view x = view(at, s, t, s, t), out = view(0x10000, t, s, 1, s);
                    long long lo = 0, hi = 0;
                    if (view_extent(&x, elem, 65535, side, side, &lo, &hi)) EXPECT(lo < hi);
                    const int rc = check_overlap(&x, &out, elem, 65535, side, side, false).code;
                    EXPECT(rc == MZ_OK || rc == MZ_ERR_INVALID_ARGUMENT);
                    EXPECT(check_overlap(&x, &x, elem, 65535, side, side, true).code == MZ_OK);           // the same view, in place
                    EXPECT(check_overlap(&x, &x, elem, 65535, side, side, false).code == MZ_ERR_INVALID_ARGUMENT);
                }
    {
        long long lo, hi;
        const mz_image_view huge = view(0x10000, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX), tiny = view(0x10000, 1, 1, 1, 1);
        EXPECT(!view_extent(&huge, 0, 65535, side, side, &lo, &hi));  // no range of 63-bit addresses: refused, not undefined
        EXPECT(check_overlap(&huge, &tiny, 0, 65535, side, side, false).code == MZ_ERR_INVALID_ARGUMENT);
        EXPECT(check_overlap(&tiny, &huge, 0, 65535, side, side, true).code == MZ_ERR_INVALID_ARGUMENT);
        const mz_image_view top = view(UINTPTR_MAX - 4095, 3 * 16 * 16, 16 * 16, 16, 1);  // one 16 x 16 uint8 image under the top of the address space
        EXPECT(view_extent(&top, 3, 1, 16, 16, &lo, &hi) && hi - lo == 3 * 16 * 16);
        const mz_image_view bgr = view(0x10000 + 2 * 256 * 4, 768, -256, 16, 1);  // negative channel stride, data at channel 2
        EXPECT(view_extent(&bgr, 0, 2, 16, 16, &lo, &hi) && lo == 0x10000 && hi == 0x10000 + 2 * 768 * 4);
    }

    // the ordinary cases: a 1080 x 1920 float32 frame
    {
        const int H = 1080, W = 1920;
        const mz_image_view frame = view(0x100000, 3LL * H * W, (int64_t)H * W, W, 1);
        EXPECT(check_overlap(&frame, &frame, 0, 2, H, W, true).code == MZ_OK);                        // mz_noise in place
        EXPECT(check_overlap(&frame, &frame, 0, 2, H, W, false).code == MZ_ERR_INVALID_ARGUMENT);     // mz_blur in place
        // two 256 x 256 crops of the frame, the second shifted by (8, 8): they share pixels
        const mz_image_view crop = view(0x100000, 3LL * H * W, (int64_t)H * W, W, 1), shifted = view(0x100000 + 4 * (8 * W + 8), 3LL * H * W, (int64_t)H * W, W, 1);
        EXPECT(check_overlap(&crop, &shifted, 0, 1, 256, 256, false).code == MZ_ERR_INVALID_ARGUMENT);
        EXPECT(check_overlap(&crop, &shifted, 0, 1, 256, 256, true).code == MZ_ERR_INVALID_ARGUMENT);
        const mz_image_view apart = view(0x100000 + 4 * 3LL * H * W * 2, 3LL * H * W, (int64_t)H * W, W, 1);  // the frame behind the batch of two
        EXPECT(check_overlap(&frame, &apart, 0, 2, H, W, false).code == MZ_OK);
        EXPECT(check_workspace((void*)0x10000, 8, 16).code == MZ_ERR_WORKSPACE_TOO_SMALL);
        EXPECT(check_workspace(nullptr, SIZE_MAX, 16).code == MZ_ERR_WORKSPACE_TOO_SMALL);
        EXPECT(check_workspace((void*)0x10000, SIZE_MAX, SIZE_MAX).code == MZ_OK);
    }

    // the launchers' helpers of mz_view.h.  A grid dimension holds 2^32 - 1 work-items, 2^24 - 1 workgroups of 256 threads (kGridRowMax);
    // 2^24 - 1 = 3^2 5 7 13 17 241 is a multiple of 3, so a plane-tile grid can have exactly that many
    {
        const long long top = 16777215;
        EXPECT(kImageThreads == 256 && kGridRowMax == top && (top + 1) * kImageThreads == 1LL << 32);
        EXPECT(grid_ok(1) && grid_ok(top) && !grid_ok(0) && !grid_ok(-1) && !grid_ok(top + 1) && !grid_ok(INT32_MAX) && !grid_ok(LLONG_MIN));
        EXPECT(grid_ok(top, 1) && grid_ok(1, top) && grid_ok(5592405, 3) && !grid_ok(5592406, 3) && !grid_ok(4096, 4096) && !grid_ok(65536, 32768));
        EXPECT(!grid_ok(LLONG_MAX, LLONG_MAX) && !grid_ok(LLONG_MAX, 2) && !grid_ok(5, 0) && !grid_ok(5, -3));
        TileGrid g;
        const int h = 17 * 241, w = 3 * 5 * 7 * 13;  // h w = (2^24 - 1) / 3
        EXPECT(plane_tile_grid(h, w, 1, 1, 1, &g) && g.tiles_x == w && g.tiles_y == h && g.tiles == 5592405LL && g.wgs == top);
        EXPECT(plane_tile_grid(16 * h - 15, 32 * w, 16, 32, 1, &g) && g.tiles_x == w && g.tiles_y == h && g.wgs == top);
        EXPECT(plane_tile_grid(17, w, 1, 1, 241, &g) && g.tiles == 17LL * w && g.wgs == top);
        EXPECT(!plane_tile_grid(h + 1, w, 1, 1, 1, &g));           // one more row of tiles
        EXPECT(!plane_tile_grid(16 * h + 1, 32 * w, 16, 32, 1, &g));
        EXPECT(!plane_tile_grid(17, w, 1, 1, 242, &g));            // one more image
        EXPECT(!plane_tile_grid(side, side, 1, 1, 65535, &g));     // 2^56 tiles: refused before anything is multiplied by 3 B
        EXPECT(!plane_tile_grid(side, side, 1, 1, 1, &g));
        EXPECT(!plane_tile_grid(side, side, 1 << 14, 1 << 14, 2, &g));  // 3 * 2^29 workgroups: they fit an int, not a grid dimension
        EXPECT(plane_tile_grid(side, side, 1 << 17, 1 << 17, 1, &g) && g.tiles == 1LL << 22 && g.wgs == 3LL << 22);
        EXPECT(plane_tile_grid(1, 1, 64, 64, 65535, &g) && g.tiles_x == 1 && g.tiles_y == 1 && g.wgs == 3 * 65535);
        EXPECT(plane_tile_grid(33, 129, 32, 128, 1, &g) && g.tiles_x == 2 && g.tiles_y == 2 && g.wgs == 12);  // ragged last tiles
        for (int bad : {INT_MIN, -1, 0}) {
            EXPECT(!plane_tile_grid(bad, 8, 8, 8, 1, &g) && !plane_tile_grid(8, bad, 8, 8, 1, &g) && !plane_tile_grid(8, 8, 8, 8, bad, &g));
        }
        EXPECT(plane_tile_grid(INT_MAX, 1, INT_MAX, INT_MAX, 1, &g) && g.wgs == 3);  // (the rounding up is done in 64 bits)

        // rows_aligned: bf16 elements (2 bytes), 16-byte rows -> strides in multiples of 8 elements
        const StridedView flipped = {(void*)0x10000, {-64, -16, -8, 1}};  // negative strides are multiples too
        EXPECT(rows_aligned(flipped, 4, 4, 2, 16));
        const StridedView odd_row = {(void*)0x10000, {-64, -16, -12, 1}}, odd_image = {(void*)0x10000, {3, 16, 8, 1}}, odd_chan = {(void*)0x10000, {64, 3, 8, 1}};
        EXPECT(!rows_aligned(odd_row, 4, 4, 2, 16) && rows_aligned(odd_row, 4, 1, 2, 16));     // one row: its stride is never stepped
        EXPECT(!rows_aligned(odd_image, 2, 4, 2, 16) && rows_aligned(odd_image, 1, 4, 2, 16));  // one image: likewise
        EXPECT(!rows_aligned(odd_chan, 1, 1, 2, 16));                                            // there are always three channels
        const StridedView off_base = {(void*)0x10008, {64, 16, 8, 1}};
        EXPECT(!rows_aligned(off_base, 1, 1, 2, 16) && rows_aligned(off_base, 1, 1, 2, 8) && !rows_aligned(off_base, 4, 4, 4, 16));
        const StridedView extreme = {(void*)(UINTPTR_MAX - 15), {INT64_MIN, INT64_MAX, INT64_MIN, 1}};
        EXPECT(!rows_aligned(extreme, 2, 2, 1, 16));  // INT64_MAX is odd

        // dense_view: the strides at the largest sides are exact, and the public checks refuse what 65535 such images would span
        const StridedView d = dense_view((void*)0x10000, side, side);
        EXPECT(d.data == (void*)0x10000 && d.s[0] == 3LL << 56 && d.s[1] == 1LL << 56 && d.s[2] == side && d.s[3] == 1);
        EXPECT((__int128)d.s[0] == (__int128)3 * side * side && d.s[0] < INT64_MAX / 2);
        const mz_image_view dv = view(0x10000, d.s[0], d.s[1], d.s[2], d.s[3]);
        long long lo, hi;
        EXPECT(!view_extent(&dv, 0, 65535, side, side, &lo, &hi));
        EXPECT(view_extent(&dv, 3, 2, side, side, &lo, &hi) && hi - lo == 6LL << 56);
        const StridedView small = dense_view(nullptr, 5, 7);
        EXPECT(small.s[0] == 105 && small.s[1] == 35 && small.s[2] == 7 && small.s[3] == 1);
    }

    if (g_failed) printf("%d expectation(s) failed\n", g_failed);
    else printf("view checks OK\n");
    return g_failed ? 1 : 0;
}
