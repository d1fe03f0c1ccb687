// Host-only check of ultrazoom_amd/csrc/mz_alpha.h (tests/test_alpha_main_cpu.py builds it with plain g++ and the address and
// undefined-behaviour sanitizers and runs it; nothing of it is loaded into Python).  The header's host part compiled without HIP: the
// level sizes and the workspace at the ends of int and of the accepted range; one texel through level 0, push and pull at extreme values
// (NaN and infinite colour under a == 0, NaN alpha, the largest and smallest float32); the exact-constant property on one push and pull.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "../ultrazoom_amd/csrc/mz_alpha.h"

using namespace mz;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static bool zero_texel(const AlphaTexel& t) {
    const double z[4] = {0.0, 0.0, 0.0, 0.0};
    return memcmp(&t, z, sizeof z) == 0;  // +0 in every component, bit for bit
}
static bool same(const AlphaTexel& a, const AlphaTexel& b) { return memcmp(&a, &b, sizeof a) == 0; }

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double fmax32 = (double)std::numeric_limits<float>::max(), fmin32 = (double)std::numeric_limits<float>::denorm_min();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    AlphaPlan p;

    // ---- the pyramid ----
    CHECK(alpha_plan(1, 1, 1, &p) && p.n == 1 && p.h[0] == 1 && p.w[0] == 1 && p.total == 16);
    CHECK(alpha_plan(1, 1, 7, &p) && p.n == 4 && p.w[1] == 4 && p.w[2] == 2 && p.w[3] == 1 && p.h[3] == 1 && p.total == 16u * (4 + 2 + 1));
    CHECK(alpha_plan(2, 5, 3, &p) && p.n == 4 && p.h[1] == 3 && p.w[1] == 2 && p.h[2] == 2 && p.w[2] == 1 && p.total == 2u * 16u * (6 + 2 + 1));
    CHECK(p.off[1] == 0 && p.off[2] == 2u * 16u * 6 && p.off[3] == 2u * 16u * 8);
    CHECK(alpha_plan(1, 1 << 28, 1 << 28, &p) && p.n == 29 && p.h[28] == 1 && p.w[28] == 1 && p.h[1] == 1 << 27);
    {
        unsigned __int128 want = 0;
        for (int l = 1; l < p.n; ++l) want += (unsigned __int128)p.h[l] * (unsigned long long)p.w[l] * 16u;
        CHECK((unsigned __int128)p.total == want && p.off[p.n - 1] + 16 == p.total);
    }
    CHECK(alpha_plan(1, 1 << 28, 1, &p) && p.n == 29 && p.w[1] == 1 && p.h[28] == 1);
    CHECK(alpha_plan(4, 1 << 28, 1 << 28, &p) == false || p.total <= ((size_t)1 << 62));  // 4 * 2^60 * 4 / 3 passes 2^62
    CHECK(!alpha_plan(65535, 1 << 28, 1 << 28, &p));
    CHECK(!alpha_plan(1, (1 << 28) + 1, 1, &p) && !alpha_plan(1, 1, imax, &p) && !alpha_plan(1, imax, imax, &p));
    CHECK(!alpha_plan(1, 0, 1, &p) && !alpha_plan(1, 1, -1, &p) && !alpha_plan(1, imin, imin, &p) && !alpha_plan(0, 1, 1, &p) && !alpha_plan(imin, 1, 1, &p));
    CHECK(alpha_plan(65535, 1 << 14, 1 << 14, &p) && p.n == 15);

    // ---- the neighbour rule ----
    CHECK(alpha_neighbour(0, 1) == 0 && alpha_neighbour(0, 5) == 0 && alpha_neighbour(1, 5) == 1 && alpha_neighbour(2, 5) == 0 && alpha_neighbour(9, 5) == 4);
    CHECK(alpha_neighbour((1 << 28) - 1, 1 << 27) == (1 << 27) - 1 && alpha_neighbour((1 << 28) - 2, 1 << 27) == (1 << 27) - 2);

    // ---- level 0: a select, never a product ----
    CHECK(alpha_clamp01(nan) == 0.0 && alpha_clamp01(-inf) == 0.0 && alpha_clamp01(inf) == 1.0 && alpha_clamp01(-0.0) == 0.0);
    CHECK(zero_texel(alpha_texel0(0.0, nan, inf, -inf)) && zero_texel(alpha_texel0(alpha_clamp01(nan), 1.0, 1.0, 1.0)));
    CHECK(zero_texel(alpha_texel0(alpha_clamp01(-3.0), fmax32, -fmax32, nan)));
    CHECK(alpha_straight(nan, 0.0, 1) == 0.0 && alpha_straight(inf, 0.0, 1) == 0.0 && alpha_straight(0.5, 0.25, 1) == 1.0 &&
          alpha_straight(0.125, 0.25, 1) == 0.5 && alpha_straight(-1.0, 0.25, 1) == 0.0 && alpha_straight(7.0, 0.25, 0) == 7.0);
    {
        const AlphaTexel t = alpha_texel0(1.0, fmax32, fmin32, -fmax32);
        CHECK(t.w == 1.0 && t.r == fmax32 && t.g == fmin32 && t.b == -fmax32);
        const AlphaTexel u = alpha_texel0(fmin32, 1.0, fmax32, 0.5);  // the smallest alpha: a product below the subnormals is a zero, not a trap
        CHECK(u.w == fmin32 && u.r == fmin32 && u.b == 0.0 && u.g > 0.0);
    }

    // ---- push ----
    const AlphaTexel zero = {0.0, 0.0, 0.0, 0.0};
    CHECK(zero_texel(alpha_push(zero, zero, zero, zero)));
    {
        const float cf[3] = {0.1f, 0.7f, 1.0f};  // float32 colours: the sums and the division are exact
        const AlphaTexel one = alpha_texel0(1.0, cf[0], cf[1], cf[2]);
        CHECK(same(alpha_push(one, zero, zero, zero), one) && same(alpha_push(one, one, zero, zero), one) && same(alpha_push(zero, one, one, one), one) &&
              same(alpha_push(one, one, one, one), one));
        const AlphaTexel big = alpha_texel0(1.0, fmax32, fmax32, -fmax32);  // four of the largest: the float64 sum holds them, the division brings them back
        CHECK(same(alpha_push(big, big, big, big), big));
        const AlphaTexel part = alpha_texel0(0.25, 0.5, 0.5, 0.5);
        const AlphaTexel s = alpha_push(part, part, zero, zero);  // w = 0.5: no division
        CHECK(s.w == 0.5 && s.r == 0.25);
        // ---- pull ----
        const AlphaTexel U = alpha_up(one, one, one, one);
        CHECK(same(U, one));                                   // 9/16 + 3/16 + 3/16 + 1/16 of one value is that value
        CHECK(same(alpha_pull(zero, U), one));                 // an empty texel takes U
        CHECK(same(alpha_pull(one, alpha_up(big, big, big, big)), one));  // a full texel keeps itself: (1 - 1) U adds +0
        const AlphaTexel h = alpha_pull(s, U);                 // w = 0.5: half of U on top
        CHECK(h.w == 1.0 && h.r == alpha_f32(0.25 + 0.5 * (double)cf[0]));  // (the sum is exact in float64: one rounding, to float32)
        CHECK(alpha_fill_value(U.w, U.r) == (double)cf[0] && alpha_fill_value(0.0, 0.0) == 0.0 && alpha_fill_value(0.0, nan) == 0.0 &&
              alpha_fill_value(fmin32, fmax32) == 1.0 && alpha_fill_value(1.0, -fmax32) == 0.0);
        const AlphaTexel e = alpha_up(zero, zero, zero, zero);
        CHECK(zero_texel(e) && zero_texel(alpha_pull(zero, e)));  // a fully transparent image: zeros, no NaN
    }
    CHECK(alpha_premultiply(0.5, 0.5) == 0.25 && alpha_premultiply(1.0, 0.0) == 0.0);
    if (failures) return 1;
    printf("alpha header OK\n");
    return 0;
}
