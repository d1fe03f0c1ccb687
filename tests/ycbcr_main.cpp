// Host-only check of ultrazoom_amd/csrc/mz_ycbcr.h (tests/test_ycbcr_main_cpu.py builds it with plain g++ and the address and
// undefined-behaviour sanitizers and runs it; nothing of it is loaded into Python).  The header's host part compiled without HIP:
// the constants of every matrix, range and depth; depth 8 against yuv_coeffs bit for bit; every 16-bit word through read and write of
// every depth and alignment; the code function at NaN, infinities and the ends of the range; the per-pixel functions' round trip through
// float32 on random (Y, Cb, Cr) triples at every depth, matrix and range; ycbcr_chroma_mode on extreme strides.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "../ultrazoom_amd/csrc/mz_ycbcr.h"

using namespace mz;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {  // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (uint32_t)((state * 0x2545F4914F6CDD1Dull) >> 32);
}

int main() {
    static const int depths[4] = {8, 10, 12, 16};
    for (int di = 0; di < 4; ++di) {
        const int d = depths[di];
        CHECK(ycbcr_depth_valid(d));
        for (int align = 0; align < 2; ++align) {  // every word: read gives a code, and write(read) gives the word's code bits back
            const YcbcrWord w = ycbcr_word(d, align);
            CHECK(w.shift == (align == YCBCR_HIGH && d > 8 ? 16 - d : 0) && w.mask == (1u << d) - 1u);
            for (uint32_t word = 0; word < 65536u; ++word) {
                const int code = ycbcr_read(w, word);
                CHECK(code >= 0 && (uint32_t)code <= w.mask);
                const uint32_t back = ycbcr_write(w, (uint32_t)code);
                CHECK(back <= 65535u && ycbcr_read(w, back) == code);
                if (align == YCBCR_HIGH) CHECK((back & ((1u << w.shift) - 1u)) == 0u && back == (word & ~((1u << w.shift) - 1u) & (w.mask << w.shift)));
                if (failures) break;
            }
        }
        for (int matrix = 0; matrix < 3; ++matrix)
            for (int range = 0; range < 2; ++range) {
                const YcbcrCoeffs c = ycbcr_coeffs(matrix, range, d);
                const YuvCoeffs& k = c.k;
                CHECK(c.maxc == (double)((1 << d) - 1) && c.mid == (double)(1 << (d - 1)) && c.mid16 == 16 * (1 << (d - 1)));
                CHECK(fabs(k.kr + k.kg + k.kb - 1.0) < 1e-15 && k.g_r < 0 && k.g_b < 0 && k.inv_sy == 1.0 / k.sy && k.inv_sc == 1.0 / k.sc);
                if (d == 8 && matrix < 2) {
                    const YuvCoeffs o = yuv_coeffs(matrix, range);
                    CHECK(memcmp(&o, &k, sizeof o) == 0);
                }
                if (matrix == YCBCR_BT2020) CHECK(fabs(k.a_r - 1.4746) < 1e-15 && fabs(k.a_b - 1.8814) < 1e-15);
                // the code function: a NaN becomes 0, the clamp holds at the infinities, the ends are reached
                const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
                CHECK(ycbcr_code(k.sy, nan, k.yoff, c.maxc) == 0u && ycbcr_code(k.sy, -inf, k.yoff, c.maxc) == 0u);
                CHECK(ycbcr_code(k.sy, inf, k.yoff, c.maxc) == (uint32_t)c.maxc && ycbcr_code(k.sy, 1e300, k.yoff, c.maxc) == (uint32_t)c.maxc);
                CHECK(ycbcr_code(k.sc, 0.0, c.mid, c.maxc) == (uint32_t)c.mid);
                // the round trip of a pixel through float32 RGB: 100 000 random (Y, Cb, Cr) triples
                int mismatches = 0;
                for (int n = 0; n < 100000; ++n) {
                    const int y = (int)(next_u32() & (uint32_t)c.maxc), cb = (int)(next_u32() & (uint32_t)c.maxc), cr = (int)(next_u32() & (uint32_t)c.maxc);
                    const YuvRgb rgb = ycbcr_to_rgb_pixel(c, y, 16 * cb, 16 * cr);
                    const YuvPixel px = rgb_to_yuv_pixel(k, (double)(float)rgb.r, (double)(float)rgb.g, (double)(float)rgb.b);
                    mismatches += ycbcr_code(k.sy, px.y, k.yoff, c.maxc) != (uint32_t)y || ycbcr_code(k.sc, px.pb, c.mid, c.maxc) != (uint32_t)cb ||
                                  ycbcr_code(k.sc, px.pr, c.mid, c.maxc) != (uint32_t)cr;
                }
                CHECK(mismatches == 0);
                if (d == 8) {  // 16 times the chroma of mz_yuv.h's pixel function at the same inputs: the same bits
                    const YuvCoeffs o = matrix < 2 ? yuv_coeffs(matrix, range) : k;
                    const YuvRgb a = ycbcr_to_rgb_pixel(c, 77, 16 * 201 + 5, 16 * 3 + 11), b = yuv_to_rgb_pixel(o, 77, 16 * 201 + 5, 16 * 3 + 11);
                    CHECK(same_bits(a.r, b.r) && same_bits(a.g, b.g) && same_bits(a.b, b.b));
                }
            }
    }
    CHECK(!ycbcr_depth_valid(0) && !ycbcr_depth_valid(9) && !ycbcr_depth_valid(14) && !ycbcr_depth_valid(32) && !ycbcr_depth_valid(-8));
    CHECK(ycbcr_hc(5, YCBCR_420) == 3 && ycbcr_hc(5, YCBCR_422) == 5 && ycbcr_wc(5, YCBCR_422) == 3 && ycbcr_wc(5, YCBCR_444) == 5);
    CHECK(ycbcr_hc(1 << 28, YCBCR_420) == 1 << 27 && ycbcr_wc((1 << 28) - 1, YCBCR_420) == 1 << 27);

    // ycbcr_chroma_mode: the findings, and no overflow on strides at the ends of int64
    const long long big = std::numeric_limits<long long>::max(), small = std::numeric_limits<long long>::min();
    alignas(16) static uint16_t mem[64];
    for (int bytes = 1; bytes <= 2; ++bytes) {
        char* base = (char*)mem;
        const StridedView planar_b{base, {64, 0, 16, 1}}, planar_r{base + 32, {64, 0, 16, 1}};
        CHECK(ycbcr_chroma_mode(planar_b, planar_r, 2, 2, bytes) == CHROMA_PLANAR);
        const StridedView off_r{base + 32 + bytes, {64, 0, 16, 1}};
        CHECK(ycbcr_chroma_mode(planar_b, off_r, 2, 2, bytes) == CHROMA_ELEMENTS);
        const StridedView pair_b{base, {64, 0, 16, 2}}, pair_r{base + bytes, {64, 0, 16, 2}};
        CHECK(ycbcr_chroma_mode(pair_b, pair_r, 2, 2, bytes) == CHROMA_PAIRS_CB_FIRST);
        CHECK(ycbcr_chroma_mode(pair_r, pair_b, 2, 2, bytes) == CHROMA_PAIRS_CR_FIRST);
        const StridedView byte_r{base + 1, {64, 0, 16, 2}};  // one BYTE apart is a pair of bytes only
        CHECK(ycbcr_chroma_mode(pair_b, byte_r, 2, 2, bytes) == (bytes == 1 ? CHROMA_PAIRS_CB_FIRST : CHROMA_ELEMENTS));
        const StridedView row5_b{base, {64, 0, 5, 2}}, row5_r{base + bytes, {64, 0, 5, 2}};  // rows that are not aligned
        CHECK(ycbcr_chroma_mode(row5_b, row5_r, 2, 2, bytes) == CHROMA_ELEMENTS);
        const StridedView ext_b{base, {big, small, big, 2}}, ext_r{base + bytes, {big, small, big, 2}};
        CHECK(ycbcr_chroma_mode(ext_b, ext_r, 65535, 1 << 28, bytes) == CHROMA_ELEMENTS);
        const StridedView ext2_b{base, {small, big, small, 1}}, ext2_r{base + 32, {small, big, small, 1}};
        CHECK(ycbcr_chroma_mode(ext2_b, ext2_r, 65535, 1 << 28, bytes) == CHROMA_PLANAR);  // (2^63 is a multiple of 8)
    }
    if (failures) return 1;
    printf("ycbcr header OK\n");
    return 0;
}
