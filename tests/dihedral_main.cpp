// Host-only driver of ultrazoom_amd/csrc/mz_dihedral.h, the one statement of the eight orientations that the device kernels and the host
// entries compile: every k over the shapes 1 x 1 .. 5 x 7 -- source index, output shape, inverse -- against a restatement by explicit
// flips and a transposition of an index table.  tests/test_dihedral_main_cpu.py compiles it with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=undefined and runs it: exit status 0 and no sanitizer report (an index outside the image would end it).
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "../ultrazoom_amd/csrc/mz_dihedral.h"

using namespace mz;

static int g_failed = 0;
#define EXPECT(cond)                                                \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                             \
        }                                                           \
    } while (0)

struct Image {
    int H, W;
    std::vector<int> v;  // row-major
    int at(int i, int j) const { return v.at((size_t)i * W + j); }
};

// the transform by its three steps, each on a whole table: rows reversed (bit 1), columns reversed (bit 0), transposed (bit 2, last)
static Image by_steps(Image x, int k) {
    if (k & 2) {
        Image y = x;
        for (int i = 0; i < x.H; ++i)
            for (int j = 0; j < x.W; ++j) y.v[(size_t)i * x.W + j] = x.at(x.H - 1 - i, j);
        x = y;
    }
    if (k & 1) {
        Image y = x;
        for (int i = 0; i < x.H; ++i)
            for (int j = 0; j < x.W; ++j) y.v[(size_t)i * x.W + j] = x.at(i, x.W - 1 - j);
        x = y;
    }
    if (k & 4) {
        Image y = {x.W, x.H, std::vector<int>(x.v.size())};
        for (int i = 0; i < x.W; ++i)
            for (int j = 0; j < x.H; ++j) y.v[(size_t)i * x.H + j] = x.at(j, i);
        x = y;
    }
    return x;
}

// the transform through dihedral_shape / dihedral_source, as the kernels read it
static Image by_source(const Image& x, int k) {
    Image y;
    dihedral_shape(k, x.H, x.W, &y.H, &y.W);
    y.v.resize((size_t)y.H * y.W);
    for (int i = 0; i < y.H; ++i)
        for (int j = 0; j < y.W; ++j) {
            int si = -1, sj = -1;
            dihedral_source(k, x.H, x.W, i, j, &si, &sj);
            EXPECT(si >= 0 && si < x.H && sj >= 0 && sj < x.W);
            y.v[(size_t)i * y.W + j] = x.at(si, sj);
        }
    return y;
}

int main() {
    for (int H = 1; H <= 5; ++H)
        for (int W = 1; W <= 7; ++W) {
            Image x = {H, W, std::vector<int>((size_t)H * W)};
            for (size_t n = 0; n < x.v.size(); ++n) x.v[n] = (int)n;
            for (int k = 0; k < 8; ++k) {
                const Image want = by_steps(x, k), got = by_source(x, k);
                EXPECT(got.H == ((k & 4) ? W : H) && got.W == ((k & 4) ? H : W));
                EXPECT(got.H == want.H && got.W == want.W && got.v == want.v);
                const int inv = dihedral_inverse(k);
                EXPECT(inv >= 0 && inv <= 7 && dihedral_inverse(inv) == k && (k >= 4 || inv == k));
                const Image back = by_source(got, inv);
                EXPECT(back.H == H && back.W == W && back.v == x.v);
                for (int other = 0; other < 8; ++other)  // no other orientation undoes k (on shapes that tell them all apart)
                    if (other != inv && H >= 2 && W >= 2 && H != W) {
                        const bool fits = ((other & 4) ? got.W : got.H) == H;
                        EXPECT(!fits || by_source(got, other).v != x.v);
                    }
            }
        }
    for (int k : {INT_MIN, -1, 8, 9, INT_MAX}) EXPECT(!dihedral_valid(k) && dihedral_inverse(k) < 0);
    // the sizes at the entries' bounds: the last element of a 2^28 x 2^28 image, every k, without overflow
    for (int k = 0; k < 8; ++k) {
        const int side = 1 << 28;
        int Ho, Wo, si, sj;
        dihedral_shape(k, side, side - 1, &Ho, &Wo);
        dihedral_source(k, side, side - 1, Ho - 1, Wo - 1, &si, &sj);
        EXPECT(si == ((k & 2) ? 0 : side - 1) && sj == ((k & 1) ? 0 : side - 2));
    }
    size_t bytes = 0;
    EXPECT(ensemble_workspace_bytes(16, 4320, 7680, &bytes) && bytes == 12ull * 16 * 4320 * 7680);
    EXPECT(ensemble_workspace_bytes(65535, 1 << 14, 1 << 14, &bytes) && bytes == 12ull * 65535 * (1ull << 28));
    EXPECT(!ensemble_workspace_bytes(65535, 1 << 28, 1 << 28, &bytes));
    EXPECT(!ensemble_workspace_bytes(INT_MAX, INT_MAX, INT_MAX, &bytes));
    EXPECT(!ensemble_workspace_bytes(0, 8, 8, &bytes) && !ensemble_workspace_bytes(1, -8, 8, &bytes));

    if (g_failed) printf("%d expectation(s) failed\n", g_failed);
    else printf("dihedral checks OK\n");
    return g_failed ? 1 : 0;
}
