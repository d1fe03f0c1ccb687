// The reference's degradation chain (transforms.py: GaussianBlur, GaussianNoise, JPEGCompression; data.py:134-164 applies them around
// the antialiased resize of mz_resize.h) as gfx950 kernels on image views: mz_blur(), mz_noise(), mz_jpeg() of include/mewzoom_hip.h.
// No reference counterpart in model.py: stands in for torchvision's gaussian_blur / gaussian_noise / jpeg.  As in mz_resize.h: one
// kernel per element type serves every layout (one-element loads and stores), so dense and strided views give the same bits; all
// address arithmetic is 64-bit and signed; no atomics; a uint8 value v means v / 255 and is stored as clamp -> * 255 + 0.5 -> truncate.
//
// BLUR (blur_kernel): k = 2 * int(3 sigma) + 1 taps, half = k / 2;  w_j = exp(-0.5 (j / sigma)^2) / sum, j = -half .. half, in double, on
//   the host (at most 31 weights: they travel as a kernel argument);  separable, reflect padding without edge repeat (index -i -> i,
//   n - 1 + i -> n - 1 - i), per channel plane.  One workgroup of 256 threads = one 32 x 32 output tile of one plane: the haloed input
//   tile is staged in LDS as float32 (exact for every element type), the horizontal pass runs LDS -> LDS (float32 intermediate, as
//   resize_kernel's), the vertical pass LDS -> store.  Both passes accumulate in FLOAT64 as acc = fma(w_j, v_j, acc) from acc = +0 in
//   ascending j.  THE LAST STEP (st_f64, mz_view.h): the second sum is stored as (float)acc for float32, as u8_of_unit((float)acc) for
//   uint8, and rounded ONCE, from float64, to a 16-bit type (not through float32: resize_kernel's 16-bit results are rounded twice,
//   this kernel's never were).  No clamp.  k = 1 runs the same two passes with the one weight 1.0: every value comes back, a -0 as +0
//   (fma(1, -0, +0)).  tests/test_image_exact_gpu.py holds the kernel to this statement bit for bit.
//
// NOISE (noise_kernel): out = clamp(x + sigma n, 0, 1) in float64, one thread per element.  THE STREAM (stated here, once):
//   Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53, 0xCD9E8D57; key bumps (Weyl) 0x9E3779B9, 0xBB67AE85;
//   key = (seed lo, seed hi);  counter = (i lo, i hi, s lo, s hi),  i = (c H + y) W + x the logical element index within the image,
//   s = offset + b the stream id (b: image index within the call).  Of the four output words the first two are used:
//   U1 = (u0 + 0.5) / 2^32,  U2 = (u1 + 0.5) / 2^32,  n = sqrt(-2 ln U1) cos(2 pi U2), all float64.
//   The noise of a pixel depends on (seed, s, i) alone: not on the layout, the strides or how a batch is split into calls.
//   Degradation.sample (ultrazoom_amd/degrade.py) draws its parameters from the same generator at stream id 2^64 - 1.
//
// JPEG (jpeg_code_kernel, jpeg_image_kernel): a baseline JPEG round trip at quality 1..100 modelled in arithmetic (no entropy coder:
//   coding is lossless).  THE MODEL (tests/degrade_ref.py restates it in numpy):
//    1. x -> 8-bit RGB by the uint8 store rule, in float32 (identity for uint8)
//    2. Y  = (299 R + 587 G + 114 B + 500) / 1000;  Cb = (-168736 R - 331264 G + 500000 B + 128500000) / 1000000;
//       Cr = (500000 R - 418688 G - 81312 B + 128500000) / 1000000: integer division (the JFIF matrix at six digits, rounded half up),
//       clamped to 0..255
//    3. planes padded to multiples of 16 by edge replication
//    4. chroma 4:2:0: (sum of the 2 x 2 + bias) >> 2, bias 1, 2, 1, 2, .. along a row
//    5. per 8 x 8 block, f = sample - 128:  C[v][u] = sum_y sum_x T[v][y] T[u][x] f[y][x],  T[0][x] = sqrt(1/8),
//       T[u][x] = cos((2 x + 1) u pi / 16) / 2, float64 (rows first).  For u, v in {0, 4} T[u][x] T[v][y] = s_u(x) s_v(y) / 8 with signs
//       s_0 = +, s_4 = + - - + + - - +: those four coefficients are S / 8 of the INTEGER sum S
//    6. Q = clamp((base s + 50) / 100, 1, 255), s = 5000 / q for q < 50, else 200 - 2 q (integer divisions), base: the two tables of
//       ITU-T T.81 Annex K (jpeg_qtable() below: host, handed to the kernel by value)
//    7. level = round-half-away-from-zero(C / Q); the four exact ones in integers: sign(S) (|S| + 4 Q) / (8 Q).  D = level Q
//    8. sample = clamp(floor((E + 1024) / 8 + R + 0.5), 0, 255):  E = sum over u, v in {0, 4} of s_v(y) s_u(x) D[v][u] (integer),
//       R = sum over the other 60 of T[v][y] T[u][x] D[v][u] in float64 (over u first): an all-zero R leaves an exact value
//    9. chroma planes of ceil(H / 2) x ceil(W / 2), neighbours beyond an edge repeat the edge sample; for output (y, x): near = (y / 2,
//       x / 2), the far row is the one above for even y and below for odd y, the far column left for even x and right for odd x;
//       col(c) = 3 P[near row][c] + P[far row][c];  value = (3 col(near) + col(far) + (8 for even x, 7 for odd x)) >> 4
//   10. R = Y + 1.402 (Cr - 128), G = Y - 0.344136 (Cb - 128) - 0.714136 (Cr - 128), B = Y + 1.772 (Cb - 128) in integers at six
//       digits: floor((.. + 500000) / 1000000), clamped to 0..255, stored in the element type (float types: (float)v / 255.0f)
//   jpeg_code_kernel: one workgroup of 256 threads = kJpegMcus 16 x 16 MCUs side by side: steps 1-8 out of LDS, the decoded Y / Cb / Cr
//   planes (uint8, padded sizes) go to the caller's workspace.  jpeg_image_kernel: one thread per pixel, steps 9-10.  Every pixel's
//   arithmetic is that of its block and its neighbours' decoded chroma: it does not depend on the tile it falls in.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mz_view.h"

namespace mz {

constexpr int kBlurMaxHalf = 15;  // sigma < 16 / 3
constexpr int kBlurTile = 32;     // output pixels a side of one blur_kernel workgroup
constexpr int kDegradeThreads = 256;
static_assert(kDegradeThreads == kImageThreads, "grid_ok() (mz_view.h) bounds a grid of workgroups of kImageThreads threads");
constexpr int kJpegMcus = 2;      // 16 x 16 MCUs of one jpeg_code_kernel workgroup, side by side

struct BlurWeights {
    int half;
    double w[2 * kBlurMaxHalf + 1];
};
// k = 2 * int(3 sigma) + 1 (transforms.py:39); returns half, or -1 for a sigma that is not finite, negative or beyond kBlurMaxHalf
inline int blur_weights(double sigma, BlurWeights* bw) {
    if (!(sigma >= 0.0) || !(3.0 * sigma < (double)(kBlurMaxHalf + 1))) return -1;
    const int half = (int)(3.0 * sigma);
    bw->half = half;
    double sum = 0.0;
    for (int j = -half; j <= half; ++j) {
        const double u = half ? (double)j / sigma : 0.0;
        bw->w[j + half] = __builtin_exp(-0.5 * (u * u));
        sum += bw->w[j + half];
    }
    for (int j = 0; j <= 2 * half; ++j) bw->w[j] /= sum;
    return half;
}

struct JpegTables {
    uint8_t q[2][64];  // luminance, chrominance; row-major [v][u]
};
inline void jpeg_qtable(int quality, JpegTables* t) {
    static const uint8_t base[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 64; ++i) {
            const int v = (base[p][i] * s + 50) / 100;
            t->q[p][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

// workspace of one mz_jpeg call: the decoded planes, uint8: Y [B][Hp][Wp], then Cb and Cr [B][2][Hp / 2][Wp / 2]
struct JpegPlan {
    int Hp, Wp;  // H, W rounded up to multiples of 16
    size_t off_y, off_c, total;
};
inline JpegPlan jpeg_plan(int B, int H, int W) {
    JpegPlan p = {};
    p.Hp = (H + 15) / 16 * 16;
    p.Wp = (W + 15) / 16 * 16;
    const size_t plane = (size_t)p.Hp * p.Wp;
    p.off_y = 0;
    p.off_c = ((size_t)B * plane + 255) & ~(size_t)255;
    p.total = p.off_c + (((size_t)B * (plane / 2) + 255) & ~(size_t)255);
    return p;
}

struct DegradeArgs {
    StridedView x, out;
    int elem;  // Elem 0..3
    int B, H, W;
};
// Each enqueues one call; hipErrorInvalidValue for a grid beyond what grid_ok() (mz_view.h) can launch
hipError_t launch_blur(const DegradeArgs& a, const BlurWeights& bw, hipStream_t s);
hipError_t launch_noise(const DegradeArgs& a, double sigma, unsigned long long seed, unsigned long long offset, hipStream_t s);
hipError_t launch_jpeg(const DegradeArgs& a, const JpegTables& t, const JpegPlan& plan, char* ws, hipStream_t s);

// Philox4x32-10 of the header comment; host and device
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

#ifdef MZ_DEGRADE_KERNELS  // mz_degrade.hip only

__device__ __forceinline__ int reflect_index(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

// grid: tiles * 3 * B workgroups, tile fastest
template <int E>
__global__ __launch_bounds__(kDegradeThreads) void blur_kernel(const StridedView x, const StridedView out, int H, int W, long long tiles, int tiles_x,
                                                                 const BlurWeights bw) {
    constexpr int T = kBlurTile, S = T + 2 * kBlurMaxHalf, SP = 64;  // staged tile: at most S x S, rows SP floats apart
    static_assert(S <= SP, "row pitch");
    __shared__ float in_t[S * SP];
    __shared__ float hrow[S * T];
    __shared__ double wl[2 * kBlurMaxHalf + 1];
    const int tid = threadIdx.x, tx = tid & (T - 1), ty = tid / T;
    const int half = bw.half, k = 2 * half + 1;
    const PlaneTile pt = plane_tile(blockIdx.x, tiles, tiles_x);
    const long long b = pt.b, c = pt.c;
    const int y0 = pt.ty * T, x0 = pt.tx * T;
    const int th = min(T, H - y0), tw = min(T, W - x0);  // outputs of this tile
    const int rows = th + 2 * half, cols = tw + 2 * half;  // staged input: every index reflects into the image (half < min(H, W))
    if (tid < k) wl[tid] = bw.w[tid];
    const long long xb = b * x.s[0] + c * x.s[1];
    for (int e = tid; e < rows * cols; e += kDegradeThreads) {
        const int r = e / cols, q = e - r * cols;
        const int gy = reflect_index(y0 - half + r, H), gx = reflect_index(x0 - half + q, W);
        in_t[r * SP + q] = ld_f32<E>(x.data, xb + (long long)gy * x.s[2] + (long long)gx * x.s[3]);
    }
    __syncthreads();
    // horizontal pass: thread (ty, tx) filters column tx of rows ty, ty + 8, ..
    if (tx < tw)
        for (int r = ty; r < rows; r += kDegradeThreads / T) {
            double acc = 0.0;
            for (int j = 0; j < k; ++j) acc = fma(wl[j], (double)in_t[r * SP + tx + j], acc);
            hrow[r * T + tx] = (float)acc;
        }
    __syncthreads();
    // vertical pass out of LDS, then the store
    if (tx < tw)
        for (int r = ty; r < th; r += kDegradeThreads / T) {
            double acc = 0.0;
            for (int j = 0; j < k; ++j) acc = fma(wl[j], (double)hrow[(r + j) * T + tx], acc);
            st_f64<E>((void*)out.data, b * out.s[0] + c * out.s[1] + (long long)(y0 + r) * out.s[2] + (long long)(x0 + tx) * out.s[3], acc);
        }
}

// grid: ceil(3 H W / 256) * B workgroups, chunk fastest; a call of more workgroups than one grid holds (grid_ok(), mz_view.h) is
// several launches, each of the workgroups from wg0 on.  x and out may be the same view: a thread reads and writes its own element only
template <int E>
__global__ __launch_bounds__(kDegradeThreads) void noise_kernel(const StridedView x, const StridedView out, int H, int W, long long chunks, long long wg0,
                                                                  double sigma, unsigned long long seed, unsigned long long offset) {
    const long long wg = wg0 + blockIdx.x;
    const long long b = wg / chunks;
    const long long i = (wg - b * chunks) * kDegradeThreads + threadIdx.x;
    const long long hw = (long long)H * W;
    if (i >= 3 * hw) return;
    const long long c = i / hw, p = i - c * hw, y = p / W, xx = p - y * W;
    const unsigned long long s = offset + (unsigned long long)b;
    uint32_t u[4];
    philox4x32_10((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), (uint32_t)s, (uint32_t)(s >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), u);
    const double u1 = ((double)u[0] + 0.5) * (1.0 / 4294967296.0), u2 = ((double)u[1] + 0.5) * (1.0 / 4294967296.0);
    const double n = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
    double v = ld_f64<E>(x.data, b * x.s[0] + c * x.s[1] + y * x.s[2] + xx * x.s[3]) + sigma * n;
    v = fmin(fmax(v, 0.0), 1.0);  // (a NaN input becomes 0)
    st_f64_unit<E>((void*)out.data, b * out.s[0] + c * out.s[1] + y * out.s[2] + xx * out.s[3], v);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
__device__ __forceinline__ int dct_sign4(int x) { return ((x + 1) & 2) ? -1 : 1; }  // s_4: + - - + + - - +

// grid: ceil(Wp / (16 kJpegMcus)) * (Hp / 16) * B workgroups, tile fastest.  Blocks of one MCU: 0..3 Y (row-major), 4 Cb, 5 Cr
template <int E>
__global__ __launch_bounds__(kDegradeThreads) void jpeg_code_kernel(const StridedView x, int H, int W, int Hp, int Wp, long long tiles, int tiles_x,
                                                                      const JpegTables qt, uint8_t* ws_y, uint8_t* ws_c) {
    constexpr int M = kJpegMcus, NB = 6 * M, TW = 16 * M;
    __shared__ double Tm[64];           // T[u][x]
    __shared__ double tmp[NB * 64];     // the pass between the two 1-D transforms
    __shared__ int blk[NB * 64];        // samples - 128, then the dequantised coefficients D[v][u]
    __shared__ int isum[NB * 8 * 2];    // per block and row: the integer sums with s_0 and s_4 along x
    __shared__ int chroma[2][16 * TW];  // full-resolution Cb, Cr of the tile
    __shared__ uint8_t ql[2][64];
    const int tid = threadIdx.x;
    const long long wg = blockIdx.x;
    const long long b = wg / tiles;
    const int tile = (int)(wg - b * tiles);
    const int y0 = (tile / tiles_x) * 16, x0 = (tile % tiles_x) * TW;
    if (tid < 64) {
        const int u = tid >> 3, xx = tid & 7;
        Tm[tid] = u == 0 ? sqrt(0.125) : 0.5 * cos((double)((2 * xx + 1) * u) * (3.14159265358979323846 / 16.0));
    }
    if (tid < 128) ql[tid >> 6][tid & 63] = qt.q[tid >> 6][tid & 63];
    // steps 1-3: the tile's pixels (edge replication: rows beyond H, columns beyond W repeat the last one)
    const long long xb = b * x.s[0];
    for (int p = tid; p < 16 * TW; p += kDegradeThreads) {
        const int py = p / TW, px = p - py * TW;
        const long long at = xb + (long long)min(y0 + py, H - 1) * x.s[2] + (long long)min(x0 + px, W - 1) * x.s[3];
        const int r = ld_8bit<E>(x.data, at), g = ld_8bit<E>(x.data, at + x.s[1]), bl = ld_8bit<E>(x.data, at + 2 * x.s[1]);
        const int yy = (299 * r + 587 * g + 114 * bl + 500) / 1000;
        const int cb = (-168736 * r - 331264 * g + 500000 * bl + 128500000) / 1000000;
        const int cr = (500000 * r - 418688 * g - 81312 * bl + 128500000) / 1000000;
        const int m = px >> 4, lx = px & 15;
        blk[(m * 6 + (py >> 3) * 2 + (lx >> 3)) * 64 + (py & 7) * 8 + (lx & 7)] = clamp255(yy) - 128;
        chroma[0][p] = clamp255(cb);
        chroma[1][p] = clamp255(cr);
    }
    __syncthreads();
    // step 4: 4:2:0
    for (int e = tid; e < 2 * 8 * (TW / 2); e += kDegradeThreads) {
        const int pl = e / (8 * (TW / 2)), r = e - pl * (8 * (TW / 2)), cy = r / (TW / 2), cx = r - cy * (TW / 2);
        const int* s = &chroma[pl][(2 * cy) * TW + 2 * cx];
        const int v = (s[0] + s[1] + s[TW] + s[TW + 1] + 1 + (cx & 1)) >> 2;
        blk[((cx >> 3) * 6 + 4 + pl) * 64 + cy * 8 + (cx & 7)] = v - 128;
    }
    __syncthreads();
    // step 5, along x: tmp[b][y][u] = sum_x T[u][x] f[y][x]
    for (int e = tid; e < NB * 64; e += kDegradeThreads) {
        const int u = e & 7;
        const int* f = &blk[e & ~7];
        double acc = 0.0;
        for (int xx = 0; xx < 8; ++xx) acc = fma(Tm[u * 8 + xx], (double)f[xx], acc);
        tmp[e] = acc;
        if ((u & 3) == 0) {
            int s = 0;
            for (int xx = 0; xx < 8; ++xx) s += u ? dct_sign4(xx) * f[xx] : f[xx];
            isum[(e >> 3) * 2 + (u >> 2)] = s;
        }
    }
    __syncthreads();
    // step 5 along y, steps 6-7: D[v][u] over the samples
    for (int e = tid; e < NB * 64; e += kDegradeThreads) {
        const int bk = e >> 6, v = (e >> 3) & 7, u = e & 7;
        const int q = ql[(bk % 6) >= 4][v * 8 + u];
        int level;
        if (((u | v) & 3) == 0) {
            int s = 0;
            for (int yy = 0; yy < 8; ++yy) s += (v ? dct_sign4(yy) : 1) * isum[(bk * 8 + yy) * 2 + (u >> 2)];
            const int mag = ((s < 0 ? -s : s) + 4 * q) / (8 * q);
            level = s < 0 ? -mag : mag;
        } else {
            double acc = 0.0;
            for (int yy = 0; yy < 8; ++yy) acc = fma(Tm[v * 8 + yy], tmp[bk * 64 + yy * 8 + u], acc);
            const double t = acc / (double)q;
            level = t < 0.0 ? -(int)floor(-t + 0.5) : (int)floor(t + 0.5);
        }
        blk[e] = level * q;
    }
    __syncthreads();
    // step 8 along u: tmp[b][v][x] = sum_u T[u][x] D[v][u], without the exact four
    for (int e = tid; e < NB * 64; e += kDegradeThreads) {
        const int v = (e >> 3) & 7, xx = e & 7;
        const int* d = &blk[e & ~7];
        double acc = 0.0;
        for (int u = 0; u < 8; ++u)
            if (((u | v) & 3) != 0) acc = fma(Tm[u * 8 + xx], (double)d[u], acc);
        tmp[e] = acc;
    }
    __syncthreads();
    // step 8 along v, and the store of the decoded planes
    for (int e = tid; e < NB * 64; e += kDegradeThreads) {
        const int bk = e >> 6, yy = (e >> 3) & 7, xx = e & 7;
        double acc = 0.0;
        for (int v = 0; v < 8; ++v) acc = fma(Tm[v * 8 + yy], tmp[bk * 64 + v * 8 + xx], acc);
        const int* d = &blk[bk * 64];
        const int sx = dct_sign4(xx), sy = dct_sign4(yy);
        const int ex = d[0] + sx * d[4] + sy * (d[32] + sx * d[36]);
        const int val = clamp255((int)floor((double)(ex + 1024) * 0.125 + acc + 0.5));
        const int m = bk / 6, k = bk - m * 6;
        if (x0 + 16 * m >= Wp) continue;  // the last tile of a row may hold fewer MCUs
        if (k < 4) {
            const int gy = y0 + (k >> 1) * 8 + yy, gx = x0 + 16 * m + (k & 1) * 8 + xx;
            ws_y[(b * Hp + gy) * (long long)Wp + gx] = (uint8_t)val;
        } else {
            const int gy = y0 / 2 + yy, gx = x0 / 2 + 8 * m + xx;
            ws_c[((b * 2 + (k - 4)) * (Hp / 2) + gy) * (long long)(Wp / 2) + gx] = (uint8_t)val;
        }
    }
}

// grid: ceil(H W / 256) * B workgroups, chunk fastest
template <int E>
__global__ __launch_bounds__(kDegradeThreads) void jpeg_image_kernel(const StridedView out, int H, int W, int Hp, int Wp, long long chunks,
                                                                       const uint8_t* ws_y, const uint8_t* ws_c) {
    const long long wg = blockIdx.x;
    const long long b = wg / chunks;
    const long long p = (wg - b * chunks) * kDegradeThreads + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int y = (int)(p / W), xx = (int)(p - (long long)y * W);
    const int ch = (H + 1) / 2, cw = (W + 1) / 2, hp2 = Hp / 2, wp2 = Wp / 2;
    const int ny = y >> 1, nx = xx >> 1;
    const int fy = min(max((y & 1) ? ny + 1 : ny - 1, 0), ch - 1), fx = min(max((xx & 1) ? nx + 1 : nx - 1, 0), cw - 1);
    const int yv = ws_y[(b * Hp + y) * (long long)Wp + xx];
    int cv[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const uint8_t* P = ws_c + (b * 2 + pl) * (long long)hp2 * wp2;
        const int near_col = 3 * P[(long long)ny * wp2 + nx] + P[(long long)fy * wp2 + nx];
        const int far_col = 3 * P[(long long)ny * wp2 + fx] + P[(long long)fy * wp2 + fx];
        cv[pl] = (3 * near_col + far_col + ((xx & 1) ? 7 : 8)) >> 4;
    }
    const int db = cv[0] - 128, dr = cv[1] - 128;
    // floor((n + 500000) / 1000000) of a possibly negative n: shifted by 512 units
    const int r = (1000000 * yv + 1402000 * dr + 500000 + 512000000) / 1000000 - 512;
    const int g = (1000000 * yv - 344136 * db - 714136 * dr + 500000 + 512000000) / 1000000 - 512;
    const int bl = (1000000 * yv + 1772000 * db + 500000 + 512000000) / 1000000 - 512;
    const long long at = b * out.s[0] + (long long)y * out.s[2] + (long long)xx * out.s[3];
    st_8bit<E>((void*)out.data, at, clamp255(r));
    st_8bit<E>((void*)out.data, at + out.s[1], clamp255(g));
    st_8bit<E>((void*)out.data, at + 2 * out.s[1], clamp255(bl));
}

#endif  // MZ_DEGRADE_KERNELS

}  // namespace mz
