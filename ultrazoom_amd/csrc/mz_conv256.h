// conv_kernel: 256 output pixels x 32 NT channels per workgroup of 4 waves, 32x32 MFMA, 2-stage LDS pipeline (launcher: mz_conv32.hip).
//   MODE_CONV3: 3x3 on 8 x 32 pixel tiles (the image head);  MODE_GEMM1: 1x1 over a gathered K axis (mixes for C <= 96, PixelCrush).
#pragma once
#include "mz_conv_common.h"

namespace mz {

// Staging goes through LDS-DMA (global_load_lds).  -DMZ_REG_STAGING builds the same kernels with plain
// global loads + ds_write instead (a debugging aid: both variants must produce identical bits).
// No script or test builds that variant any more, but deleting the dead branches is a change of device code: stage_load's else
// branch names `tid`, so the lambda captures it, and without that capture every conv_kernel<.., MODE_CONV3> compiles to other
// address arithmetic (compared listing by listing).  It goes in a change that shows that listing diff.
#ifdef MZ_REG_STAGING
static constexpr bool kGlds = false;
#else
static constexpr bool kGlds = true;
#endif
// VIEW (MODE_CONV3, EPI_FINAL): the image head on image views (final_epilogue<.., VIEW>)
template <class TT, int NT, int MODE, bool VIEW = false>
__global__ __launch_bounds__(256, 2) void conv_kernel(const ConvArgs a) {
    using G = Geo<MODE>;
    constexpr int SZ = TT::SZ;
    constexpr int TAPS = G::TAPS;
    constexpr int S = G::S;
    constexpr int BN = 32 * NT;
    constexpr int A_BYTES = G::A_ENT * 16;
    constexpr int B_PIECES = TAPS * S * NT;
    constexpr int STAGE = A_BYTES + B_PIECES * 1024;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const int r = lane & 31;

    // ---- workgroup -> (pixel tile, N tile); consecutive logical ids share an XCD (and its L2) ----
    int mtile, ntile;
    if (!map_tile(a, mtile, ntile)) return;  // padding id of a partial tile group (whole workgroup, uniform)
    const int nbase = ntile * BN;
    const char* wtile = (const char*)a.wpk + (size_t)ntile * a.nchunks * (TAPS * NT * 1024);

    // ---- tile geometry ----
    int b = 0, y0 = 0, x0 = 0;   // CONV3
    long long m0 = 0;            // GEMM1
    const long long M = (long long)a.B * a.Ho * a.Wo;
    if (MODE == MODE_CONV3) {
        const int tpi = a.tiles_x * a.tiles_y;
        b = fdiv(mtile, tpi, a.inv_tpi);
        const int rem = mtile - b * tpi;
        const int ty = fdiv(rem, a.tiles_x, a.inv_tiles_x);
        y0 = ty * 8;
        x0 = (rem - ty * a.tiles_x) * 32;
        if constexpr (VIEW) {
            if (tile_outside_window(a, y0, x0, 8, 32)) return;  // (whole workgroup, uniform)
        }
    } else {
        m0 = (long long)mtile * 256;
    }

    // ---- per-thread staging sources (fixed for the whole K loop) ----
    // CONV3: entries e = tid + 256*i of the halo image; GEMM1: pixel m0 + tid of both sources.
    long long aoff[3];
    if (MODE == MODE_CONV3) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int e = tid + 256 * i;
            const int plane = e >= 352 ? 1 : 0;
            const int p = e - plane * 352;
            const int py = p / 34, px = p - py * 34;
            const int gy = y0 - 1 + py, gx = x0 - 1 + px;
            const bool ok = (e < 704) && (p < 340) && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            aoff[i] = ok ? ((((long long)b * a.p0 + plane) * a.H + gy) * a.W + gx) * 16 : -1;
        }
    } else {
        const long long m = m0 + tid;
        aoff[0] = aoff[1] = aoff[2] = -1;
        if (m < M) {
            const int hwo = a.Ho * a.Wo;
            const int bb = (int)(m / hwo);
            const int pix = (int)(m - (long long)bb * hwo);
            if (a.src == SRC_CRUSH) {
                const int oy = pix / a.Wo, ox = pix - oy * a.Wo;
                aoff[0] = ((long long)bb * a.p0 * a.H * a.W + (long long)(2 * oy) * a.W + 2 * ox) * 16;
            } else {
                aoff[0] = ((long long)bb * a.p0 * hwo + pix) * 16;
                aoff[1] = ((long long)bb * a.p1 * hwo + pix) * 16;
            }
        }
    }
    const long long plane_in = (long long)a.H * a.W * 16;  // bytes between two planes of an input tensor

    auto stage_load = [&](int st, int buf) {
        char* Abuf = smem + buf * STAGE;
        char* Bbuf = Abuf + A_BYTES;
        // ---- weights: contiguous run of pieces, one KiB per wave-instruction ----
        const int kc0 = st * S;
        const int npieces = B_PIECES;  // GEMM1: nchunks is padded to a multiple of S with zero weights
        const char* wsrc = wtile + (size_t)kc0 * (TAPS * NT * 1024);
        for (int j = w; j < npieces; j += 4) {
            if (kGlds) {
                glds16(wsrc + j * 1024 + lane * 16, Bbuf + j * 1024);
            } else {
                *(uint4*)(Bbuf + j * 1024 + lane * 16) = *(const uint4*)(wsrc + j * 1024 + lane * 16);
            }
        }
        // ---- activations ----
        if (MODE == MODE_CONV3) {
            const long long kbyte = 2LL * kc0 * plane_in;  // a K-chunk = two planes
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (i == 2 && w == 3) break;  // entries 704.. do not exist
                const char* src = aoff[i] >= 0 ? (const char*)a.in0 + aoff[i] + kbyte : (const char*)a.zero;
                if (kGlds) {
                    glds16(src, Abuf + (64 * w + 256 * i) * 16);
                } else {
                    *(uint4*)(Abuf + (tid + 256 * i) * 16) = *(const uint4*)src;
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int kc = kc0 + s;
                const char* base;
                if (kc >= a.nchunks_real) {
                    base = nullptr;  // K padding: zero activations against zero weights
                } else if (a.src == SRC_CRUSH) {
                    const int tap = kc / a.nchunks0;
                    const int cc = kc - tap * a.nchunks0;
                    const long long toff = ((long long)(tap >> 1) * a.W + (tap & 1)) * 16 + 2LL * cc * plane_in;
                    base = aoff[0] >= 0 ? (const char*)a.in0 + aoff[0] + toff : nullptr;
                } else if (kc < a.nchunks0) {
                    base = aoff[0] >= 0 ? (const char*)a.in0 + aoff[0] + 2LL * kc * plane_in : nullptr;
                } else {
                    base = aoff[1] >= 0 ? (const char*)a.in1 + aoff[1] + 2LL * (kc - a.nchunks0) * plane_in : nullptr;
                }
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const char* src = base ? base + hh * plane_in : (const char*)a.zero;
                    char* dstw = Abuf + s * 8192 + hh * 4096 + (64 * w) * 16;
                    if (kGlds) {
                        glds16(src, dstw);
                    } else {
                        *(uint4*)(dstw + lane * 16) = *(const uint4*)src;
                    }
                }
            }
        }
    };

    f32x16 acc[2][NT];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mf][nt][i] = 0.0f;

    const int a_lane = (MODE == MODE_CONV3) ? h * G::PLANE + ((2 * w) * 34 + r) * 16
                                            : h * G::PLANE + (64 * w + r) * 16;

    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const int nstages = (a.nchunks + S - 1) / S;
    stage_load(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int st = 0; st < nstages; ++st) {
        const int cur = st & 1;
        if (st + 1 < nstages) stage_load(st + 1, cur ^ 1);

        const uint32_t a_addr = lds_base + cur * STAGE + a_lane;
        const uint32_t b_addr = lds_base + cur * STAGE + A_BYTES + lane * 16;
        Frags<NT> fa, fb;
        issue_reads<NT, MODE, 0>(fa, a_addr, b_addr);
        wait_frags<NT>(fa);
        run_items<TT, NT, MODE, 0, TAPS * S>(acc, fa, fb, a_addr, b_addr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ============================== epilogue ==============================
    // The staging buffers are free now (every wave is past the last barrier, no DMA in flight).
    {
        constexpr int EPW = 32 * (BN * SZ + 16) > 32 * 80 ? 32 * (BN * SZ + 16) : 32 * 80;
        const int ey[2] = {y0 + 2 * w, y0 + 2 * w + 1};
        const int ex[2] = {x0, x0};
        const long long em[2] = {m0 + 64 * w, m0 + 64 * w + 32};
        conv_epilogue<TT, NT, MODE == MODE_CONV3, VIEW>(a, a.epi, a.silu, acc, smem + w * EPW, smem + 4 * EPW + w * kFinalWinBytes, lane, nbase, b, ey, ex, em);
    }
}

}  // namespace mz
