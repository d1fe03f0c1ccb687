// What conv_kernel (mz_conv256.h), conv3w_kernel and conv3p_kernel (mz_conv3w.h) share: the software-pipelined K items of the
// 32x32 MFMA over an LDS stage (Geo<MODE>: mz_geo.h) and the epilogues on its accumulator layout.
//
// Everything here is written for 64-wide wavefronts and the CDNA4 matrix cores:
//   v_mfma_f32_32x32x16_{bf16,f16}  (8 K-elements per lane)  for the 16-bit modes
//   v_mfma_f32_32x32x2_f32          (exact f32)              for the f32 verification mode
//
// Convolution = implicit GEMM computed TRANSPOSED: D[n][pixel] = sum_k W[n][k] * X[pixel][k].
// The weight fragment is the MFMA "A" operand and the activation fragment the "B" operand, so an
// accumulator register quad holds 4 CONSECUTIVE channels of one pixel (rows of a 32x32 tile are
// (reg&3) + 8*(reg>>2) + 4*(lane>>5), the column = lane&31 = pixel): NHWC packing in the epilogue
// needs no cross-lane traffic.
//
// Activation tensors in HBM are "plane-major": [B][P][H][W][16 bytes], a plane being 16 bytes of
// consecutive channels (8 bf16/f16 or 4 f32 channels); P = padded_channels * sizeof / 16.  A 3x3 halo
// row or a run of pixels of one plane is then CONTIGUOUS in memory, so a global_load_lds instruction
// touches a handful of cache lines instead of one per lane.
//
// LDS image of one K-stage (all sizes in bytes; a "chunk" is 32 bytes of channels per pixel, i.e.
// 16 bf16/f16 channels or 8 f32 channels, split in two 16-byte "planes" = the two lane halves):
//   A (activations)  CONV3: [plane 2][pixel 352 (10 rows x 34 cols halo, padded)][16]   = 11264
//                    GEMM1: [chunk S][plane 2][pixel 256][16]                           = S*8192
//   B (weights)      [chunk S][tap][nt][lane 64][16]  — already in fragment order in HBM, so a
//                    stage is ONE contiguous run of TAPS*S*NT KiB copied by global_load_lds.
// Both images are lane-linear, which is what global_load_lds (LDS-DMA) requires, and every
// ds_read_b128 of a fragment covers contiguous 512-byte runs per half-wave: bank-conflict free.
#pragma once
#include "mz_device.h"
#include "mz_geo.h"

namespace mz {

// One "item" = one (chunk-in-stage, filter tap) pair = one 32-byte K-chunk of matrix work:
// 2 + NT fragment reads (two pixel fragments, NT weight fragments) feeding 2 * NT MFMAs.
template <int NT, int MODE, int ITEM, int K> __device__ __forceinline__ void issue_read(Frags<NT>& f, uint32_t a_addr, uint32_t b_addr) {
    using G = Geo<MODE>;
    constexpr int s = ITEM / G::TAPS, tap = ITEM % G::TAPS;
    constexpr int aofs = (MODE != MODE_GEMM1) ? ((tap / 3) * G::ROWW + (tap % 3)) * 16 : s * 8192;
    if constexpr (K == 0) f.x0 = lds_read128<aofs>(a_addr);
    else if constexpr (K == 1) f.x1 = lds_read128<aofs + G::MF_STRIDE>(a_addr);
    else if constexpr (K < 2 + NT) f.w[K - 2] = lds_read128<(ITEM * NT + (K - 2)) * 1024>(b_addr);
}
template <int NT, int MODE, int ITEM> __device__ __forceinline__ void issue_reads(Frags<NT>& f, uint32_t a_addr, uint32_t b_addr) {
    issue_read<NT, MODE, ITEM, 0>(f, a_addr, b_addr);
    issue_read<NT, MODE, ITEM, 1>(f, a_addr, b_addr);
    issue_read<NT, MODE, ITEM, 2>(f, a_addr, b_addr);
    issue_read<NT, MODE, ITEM, 3>(f, a_addr, b_addr);
    issue_read<NT, MODE, ITEM, 4>(f, a_addr, b_addr);
    issue_read<NT, MODE, ITEM, 5>(f, a_addr, b_addr);
}
// MFMA step M of an item (M = 2*nt + mf), followed by two of the NEXT item's fragment reads: the reads issue in
// the shadow of the MFMA just issued (the matrix pipe accepts one 32x32x16 MFMA per 32 cycles), and all of them
// are in flight at least (2*NT - 3) MFMAs before the item's closing s_waitcnt.
template <class TT, int NT, int MODE, int ITEM, int NITEMS, int M>
__device__ __forceinline__ void mfma_steps(f32x16 (&acc)[2][NT], const Frags<NT>& cur, Frags<NT>& nxt, uint32_t a_addr,
                                           uint32_t b_addr) {
    if constexpr (M < 2 * NT) {
        mma<TT>(acc[M & 1][M >> 1], cur.w[M >> 1], (M & 1) ? cur.x1 : cur.x0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ITEM + 1 < NITEMS) {
            issue_read<NT, MODE, ITEM + 1, 2 * M>(nxt, a_addr, b_addr);
            issue_read<NT, MODE, ITEM + 1, 2 * M + 1>(nxt, a_addr, b_addr);
            if constexpr (M == 2 * NT - 1) {  // NT == 1: 3 reads, 2 MFMAs
                issue_read<NT, MODE, ITEM + 1, 2 * M + 2>(nxt, a_addr, b_addr);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_steps<TT, NT, MODE, ITEM, NITEMS, M + 1>(acc, cur, nxt, a_addr, b_addr);
    }
}
// cur holds the (already waited-for) fragments of ITEM; nxt receives those of ITEM+1 while ITEM's MFMAs run.
template <class TT, int NT, int MODE, int ITEM, int NITEMS>
__device__ __forceinline__ void run_items(f32x16 (&acc)[2][NT], Frags<NT>& cur, Frags<NT>& nxt, uint32_t a_addr,
                                          uint32_t b_addr) {
    if constexpr (ITEM < NITEMS) {
        __builtin_amdgcn_sched_barrier(0);
        mfma_steps<TT, NT, MODE, ITEM, NITEMS, 0>(acc, cur, nxt, a_addr, b_addr);
        if constexpr (ITEM + 1 < NITEMS) wait_frags<NT>(nxt);
        run_items<TT, NT, MODE, ITEM + 1, NITEMS>(acc, nxt, cur, a_addr, b_addr);
    }
}

// PixelShuffle(2) + bicubic skip + residual add (+ clamp) -> NCHW image (reference model.py:926-930, 156, 162, 177).
// U8: both images are uint8 (a compile-time switch: a per-load branch would serialise the 48 taps of every lane).
// VIEW: both images are strided views (ConvArgs::vin / vout, 64-bit element offsets) and only the output pixels inside the window are
// stored; a lane then stores the three channels of one output pixel back to back, so that a packed HWC row of a wave is one run.
// The arithmetic is the dense instantiation's, operation by operation: a view changes addresses, never values.
template <class TT, int NT, bool U8, bool VIEW>
__device__ __forceinline__ void final_epilogue(const ConvArgs& a, f32x16 (&acc)[2][NT], char* ep, char* win, int lane, int b,
                                               const int (&ey)[2], const int (&ex)[2]) {
    constexpr int SZ = TT::SZ;
    const int h = lane >> 5, r = lane & 31;
    constexpr int ROWF = 80;  // 16 floats + 16 bytes pad
    const long long plane_i = (long long)a.Hi * a.Wi;
    const long long plane_o = (long long)a.Hout * a.Wout;
#pragma unroll
    for (int mf = 0; mf < 2; ++mf) {
        const int y = ey[mf];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[mf][0][4 * q + j];
            *(float4*)(ep + r * ROWF + (8 * q + 4 * h) * 4) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __builtin_amdgcn_wave_barrier();
        const int px = lane >> 1, jj = lane & 1;
        const int x = ex[mf] + px;
        const int X = 2 * x + jj;
        // the conv results of this lane's six outputs, read BEFORE any image load is issued: hipcc drains vmcnt to 0 in
        // front of every LDS read of a kernel that uses LDS-DMA, which would serialise the 96 image loads below
        float zres[2][3];
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
            for (int c = 0; c < 3; ++c) zres[i2][c] = *(const float*)(ep + px * ROWF + ((2 * i2 + jj) * 4 + c) * 4);
        // (wave-uniform; VIEW: a row pair outside the window's rows stores nothing)
        if (y < a.H && (!VIEW || (2 * y + 1 >= a.win_y0 && 2 * y < a.win_y0 + a.win_h))) {
            // The bicubic skip reads a 4 x 4 window of the input image per output pixel.  The 64 output columns x 2 output rows of this
            // fragment share ONE window of 4 (R = 4, 8: both rows fall into the same phase half of a source pixel) or 5 (R = 2) image
            // rows x at most 37 columns x 3 channels: the wave loads it once, lane l taking column cbase + l of every row and channel
            // (12 or 15 two-byte loads per lane), passes it through LDS, and every lane picks its 16 taps per channel from there.
            // Before, every lane loaded its own 96 taps: the kernel was bound by the number of load INSTRUCTIONS (a 64-lane load of
            // any width occupies the CU's address unit for 16 cycles; 95 % of the image head's time).
            const int R = a.R;
            int row0[2];
            float cy[2][4];
#pragma unroll
            for (int i2 = 0; i2 < 2; ++i2) {
                const int Y = 2 * y + i2;
                const int ky = Y / R, phy = Y - ky * R;
                const float sy = (phy + 0.5f) / (float)R - 0.5f;
                const int fy = sy < 0.0f ? -1 : 0;
                cubic_coeffs(sy - (float)fy, cy[i2]);
                row0[i2] = ky + fy - 1;  // first (unclamped) row of the 4-tap window
            }
            const int rbase = __builtin_amdgcn_readfirstlane(row0[0] < row0[1] ? row0[0] : row0[1]);
            const int d0 = __builtin_amdgcn_readfirstlane(row0[0] - rbase), d1 = __builtin_amdgcn_readfirstlane(row0[1] - rbase);  // 0 or 1
            const bool five = (d0 | d1) != 0;
            const int cbase = __builtin_amdgcn_readfirstlane((2 * ex[mf]) / R) - 2;  // column of window slot 0 (fx - 1 >= -2)
            const int wcol = min(max(cbase + lane, 0), a.Wi - 1);                    // (slots past the window hold clamped repeats)
            uint32_t* const wl = (uint32_t*)win;
            uint32_t wv[15];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long ip = VIEW ? (long long)b * a.vin[0] + (long long)c * a.vin[1] : ((long long)b * 3 + c) * plane_i;
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    if (i == 4 && !five) { wv[c * 5 + i] = 0u; break; }
                    const long long row = min(max(rbase + i, 0), a.Hi - 1);
                    wv[c * 5 + i] = ld_img_raw<TT, U8>(a.img, ip + (VIEW ? row * a.vin[2] + (long long)wcol * a.vin[3] : row * a.Wi + wcol));
                }
            }
#pragma unroll
            for (int j = 0; j < 15; ++j) wl[j * 64 + lane] = wv[j];
            __builtin_amdgcn_wave_barrier();
            if (x < a.W) {
                // horizontal taps of this output column
                const int kx = X / R, phx = X - kx * R;
                const float sx = (phx + 0.5f) / (float)R - 0.5f;
                const int fx = sx < 0.0f ? -1 : 0;
                float cx[4];
                cubic_coeffs(sx - (float)fx, cx);
                // window slot of the first tap: slot s holds column clamp(cbase + s), so slots o .. o + 3 are exactly the clamped taps
                // clamp(kx + fx - 1 + k) of the per-lane version; 0 <= o, o + 3 <= 36 (R = 2)
                const int o = kx + fx - 1 - cbase;
                float res[2][3];  // VIEW: this lane's six results, stored pixel by pixel behind the channel loop
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    // the rows' horizontal sums once, shared by both output rows (same operations in the same order as a per-row loop)
                    float rowv[5];
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        if (i == 4 && !five) { rowv[i] = 0.f; break; }
                        const uint32_t* t = wl + (c * 5 + i) * 64 + o;
                        rowv[i] = img_cvt<TT, U8>(t[0]) * cx[0] + img_cvt<TT, U8>(t[1]) * cx[1] + img_cvt<TT, U8>(t[2]) * cx[2] +
                                  img_cvt<TT, U8>(t[3]) * cx[3];
                    }
#pragma unroll
                    for (int i2 = 0; i2 < 2; ++i2) {
                        const int d = i2 == 0 ? d0 : d1;
                        float sres = 0.0f;
#pragma unroll
                        for (int i = 0; i < 4; ++i) sres += (d ? rowv[i + 1] : rowv[i]) * cy[i2][i];
                        float v = sres + zres[i2][c];
                        if (a.clamp) v = fminf(fmaxf(v, 0.0f), 1.0f);
                        const int Y = 2 * y + i2;
                        if constexpr (VIEW) res[i2][c] = v;
                        else st_img<TT, U8>(a.out, (((long long)b * 3 + c) * plane_o) + (long long)Y * a.Wout + X, v);
                    }
                }
                if constexpr (VIEW) {
                    const int Xw = X - a.win_x0;
#pragma unroll
                    for (int i2 = 0; i2 < 2; ++i2) {
                        const int Yw = 2 * y + i2 - a.win_y0;
                        if ((unsigned)Yw >= (unsigned)a.win_h || (unsigned)Xw >= (unsigned)a.win_w) continue;
                        const long long op = (long long)b * a.vout[0] + (long long)Yw * a.vout[2] + (long long)Xw * a.vout[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) st_img<TT, U8>(a.out, op + (long long)c * a.vout[1], res[i2][c]);
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// VIEW: true when none of the 2 th x 2 tw output pixels of the image head's tile at (y0, x0) lies inside the window: the workgroup
// would store nothing and may return before its K loop (upscale_tiled: the halo of a tile)
__device__ __forceinline__ bool tile_outside_window(const ConvArgs& a, int y0, int x0, int th, int tw) {
    return 2 * y0 >= a.win_y0 + a.win_h || 2 * (y0 + th) <= a.win_y0 || 2 * x0 >= a.win_x0 + a.win_w || 2 * (x0 + tw) <= a.win_x0;
}

// Store epilogues (STORE, D2S, MIX), specialised at compile time; `conv_epilogue` below dispatches.
template <class TT, int NT, bool IS_CONV, int EPI, bool SILU>
__device__ __forceinline__ void store_epilogue(const ConvArgs& a, f32x16 (&acc)[2][NT], int lane, int nbase, int b,
                                               const int (&ey)[2], const int (&ex)[2], const long long (&em)[2]) {
    constexpr int SZ = TT::SZ;
    const int h = lane >> 5, r = lane & 31;
    // Direct 16-byte stores, no LDS.  An accumulator quad = 4 consecutive channels of the lane's pixel.  f32: that is one
    // 16-byte plane entry.  16-bit types: lanes (0, r) and (1, r) hold the two halves of an entry, so two quads are
    // exchanged with v_permlane32_swap: afterwards lane (0, r) owns all 8 channels of the even quad's plane and lane
    // (1, r) those of the odd quad's plane.  r walks 32 consecutive pixels: one store instruction writes two
    // 512-byte runs.
    constexpr int PPU = SZ == 2 ? 8 : 4;  // channels per plane (= per 16-byte unit)
    constexpr int UNITS = SZ == 2 ? 2 : 4;  // store units this lane produces per 32-channel accumulator tile
    const long long hwo = (long long)a.Ho * a.Wo;
    const long long M = (long long)a.B * hwo;
    constexpr bool d2s = IS_CONV && EPI == EPI_D2S;
#pragma unroll
    for (int mf = 0; mf < 2; ++mf) {
        int bimg = -1;       // image index, -1 = pixel outside the tensor
        long long pix = 0;   // y * Wo + x inside the image
        int py = 0, pxx = 0;
        if (IS_CONV) {
            py = ey[mf];
            pxx = ex[mf] + r;
            if (py < a.H && pxx < a.W) {
                bimg = b;
                pix = (long long)py * a.W + pxx;
            }
        } else {
            const long long m = em[mf] + r;
            if (m < M) {
                bimg = (int)(m / hwo);
                pix = m - (long long)bimg * hwo;
            }
        }
        const long long plane_o = d2s ? (long long)a.Hout * a.Wout * 16 : hwo * 16;
        char* const obase = (char*)a.out + (long long)(bimg < 0 ? 0 : bimg) * a.p_out * plane_o;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int u = 0; u < UNITS; ++u) {
                float v[PPU];
                int cu;  // 16-byte unit index inside this workgroup's BN channels
                if constexpr (SZ == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float ea = acc[mf][nt][8 * u + j], eb = acc[mf][nt][8 * u + 4 + j];
                        const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, ea),
                                                                         __builtin_bit_cast(uint32_t, eb), false, false);
                        const uint32_t s0 = sw[0], s1 = sw[1];
                        v[j] = __builtin_bit_cast(float, s0);
                        v[4 + j] = __builtin_bit_cast(float, s1);
                    }
                    cu = 4 * nt + 2 * u + h;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = acc[mf][nt][4 * u + j];
                    cu = 8 * nt + 2 * u + h;
                }
                const int n = nbase + cu * PPU;
                if constexpr (SILU) {
#pragma unroll
                    for (int j = 0; j < PPU; ++j) v[j] = v[j] * sigmoidf_(v[j]);
                }
                if (bimg < 0) continue;
                char* dst;
                if constexpr (d2s) {
                    if (n >= 4 * a.cp_out) continue;
                    const int ij = n / a.cp_out;
                    const int c = n - ij * a.cp_out;
                    const int Y = 2 * py + (ij >> 1), X = 2 * pxx + (ij & 1);
                    dst = obase + (c / PPU) * plane_o + ((long long)Y * a.Wout + X) * 16;
                } else {
                    if (n >= a.cp_out) continue;
                    const int plane = n / PPU;
                    if constexpr (!IS_CONV && EPI == EPI_MIX) {  // only the 1x1 kernel runs the mix
                        float xv[PPU], zv[PPU];
                        ld_unit<TT>((const char*)a.in0 + (((long long)bimg * a.p0 + plane) * hwo + pix) * 16, xv);
                        ld_unit<TT>((const char*)a.in1 + (((long long)bimg * a.p1 + plane) * hwo + pix) * 16, zv);
#pragma unroll
                        for (int j = 0; j < PPU; ++j) v[j] = blend_(xv[j], zv[j], v[j], a.inv_mix_scale);
                    }
                    dst = obase + plane * plane_o + pix * 16;
                }
                st_unit<TT>(dst, v);
            }
        }
    }
}

// ================================================================================================
// epilogue, shared by every convolution kernel.  Wave-local (no workgroup barrier); only FINAL touches LDS (the
// wave's own region `ep`).  Pixel geometry of the wave's two M fragments:
//   IS_CONV: fragment mf covers pixels (ey[mf], ex[mf] + r) of image b;   else: linear pixels em[mf] + r.
// ================================================================================================
// VIEW: EPI_FINAL reads and writes image views (the kernels' VIEW instantiations)
template <class TT, int NT, bool IS_CONV, bool VIEW = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, const int epi, const int silu, f32x16 (&acc)[2][NT], char* ep,
                                              char* win, int lane, int nbase, int b, const int (&ey)[2], const int (&ex)[2],
                                              const long long (&em)[2]) {
    if (epi == EPI_FINAL) {
        if (IS_CONV) {
            if (a.io_u8) final_epilogue<TT, NT, true, VIEW>(a, acc, ep, win, lane, b, ey, ex);
            else final_epilogue<TT, NT, false, VIEW>(a, acc, ep, win, lane, b, ey, ex);
        }
        return;
    }
    if constexpr (IS_CONV) {
        if (epi == EPI_D2S) store_epilogue<TT, NT, true, EPI_D2S, false>(a, acc, lane, nbase, b, ey, ex, em);
        else if (silu) store_epilogue<TT, NT, true, EPI_STORE, true>(a, acc, lane, nbase, b, ey, ex, em);
        else store_epilogue<TT, NT, true, EPI_STORE, false>(a, acc, lane, nbase, b, ey, ex, em);
    } else {
        if (epi == EPI_MIX) store_epilogue<TT, NT, false, EPI_MIX, false>(a, acc, lane, nbase, b, ey, ex, em);
        else if (silu) store_epilogue<TT, NT, false, EPI_STORE, true>(a, acc, lane, nbase, b, ey, ex, em);
        else store_epilogue<TT, NT, false, EPI_STORE, false>(a, acc, lane, nbase, b, ey, ex, em);
    }
}

}  // namespace mz
