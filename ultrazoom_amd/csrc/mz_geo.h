// LDS geometry of the 256- and 512-pixel convolution kernels (conv_kernel, conv3w, conv3p, conv3s) and the LDS bytes their launches ask
// for.  Plain constexpr C++: the kernels and the host (Runner::conv3, mz_runner.h: a fused Conv3Call's x_via_lds) read the same constants.
#pragma once
#include "mz_kernels.h"

namespace mz {

#ifndef MZ_GEMM1_S
#define MZ_GEMM1_S 2  // K-chunks per stage of the 1x1 kernel: 44 KiB of LDS -> 3 workgroups per CU (measured best of 1..4)
#endif
template <int MODE> struct Geo;
template <> struct Geo<MODE_CONV3> {  // 4 waves, 8 x 32 pixels
    static constexpr int TAPS = 9;
    static constexpr int S = 1;            // chunks per stage
    static constexpr int ROWW = 34;        // halo row width
    static constexpr int A_ENT = 704;      // 16-byte entries per A image (2 planes x 352)
    static constexpr int PLANE = 352 * 16;
    static constexpr int MF_STRIDE = 34 * 16;  // second M fragment = next tile row
};
template <> struct Geo<MODE_GEMM1> {
    static constexpr int TAPS = 1;
    static constexpr int S = MZ_GEMM1_S;
    static constexpr int ROWW = 0;
    static constexpr int A_ENT = MZ_GEMM1_S * 512;
    static constexpr int PLANE = 256 * 16;
    static constexpr int MF_STRIDE = 32 * 16;
};
template <> struct Geo<MODE_C3W16> {  // 8 compute waves, 16 x 32 pixels: wave w owns rows 2w, 2w+1
    static constexpr int TAPS = 9;
    static constexpr int S = 1;
    static constexpr int TH = 16, TW = 32;
    static constexpr int ROWW = 34;
    static constexpr int NPIX = 18 * 34;   // 612 halo pixels
    static constexpr int PLANE_ENT = 640;  // padded so that 2 planes = a whole number of 64-entry DMA instructions
    static constexpr int A_ENT = 2 * PLANE_ENT;
    static constexpr int PLANE = PLANE_ENT * 16;
    static constexpr int MF_STRIDE = 34 * 16;
    static constexpr int ROW_PER_WAVE = 2;
};
template <> struct Geo<MODE_C3W8> {  // 8 compute waves, 8 x 64 pixels: wave w owns row w, fragments = its two halves
    static constexpr int TAPS = 9;
    static constexpr int S = 1;
    static constexpr int TH = 8, TW = 64;
    static constexpr int ROWW = 66;
    static constexpr int NPIX = 10 * 66;   // 660 halo pixels
    static constexpr int PLANE_ENT = 672;
    static constexpr int A_ENT = 2 * PLANE_ENT;
    static constexpr int PLANE = PLANE_ENT * 16;
    static constexpr int MF_STRIDE = 32 * 16;
    static constexpr int ROW_PER_WAVE = 1;
};
constexpr int kFinalWinBytes = 15 * 64 * 4;  // per wave: the bicubic window of a 32-pixel fragment (5 rows x 3 channels x 64 columns x 4 bytes)
constexpr int gemm1_chunks_per_stage() { return MZ_GEMM1_S; }
// one K stage in LDS: the A image + the weights of its chunks.  The 512-pixel kernels turn a ring of three such slots, conv_kernel two.
template <int MODE> constexpr int stage_bytes(int nt) { return Geo<MODE>::A_ENT * 16 + Geo<MODE>::TAPS * Geo<MODE>::S * nt * 1024; }
template <int MODE> constexpr size_t conv_lds_bytes(int nt) {
    constexpr bool wide = MODE == MODE_C3W16 || MODE == MODE_C3W8;
    constexpr size_t waves = wide ? 8 : 4;  // compute waves
    const size_t staging = (wide ? 3 : 2) * (size_t)stage_bytes<MODE>(nt);
    // epilogue scratch of the compute waves + (EPI_FINAL) their bicubic windows behind it: smem + waves * EPW + w * kFinalWinBytes
    const size_t epi = waves * 32 * (size_t)(32 * nt * 4 + 16) + waves * (size_t)kFinalWinBytes;
    return staging > epi ? staging : epi;
}
// conv3s_kernel: two 4-plane halo images + the two halves of a chunk's weights
template <int MODE> constexpr size_t conv16_lds_bytes(int nt, bool fuse) {
    const size_t a_slot = 4 * (size_t)Geo<MODE>::PLANE_ENT * 16;
    const size_t b_slot = 2 * (size_t)((9 * nt + 1) / 2) * 1024;
    const size_t gate = fuse ? (size_t)4 * nt * nt * 1024 : 0;  // lives in the second weight slot and the LDS behind it
    return 2 * a_slot + b_slot + (gate > b_slot ? gate : b_slot);
}

}  // namespace mz
