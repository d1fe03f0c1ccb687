// The weight packings (PackLayout, mz_kernels.h) as one map from a packed element to its OIHW source: pack_kernel (mz_kernels.hip)
// runs it on the device, mz_debug_pack (mz_debug.cpp) on the host.
#pragma once
#include "mz_kernels.h"

namespace mz {

// Element idx of a packing [ntile][kchunk][tap][frag][64 lanes][16 bytes] of SZ-byte elements -> its index in the float32 weights
// [cout][cin][kh][kw], or -1 for padding (packed as zero).
template <int SZ> __host__ __device__ inline long long pack_source(const PackArgs& a, long long idx) {
    constexpr int CK = SZ == 2 ? 16 : 8;  // channels per PK_MAIN chunk (chunk_channels())
    constexpr int EPL = 16 / SZ;          // elements per lane
    const bool s16 = a.layout != PK_MAIN;  // 16-channel fragments of the 16x16x32 MFMA, 32-channel K chunks
    long long t = idx;
    const int e = (int)(t % EPL); t /= EPL;
    const int lane = (int)(t % 64); t /= 64;
    const int nt = (int)(t % a.frags); t /= a.frags;
    const int tap = (int)(t % a.taps); t /= a.taps;
    const int kc = (int)(t % a.nchunks); t /= a.nchunks;
    const int nb = (int)t;
    int n = s16 ? (nb * a.frags + nt) * 16 + (lane & 15) : (nb * a.frags + nt) * 32 + (lane & 31);
    if (a.layout == PK_MIX16B) {
        // mix16b_kernel: accumulator rows in B-OPERAND order.  Row r = 4 g + j of fragment 2 m + h stands for channel
        // 32 m + 8 g + 4 h + j of the N tile, so that lane (g, c) of the accumulators owns exactly the eight channels whose x and z it
        // loaded as the B operand of K step m: the blend needs no second read of x and z, and its result is a whole 16-byte entry
        const int r = lane & 15;
        n = nb * (a.frags * 16) + 32 * (nt >> 1) + 8 * (r >> 2) + 4 * (nt & 1) + (r & 3);
    }
    const int hh = lane >> 5;
    const int kin = s16 ? (lane >> 4) * 8 + e : hh * (CK / 2) + e;  // channel within the chunk
    const int ckk = s16 ? 32 : CK;                                  // channels per chunk

    // output channel
    int o = -1;
    if (a.out_map == OUT_PLAIN) {
        o = n < a.cout ? n : -1;
    } else if (a.out_map == OUT_D2S) {
        const int ij = n / a.cq_p, c = n - ij * a.cq_p;
        o = (ij < 4 && c < a.cq) ? c * 4 + ij : -1;  // PixelShuffle(2): in-channel = c*4 + 2i + j
    } else {
        const int ij = n >> 2, c = n & 3;
        o = (n < 16 && c < 3) ? c * 4 + ij : -1;
    }
    // input channel and filter tap
    int ci = -1, ty = 0, tx = 0;
    if (a.in_map == SRC_PLAIN) {
        const int k = kc * ckk + kin;
        ci = k < a.c0 ? k : -1;
        ty = tap / a.kw;
        tx = tap - ty * a.kw;
    } else if (a.in_map == SRC_CONCAT) {
        int ks = kc;
        if (a.layout == PK_MIX16B) {
            // ... and the K steps of an N tile start with its OWN x and z channels (six steps each, kept in registers for the blend);
            // the rest follows in natural order (mix16b_step() in the kernel is the same map)
            const int hs = a.nchunks >> 1, t6 = 6 * nb;
            if (kc < 6) ks = t6 + kc;
            else if (kc < 12) ks = hs + t6 + (kc - 6);
            else {
                ks = kc - 12;
                if (ks >= t6) ks += 6;
                if (ks >= hs + t6) ks += 6;
            }
        }
        const int k = ks * ckk + kin;
        if (k < a.cp0) ci = k < a.c0 ? k : -1;
        else ci = (k - a.cp0) < a.c1 ? a.c0 + (k - a.cp0) : -1;
    } else if (a.layout == PK_GATE16T) {
        // conv3t_kernel's gate (C <= 48: three 16-channel fragments of x, three of z): K step kc = fragments 2 kc and 2 kc + 1 of
        // [x0 x1 x2 z0 z1 z2], the K elements of lane group g in accumulator-row order: e < 4 -> the first fragment's channels 4 g + e,
        // e >= 4 -> the second's
        const int g = lane >> 4;
        const int fr = 2 * kc + (e < 4 ? 0 : 1);
        const int ch = 16 * (fr % 3) + 4 * g + (e & 3);
        if (fr < 3) ci = ch < a.c0 ? ch : -1;
        else ci = ch < a.c1 ? a.c0 + ch : -1;
    } else if (a.layout == PK_GATE16 || a.layout == PK_GATE16R) {
        // fused gate for the 16x16x32 kernel: K-steps [0, ncx) = x channels in natural order (32 per step); then one
        // K-step per PAIR of 16-channel accumulator fragments of z, K elements in the order the accumulator quads of
        // lane group g = lane >> 4 supply them: e < 4 -> fragment 2m, channel 4g + e; e >= 4 -> fragment 2m + 1
        const int ncx = (a.cp0 + 31) / 32;
        if (kc < ncx && a.layout == PK_GATE16R) {
            // conv3r_kernel's fused variant: the x half in accumulator-row order too (x is fetched in accumulator layout, so
            // that a pair of its channel fragments is a B operand as it stands)
            const int g = lane >> 4;
            const int xch = 32 * kc + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
            ci = xch < a.c0 ? xch : -1;
        } else if (kc < ncx) {
            const int k = kc * 32 + kin;
            ci = k < a.c0 ? k : -1;
        } else {
            const int m = kc - ncx, g = lane >> 4;
            const int zch = 32 * m + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
            ci = zch < a.c1 ? a.c0 + zch : -1;
        }
    } else if (a.in_map == SRC_MIXF) {
        // fused AdaptiveResidualMix gate (PK_MAIN): chunks [0, ncx) = x channels in natural order; then one chunk per
        // (32-row accumulator tile, fragment g) of z, K-elements in ACCUMULATOR ROW order (ZFrag<TT>::make)
        const int ncx = a.cp0 / CK;
        if (kc < ncx) {
            const int k = kc * CK + kin;
            ci = k < a.c0 ? k : -1;
        } else {
            constexpr int ZG = SZ == 2 ? 2 : 4;
            const int gz = kc - ncx, ntz = gz / ZG, g = gz - ntz * ZG;
            const int zrow = 32 * ntz + (SZ == 2 ? 16 * g + 8 * (e >> 2) + 4 * hh + (e & 3) : 8 * g + 4 * hh + e);
            ci = zrow < a.c1 ? a.c0 + zrow : -1;
        }
    } else {  // CRUSH: K axis = [tap][padded channel]
        const int cpt = a.cp0 / CK;  // chunks per tap
        const int st = kc / cpt;
        const int k = (kc - st * cpt) * CK + kin;
        ci = (st < 4 && k < a.c0) ? k : -1;  // st >= 4: K padding
        ty = st >> 1;
        tx = st & 1;
    }
    if (o < 0 || ci < 0) return -1;
    return (((long long)o * a.cin + ci) * a.kh + ty) * a.kw + tx;
}

}  // namespace mz
