// conv3w_kernel / conv3p_kernel: 3x3 convolution on 512-pixel tiles with the 32x32 MFMA, per tile and persistent (launchers: mz_conv32.hip).
#pragma once
#include "mz_conv_common.h"

namespace mz {

// ================================================================================================
// 3x3 convolution, wide tile: 512 output pixels x BN channels per workgroup, 8 compute waves + 1 loader wave.
//   - the weight stage (9 * NT KiB per K-chunk) is fetched ONCE for 512 pixels, by a dedicated wave;
//   - each compute wave issues only its 2-3 activation DMA instructions per stage;
//   - 3-slot LDS ring [A0 B0 | A1 B1 | A2 B2], prefetch distance 2 stages, counted s_waitcnt vmcnt(N): the
//     DMA of stage t+2 stays in flight across the single barrier of stage t.  The ring is rotated so that the
//     LAST stage sits in slot 0: slots 1-2 are then one contiguous free region during the last stage(s).
//   - FUSE: the AdaptiveResidualMix that follows conv2 of a block (reference model.py:507-511, 826-839) runs in
//     the epilogue.  With BN == all channels every wave owns all channels of its 64 pixels, so the gate
//     beta = Wx.x + Wz.z is wave-local: z goes from the accumulators straight into the MFMA B operand (the
//     accumulator rows are the K index; the gate weights are packed in that row order), x fragments come
//     from HBM as plain 16-byte loads (plane-major layout), and the gate weights are prefetched by the loader
//     wave into ring slots 1-2 while the last K-stage is being computed.
// ================================================================================================

// z accumulators -> MFMA B-operand fragments, and back to the (rounded) values for the blend
template <class TT> struct ZFrag;
template <> struct ZFrag<TF32> {
    static constexpr int ZG = 4;  // fragments per 32-row accumulator tile
    static __device__ __forceinline__ u32x4 make(const f32x16& t, int g) {
        // (copy each element to a scalar first: __builtin_bit_cast applied to an ext-vector element reads element 0)
        const float e0 = t[4 * g + 0], e1 = t[4 * g + 1], e2 = t[4 * g + 2], e3 = t[4 * g + 3];
        u32x4 f;
        f[0] = __builtin_bit_cast(uint32_t, e0); f[1] = __builtin_bit_cast(uint32_t, e1);
        f[2] = __builtin_bit_cast(uint32_t, e2); f[3] = __builtin_bit_cast(uint32_t, e3);
        return f;
    }
    static __device__ __forceinline__ void quad(const u32x4 (&f)[4], int q, float v[4]) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const f32x4 t = __builtin_bit_cast(f32x4, f[q]);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    }
};
template <> struct ZFrag<TBF16> {
    static constexpr int ZG = 2;
    static __device__ __forceinline__ u32x4 make(const f32x16& t, int g) {
        u32x4 f;
        f[0] = pack_bf16(t[8 * g + 0], t[8 * g + 1]); f[1] = pack_bf16(t[8 * g + 2], t[8 * g + 3]);
        f[2] = pack_bf16(t[8 * g + 4], t[8 * g + 5]); f[3] = pack_bf16(t[8 * g + 6], t[8 * g + 7]);
        return f;
    }
    static __device__ __forceinline__ void quad(const u32x4 (&f)[2], int q, float v[4]) {
        const u32x4 t = f[q >> 1];
        const uint32_t lo = (q & 1) ? t[2] : t[0], hi = (q & 1) ? t[3] : t[1];
        v[0] = __builtin_bit_cast(float, lo << 16); v[1] = __builtin_bit_cast(float, lo & 0xffff0000u);
        v[2] = __builtin_bit_cast(float, hi << 16); v[3] = __builtin_bit_cast(float, hi & 0xffff0000u);
    }
};
template <> struct ZFrag<TF16> {
    static constexpr int ZG = 2;
    static __device__ __forceinline__ u32x4 make(const f32x16& t, int g) {
        u32x4 f;
        f[0] = pack_f16(t[8 * g + 0], t[8 * g + 1]); f[1] = pack_f16(t[8 * g + 2], t[8 * g + 3]);
        f[2] = pack_f16(t[8 * g + 4], t[8 * g + 5]); f[3] = pack_f16(t[8 * g + 6], t[8 * g + 7]);
        return f;
    }
    static __device__ __forceinline__ void quad(const u32x4 (&f)[2], int q, float v[4]) {
        const u32x4 t = f[q >> 1];
        const uint32_t lo = (q & 1) ? t[2] : t[0], hi = (q & 1) ? t[3] : t[1];
        v[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(lo & 0xffff)); v[1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(lo >> 16));
        v[2] = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi & 0xffff)); v[3] = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi >> 16));
    }
};

// VIEW (EPI_FINAL, not FUSE): the image head on image views (final_epilogue<.., VIEW>)
template <class TT, int NT, int MODE, bool FUSE, bool VIEW = false>
__global__ __launch_bounds__(576, 3) void conv3w_kernel(const ConvArgs a) {
    using G = Geo<MODE>;
    constexpr int SZ = TT::SZ;
    constexpr int BN = 32 * NT;
    constexpr int A_SLOT = G::A_ENT * 16;
    constexpr int A_INSTR = G::A_ENT / 64;
    constexpr int B_PIECES = 9 * NT;
    constexpr int B_SLOT = B_PIECES * 1024;
    constexpr int SLOT = A_SLOT + B_SLOT;
    static_assert(B_PIECES < 60, "vmcnt is a 6-bit counter");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7 compute, 8 = weight loader
    const int h = lane >> 5;
    const int r = lane & 31;

    int mtile, ntile;
    if (!map_tile(a, mtile, ntile)) return;  // padding id of a partial tile group (whole workgroup, uniform)
    const int nbase = ntile * BN;
    const int nstages = a.nchunks;
    const int last = nstages - 1;
    const int s0 = (3 - last % 3) % 3;  // slot(st) = (st + s0) % 3, so slot(last) == 0
    char* const mixw = smem + SLOT;     // FUSE: gate weights live in slots 1-2 once those are free
    if constexpr (VIEW) {  // the tile's origin as the compute waves derive it below, ahead of the loader wave's branch
        const int vtpi = a.tiles_x * a.tiles_y;
        const int vrem = mtile - fdiv(mtile, vtpi, a.inv_tpi) * vtpi;
        const int vty = fdiv(vrem, a.tiles_x, a.inv_tiles_x);
        if (tile_outside_window(a, vty * G::TH, (vrem - vty * a.tiles_x) * G::TW, G::TH, G::TW)) return;  // (whole workgroup, uniform)
    }

    if (w == 8) {
        // ------------------------- weight loader wave -------------------------
        const char* wsrc = (const char*)a.wpk + (size_t)ntile * a.nchunks * (B_PIECES * 1024) + lane * 16;
        auto loadB = [&](int st, int slot) {
            const char* src = wsrc + (size_t)st * (B_PIECES * 1024);
            char* dst = smem + slot * SLOT + A_SLOT;
#pragma unroll
            for (int j = 0; j < B_PIECES; ++j) glds16(src + j * 1024, dst + j * 1024);
        };
        int sl = s0;
        loadB(0, sl);
        sl = sl == 2 ? 0 : sl + 1;
        if (nstages > 1) loadB(1, sl);
        sl = sl == 2 ? 0 : sl + 1;  // slot of stage st + 2
        const int mix1 = FUSE ? (a.mix_pieces < SLOT / 1024 ? a.mix_pieces : SLOT / 1024) : 0;  // pieces that fit slot 1
        for (int st = 0; st < nstages; ++st) {
            if (st + 1 < nstages) wait_vmcnt<B_PIECES>(); else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            if (st + 2 < nstages) loadB(st + 2, sl);
            if (FUSE) {
                const char* msrc = (const char*)a.wmix + lane * 16;
                if (st == (last > 0 ? last - 1 : 0))  // slot 1 was last read in stage last-2: free after this barrier
                    for (int j = 0; j < mix1; ++j) glds16(msrc + j * 1024, mixw + j * 1024);
                if (st == last)                       // slot 2 was last read in stage last-1
                    for (int j = mix1; j < a.mix_pieces; ++j) glds16(msrc + j * 1024, mixw + j * 1024);
            }
            sl = sl == 2 ? 0 : sl + 1;
        }
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (FUSE) __builtin_amdgcn_s_barrier();  // the compute waves' barrier between the gate GEMM and the stores
        return;
    }

    // ------------------------- compute waves -------------------------
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = fdiv(mtile, tpi, a.inv_tpi);
    const int trem = mtile - b * tpi;
    const int tyi = fdiv(trem, a.tiles_x, a.inv_tiles_x);
    const int y0 = tyi * G::TH;
    const int x0 = (trem - tyi * a.tiles_x) * G::TW;

    // activation DMA: instruction j covers entries [64 j, 64 j + 64) of the halo image; wave w issues j = w, w+8, w+16
    const long long plane_in = (long long)a.H * a.W * 16;
    long long aoff[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int e = 64 * (w + 8 * i) + lane;
        const int plane = e >= G::PLANE_ENT ? 1 : 0;
        const int p = e - plane * G::PLANE_ENT;
        const int py = p / G::ROWW, px = p - py * G::ROWW;
        const int gy = y0 - 1 + py, gx = x0 - 1 + px;
        const bool ok = (e < G::A_ENT) && (p < G::NPIX) && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        aoff[i] = ok ? ((((long long)b * a.p0 + plane) * a.H + gy) * a.W + gx) * 16 : -1;
    }
    const int nA = (A_INSTR - w + 7) / 8;  // 2 or 3 instructions per stage for this wave
    auto loadA = [&](int st, int slot) {
        const long long kbyte = 2LL * st * plane_in;
        char* dst = smem + slot * SLOT;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (w + 8 * i >= A_INSTR) break;
            const char* src = aoff[i] >= 0 ? (const char*)a.in0 + aoff[i] + kbyte : (const char*)a.zero;
            glds16(src, dst + (w + 8 * i) * 1024);
        }
    };
    int slot = s0;
    int sl2 = s0;
    loadA(0, sl2);
    sl2 = sl2 == 2 ? 0 : sl2 + 1;
    if (nstages > 1) loadA(1, sl2);
    sl2 = sl2 == 2 ? 0 : sl2 + 1;  // slot of stage st + 2

    f32x16 acc[2][NT];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mf][nt][i] = 0.0f;

    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const uint32_t a_lane = lds_base + h * G::PLANE + ((G::ROW_PER_WAVE * w) * G::ROWW + r) * 16;
    const uint32_t b_lane = lds_base + A_SLOT + lane * 16;

    // pixel geometry of this wave's two M fragments
    int ey[2], ex[2];
    if (G::ROW_PER_WAVE == 2) {
        ey[0] = y0 + 2 * w; ey[1] = y0 + 2 * w + 1;
        ex[0] = x0; ex[1] = x0;
    } else {
        ey[0] = y0 + w; ey[1] = y0 + w;
        ex[0] = x0; ex[1] = x0 + 32;
    }
    // FUSE: the block input x as MFMA B fragments, fetched by LDS-DMA into this wave's corner of ring slots 1-2
    const int ncx = FUSE ? a.p1 / 2 : 0;  // K-chunks of x (two planes per chunk)
    const long long plane_x = (long long)a.H * a.W * 16;
    char* const xr = mixw + (FUSE ? a.mix_pieces * 1024 + w * (ncx * 1024) : 0);
    auto pix_ok = [&](int mf) { return ey[mf] < a.H && ex[mf] + r < a.W; };
    auto x_base = [&](int mf) {
        return (const char*)a.in1 + ((((long long)b * a.p1) * a.H + ey[mf]) * a.W + ex[mf] + r) * 16;
    };
    auto x_dma = [&](int mf) {  // entry (chunk c, lane (h, r)) = plane 2c + h of pixel r
        const bool ok = pix_ok(mf);
        const char* xb = x_base(mf);
        for (int c = 0; c < ncx; ++c) glds16(ok ? xb + (2LL * c + h) * plane_x : (const char*)a.zero, xr + c * 1024);
    };

    for (int st = 0; st < nstages; ++st) {
        // my own activation DMA of stage st has landed once at most the newer stage's instructions are pending
        if (st + 1 < nstages) {
            if (nA == 3) wait_vmcnt<3>(); else wait_vmcnt<2>();
        } else {
            wait_vmcnt<0>();
        }
        __builtin_amdgcn_s_barrier();  // stage st is complete in LDS; everyone is done reading stage st-1
        if (st + 2 < nstages) loadA(st + 2, sl2);
        if (FUSE && st == last && a.x_via_lds) x_dma(0);  // slots 1-2 are free from here on; lands under this stage's MFMAs

        const uint32_t a_addr = a_lane + slot * SLOT;
        const uint32_t b_addr = b_lane + slot * SLOT;
        Frags<NT> fa, fb;
        issue_reads<NT, MODE, 0>(fa, a_addr, b_addr);
        wait_frags<NT>(fa);
        run_items<TT, NT, MODE, 0, 9>(acc, fa, fb, a_addr, b_addr);
        slot = slot == 2 ? 0 : slot + 1;
        sl2 = sl2 == 2 ? 0 : sl2 + 1;
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // all fragment reads are done (and, FUSE, the gate weights have landed)

    constexpr int EPW = 32 * (BN * SZ + 16) > 32 * 80 ? 32 * (BN * SZ + 16) : 32 * 80;
    const long long em[2] = {0, 0};

    if (FUSE) {
        // ---- AdaptiveResidualMix in registers: acc = z (conv2 output), x = a.in1 (the block input) ----
        using Z = ZFrag<TT>;
        constexpr int ZG = Z::ZG;
        constexpr int PPU = SZ == 2 ? 8 : 4;
        // Register diet (the 9-wave workgroup caps a wave at 168 VGPRs): z of BOTH fragments is packed to the storage
        // type first (the unfused path rounds z the same way when it stores it), the accumulators die, and each
        // fragment's blended result is packed again until the store phase.
        u32x4 zf[2][NT][ZG];
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g = 0; g < ZG; ++g) {
                    zf[mf][nt][g] = Z::make(acc[mf][nt], g);
                    // opaque: stops hipcc from forwarding pack -> unpack and keeping 96 unpacked floats alive
                    asm volatile("" : "+v"(zf[mf][nt][g]));
                }
        u32x4 res[2][NT][ZG];
#pragma unroll
        for (int mf = 0; mf < 2; ++mf) {
            const bool inside = pix_ok(mf);
            const char* xbase = x_base(mf);
            f32x16 beta[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) beta[nt][i] = 0.0f;
            // gate, z half: accumulator rows are the K index (weights were packed in that row order)
            const char* wz = mixw + ncx * NT * 1024 + lane * 16;
#pragma unroll
            for (int ntz = 0; ntz < NT; ++ntz)
#pragma unroll
                for (int g = 0; g < ZG; ++g) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const u32x4 wv = *(const u32x4*)(wz + ((ntz * ZG + g) * NT + nt) * 1024);
                        mma<TT>(beta[nt], wv, zf[mf][ntz][g]);
                    }
                    __builtin_amdgcn_sched_barrier(0);  // keep hipcc from hoisting every weight fragment read up front
                }
            // gate, x half
            if (a.x_via_lds) {
                if (mf == 1) wait_vmcnt<0>();  // mf 1's fragments were requested after mf 0's blend (below)
                for (int c = 0; c < ncx; ++c) {
                    const u32x4 xf = *(const u32x4*)(xr + c * 1024 + lane * 16);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const u32x4 wv = *(const u32x4*)(mixw + (c * NT + nt) * 1024 + lane * 16);
                        mma<TT>(beta[nt], wv, xf);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                for (int c0 = 0; c0 < ncx; c0 += 2) {  // straight from HBM, two K-chunks in flight (register budget)
                    u32x4 xf[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        xf[i] = u32x4{0u, 0u, 0u, 0u};
                        if (inside && c0 + i < ncx) xf[i] = *(const u32x4*)(xbase + (2LL * (c0 + i) + h) * plane_x);
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (c0 + i < ncx) {
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt) {
                                const u32x4 wv = *(const u32x4*)(mixw + ((c0 + i) * NT + nt) * 1024 + lane * 16);
                                mma<TT>(beta[nt], wv, xf[i]);
                            }
                        }
                    }
                }
            }
            // blend: out = x + sigmoid(alpha) * sigmoid(beta) * (z - x), in place, one quad at a time
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float xv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4];
                    Z::quad(zf[mf][nt], q, zv);
                    const int n = 32 * nt + 8 * q + 4 * h;
                    if (a.x_via_lds) {
                        // channels n..n+3 of pixel r sit in chunk n / CK, plane (n / PPU) & 1 of the fragment image
                        const int plane = n / PPU, inner = (n - plane * PPU) * SZ;
                        if (plane < a.p1) ld4<TT>(xr + (plane >> 1) * 1024 + ((plane & 1) * 32 + r) * 16 + inner, xv);
                    } else if (inside && n < a.cp_out) {
                        const int plane = n / PPU, inner = (n - plane * PPU) * SZ;
                        ld4<TT>(xbase + plane * plane_x + inner, xv);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        beta[nt][4 * q + j] = blend_(xv[j], zv[j], beta[nt][4 * q + j], a.inv_mix_scale);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int g = 0; g < ZG; ++g) {
                    res[mf][nt][g] = Z::make(beta[nt], g);
                    asm volatile("" : "+v"(res[mf][nt][g]));
                }
            }
            if (a.x_via_lds && mf == 0) {
                __builtin_amdgcn_wave_barrier();
                x_dma(1);  // overlaps mf 1's z-half MFMAs
            }
        }
        // unpack the (already rounded) results back into the accumulator registers for the common store path
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[4];
                    Z::quad(res[mf][nt], q, v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mf][nt][4 * q + j] = v[j];
                }
        __builtin_amdgcn_s_barrier();  // every wave is done with the gate weights: the ring can take epilogue data
        conv_epilogue<TT, NT, true>(a, EPI_STORE, 0, acc, smem + w * EPW, smem + 8 * EPW + w * kFinalWinBytes, lane, nbase, b, ey, ex, em);
    } else {
        conv_epilogue<TT, NT, true, VIEW>(a, a.epi, a.silu, acc, smem + w * EPW, smem + 8 * EPW + w * kFinalWinBytes, lane, nbase, b, ey, ex, em);
    }
}

// ================================================================================================
// 3x3 convolution, wide tile, PERSISTENT: one workgroup per CU walks its XCD's share of the tile list, and the
// LDS ring simply keeps turning across tile boundaries.  Two loader waves issue every LDS-DMA (wave 8 the halo
// images, wave 9 the weight stages), two K-stages ahead of the compute waves -- also across a tile boundary, so
// the first two stages of the next tile land while this tile's last stages and its epilogue run.  The compute
// waves issue no loads at all: they never wait on vmcnt, so the epilogue's stores drain under the next tile's
// MFMAs instead of at the end of a workgroup's life.  (Store epilogues only: STORE / D2S need no LDS.)
// ================================================================================================
template <class TT, int NT, int MODE>
__global__ __launch_bounds__(640) void conv3p_kernel(const ConvArgs a) {
    using G = Geo<MODE>;
    constexpr int A_SLOT = G::A_ENT * 16;
    constexpr int A_INSTR = G::A_ENT / 64;
    constexpr int B_PIECES = 9 * NT;
    constexpr int B_SLOT = B_PIECES * 1024;
    constexpr int SLOT = A_SLOT + B_SLOT;
    constexpr int BN = 32 * NT;
    static_assert(2 * B_PIECES < 64 && 2 * A_INSTR < 64, "vmcnt is a 6-bit counter");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7 compute, 8 = halo loader, 9 = weight loader
    const int nstages = a.nchunks;

    // this workgroup's tile list: logical ids base + pos, base + pos + step, ... inside its XCD's contiguous range
    const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3, step = gridDim.x >> 3;
    const int q = a.grid >> 3, rem = a.grid & 7;
    const int cnt = q + (xcd < rem ? 1 : 0);
    const int base = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
    // first valid (non-padding) tile at or after list position i; cnt when the list is exhausted
    auto seek = [&](int i, int& mtile, int& ntile) __attribute__((always_inline)) {
        while (i < cnt && !tile_of(a, base + i, mtile, ntile)) i += step;
        return i;
    };
    int mtile = 0, ntile = 0;
    int cur = seek(pos, mtile, ntile);
    if (cur >= cnt) return;  // uniform over the workgroup

    const int tpi = a.tiles_x * a.tiles_y;
    auto tile_origin = [&](int mt, int& b, int& y0, int& x0) __attribute__((always_inline)) {
        b = fdiv(mt, tpi, a.inv_tpi);
        const int trem = mt - b * tpi;
        const int tyi = fdiv(trem, a.tiles_x, a.inv_tiles_x);
        y0 = tyi * G::TH;
        x0 = (trem - tyi * a.tiles_x) * G::TW;
    };

    if (w >= 8) {
        // ------------------------- loader waves -------------------------
        // how many stages this workgroup will run in total (the compute waves meet us at one barrier per stage)
        int ntl = 0;
        {
            int mt_, nt_;
            for (int i = cur; i < cnt; i = seek(i + step, mt_, nt_)) ++ntl;
        }
        const int total = ntl * nstages;
        const long long plane_in = (long long)a.H * a.W * 16;
        int l_pos = cur, l_st = 0, l_slot = 0, pending = 0;
        bool l_ok = true;
        if (w == 9) {
            const char* wsrc = (const char*)a.wpk + (size_t)ntile * nstages * B_SLOT + lane * 16;
            auto issue = [&]() __attribute__((always_inline)) {
                if (!l_ok) return;
                const char* src = wsrc + (size_t)l_st * B_SLOT;
                char* dst = smem + l_slot * SLOT + A_SLOT;
#pragma unroll
                for (int j = 0; j < B_PIECES; ++j) glds16(src + j * 1024, dst + j * 1024);
                ++pending;
                l_slot = l_slot == 2 ? 0 : l_slot + 1;
                if (++l_st == nstages) {
                    l_st = 0;
                    int mt_, nt_ = 0;
                    l_pos = seek(l_pos + step, mt_, nt_);
                    l_ok = l_pos < cnt;
                    wsrc = (const char*)a.wpk + (size_t)nt_ * nstages * B_SLOT + lane * 16;
                }
            };
            issue();
            issue();
            for (int g = 0; g < total; ++g) {
                if (pending >= 2) wait_vmcnt<B_PIECES>(); else wait_vmcnt<0>();
                --pending;
                __builtin_amdgcn_s_barrier();
                issue();
            }
        } else {
            // halo image: instruction j covers entries [64 j, 64 j + 64); per-lane byte offsets inside image b
            uint32_t aoff[A_INSTR];
            const char* img = nullptr;
            auto set_tile = [&](int mt) __attribute__((always_inline)) {
                int b, y0, x0;
                tile_origin(mt, b, y0, x0);
                img = (const char*)a.in0 + (long long)b * a.p0 * plane_in;
#pragma unroll
                for (int j = 0; j < A_INSTR; ++j) {
                    const int e = 64 * j + lane;
                    const int plane = e >= G::PLANE_ENT ? 1 : 0;
                    const int p = e - plane * G::PLANE_ENT;
                    const int py = p / G::ROWW, px = p - py * G::ROWW;
                    const int gy = y0 - 1 + py, gx = x0 - 1 + px;
                    const bool ok = (p < G::NPIX) && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
                    aoff[j] = ok ? (((uint32_t)plane * (uint32_t)a.H + (uint32_t)gy) * (uint32_t)a.W + (uint32_t)gx) * 16u : 0xffffffffu;  // host: planes * H * W * 16 < 2^32
                }
            };
            set_tile(mtile);
            auto issue = [&]() __attribute__((always_inline)) {
                if (!l_ok) return;
                const char* src = img + 2LL * l_st * plane_in;
                char* dst = smem + l_slot * SLOT;
#pragma unroll
                for (int j = 0; j < A_INSTR; ++j)
                    glds16(aoff[j] != 0xffffffffu ? src + aoff[j] : (const char*)a.zero, dst + j * 1024);
                ++pending;
                l_slot = l_slot == 2 ? 0 : l_slot + 1;
                if (++l_st == nstages) {
                    l_st = 0;
                    int mt_ = 0, nt_;
                    l_pos = seek(l_pos + step, mt_, nt_);
                    l_ok = l_pos < cnt;
                    if (l_ok) set_tile(mt_);
                }
            };
            issue();
            issue();
            for (int g = 0; g < total; ++g) {
                if (pending >= 2) wait_vmcnt<A_INSTR>(); else wait_vmcnt<0>();
                --pending;
                __builtin_amdgcn_s_barrier();
                issue();
            }
        }
        return;
    }

    // ------------------------- compute waves -------------------------
    const int h = lane >> 5, r = lane & 31;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const uint32_t a_lane = lds_base + h * G::PLANE + ((G::ROW_PER_WAVE * w) * G::ROWW + r) * 16;
    const uint32_t b_lane = lds_base + A_SLOT + lane * 16;
    const long long em[2] = {0, 0};
    int slot = 0;
    while (cur < cnt) {
        int b, y0, x0;
        tile_origin(mtile, b, y0, x0);
        const int nbase = ntile * BN;
        int ey[2], ex[2];
        if (G::ROW_PER_WAVE == 2) {
            ey[0] = y0 + 2 * w; ey[1] = y0 + 2 * w + 1;
            ex[0] = x0; ex[1] = x0;
        } else {
            ey[0] = y0 + w; ey[1] = y0 + w;
            ex[0] = x0; ex[1] = x0 + 32;
        }
        f32x16 acc[2][NT];
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mf][nt][i] = 0.0f;

        for (int st = 0; st < nstages; ++st) {
            __builtin_amdgcn_s_barrier();  // stage landed (the loaders waited for it); everyone is done with the slot two back
            const uint32_t a_addr = a_lane + slot * SLOT;
            const uint32_t b_addr = b_lane + slot * SLOT;
            Frags<NT> fa, fb;
            issue_reads<NT, MODE, 0>(fa, a_addr, b_addr);
            wait_frags<NT>(fa);
            run_items<TT, NT, MODE, 0, 9>(acc, fa, fb, a_addr, b_addr);
            slot = slot == 2 ? 0 : slot + 1;
        }
        if (a.epi == EPI_D2S) store_epilogue<TT, NT, true, EPI_D2S, false>(a, acc, lane, nbase, b, ey, ex, em);
        else if (a.silu) store_epilogue<TT, NT, true, EPI_STORE, true>(a, acc, lane, nbase, b, ey, ex, em);
        else store_epilogue<TT, NT, true, EPI_STORE, false>(a, acc, lane, nbase, b, ey, ex, em);
        cur = seek(cur + step, mtile, ntile);
    }
}

}  // namespace mz
