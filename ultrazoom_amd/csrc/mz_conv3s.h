// conv3s_kernel: persistent 3x3 convolution on 512-pixel tiles with the 16x16x32 MFMA, 16-bit types (launcher: mz_conv3s.hip).
#pragma once
#include "mz_device.h"
#include "mz_geo.h"

namespace mz {

// ================================================================================================
// 3x3 convolution on v_mfma_f32_16x16x32_{bf16,f16}, persistent (16-bit types only).
// Why a second MFMA shape: the chip is power-limited in this loop and holds a visibly higher clock
// on the 16x16x32 shape than on 32x32x16 at identical FLOPs, LDS bytes and staging traffic.
//   * K-step of one MFMA = 32 channels = FOUR 16-byte planes: lane (g, c) = (lane >> 4, lane & 15) supplies plane g
//     of pixel c (B operand) / of output channel c (A operand); it receives channels 4g..4g+3 of pixel c.
//   * wave tile as before: 64 pixels x BN channels = 4 pixel fragments x 2*NT channel fragments (96 accumulator regs).
//   * a 32-channel K-stage with all 9 taps would need 94 KB per ring slot, so the two operands turn on separate
//     rings: the halo image (4 planes, 40 KB) is double-buffered per 32-channel chunk, the weights stream in
//     tap-ROW sub-stages (3 taps x 2*NT fragments = 18 KB) through 3 slots; one barrier per sub-stage.  With three
//     sub-stages per chunk the weight slot of a sub-stage is simply its tap row.
//   * loaders / persistence / tile walk exactly as conv3p_kernel.
//   * inside a sub-stage the fragments are software-pipelined per GROUP of 8 MFMAs (two channel fragments x four
//     pixel fragments): the next group's 2 weight fragments and a share of the next tap's 4 pixel fragments are
//     requested in the shadow of the group's first MFMAs.
// ================================================================================================
struct Frag16 {
    u32x4 x[2][4];  // [tap parity][pixel fragment]
    u32x4 w[3][2];  // [group % 3][channel fragment of the group]: requested TWO groups ahead
};
// wait_w16 (mz_device.h) that also names the four pixel fragments of the next tap
template <int N> __device__ __forceinline__ void wait_wx16(u32x4& w0, u32x4& w1, u32x4& x0, u32x4& x1, u32x4& x2, u32x4& x3) {
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(w0), "+v"(w1), "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3) : "n"(N) : "memory");
}
// byte offset of pixel fragment pf of tap (dy, dx) inside one plane of the halo image, relative to the wave's first row
template <int MODE, int TAP, int PF> constexpr int s16_a_off() {
    using G = Geo<MODE>;
    constexpr int DY = TAP / 3, DX = TAP % 3;
    return G::ROW_PER_WAVE == 2 ? ((DY + (PF >> 1)) * G::ROWW + DX + 16 * (PF & 1)) * 16 : (DY * G::ROWW + DX + 16 * PF) * 16;
}
// A 32-channel chunk = 9 * NT GROUPS; group G = (tap G / NT, channel-fragment pair G % NT) = 8 MFMAs, its two weight
// fragments are pieces 2G, 2G+1 of the chunk's packed weights.  The chunk's weights arrive in two halves (groups
// [0, G0) and [G0, NG), one LDS slot each), so there are two barriers per chunk -- the cadence of the 32x32x16
// kernel's two 16-channel stages.
// While group G runs it requests the weight pair of group G + 2 (inside the same half) and its share of the NEXT
// tap's pixel fragments (NT = 3: two each in the tap's groups 0 and 1; NT = 2: all four in group 0; NT = 1: all
// four, one group ahead).  Tap t uses pixel buffer t & 1; pixel fragments are prefetched across the mid-chunk barrier
// (the halo image does not change there), weight fragments are not (the second half has just landed).
template <int NT> struct S16Geo {
    static constexpr int NG = 9 * NT;
    static constexpr int G0 = (NG + 1) / 2;
    static constexpr int B_SLOT = 2 * G0 * 1024;
    // LDS byte offset of weight piece k of group G, relative to the weight area
    static constexpr int w_off(int G, int k) { return G < G0 ? (2 * G + k) * 1024 : B_SLOT + (2 * (G - G0) + k) * 1024; }
};
template <int NT, int G, int GE> struct S16Plan {  // group G of the segment ending at GE
    static constexpr int t = G / NT, n = G % NT;
    static constexpr bool w_issue = G + 2 < GE;
    // (requesting all four in the tap's first group keeps them live a group longer: 30 spilled VGPRs, +12 % time)
    static constexpr int x_count = t + 1 < 9 ? (NT == 3 ? (n < 2 ? 2 : 0) : (n == 0 ? 4 : 0)) : 0;
    static constexpr int x_first = NT == 3 ? 2 * n : 0;
    static constexpr int issued = (w_issue ? 2 : 0) + x_count;  // reads requested during this group
    // everything requested BEFORE this group has landed once at most `issued` reads are outstanding; NT = 1 needs the
    // pixel fragments it has just requested right away
    static constexpr int allow = NT == 1 ? (w_issue ? 2 : 0) : issued;
};
template <class TT, int NT, int MODE, int G, int GE, int M>
__device__ __forceinline__ void s16_mfmas(f32x4 (&acc)[4][2 * NT], Frag16& f, uint32_t a_addr, uint32_t b_addr) {
    if constexpr (M < 8) {
        using P = S16Plan<NT, G, GE>;
        constexpr int t = P::t, n = P::n, xp = t & 1, wp = G % 3;
        // pixel-fragment major, the channel pair in serpentine order, odd pairs of a tap walk the pixel fragments backwards: one operand
        // changes per MFMA (conv3r_kernel's order, DESIGN.md 5.2c: the same sums at a higher clock)
        constexpr int pf = (n & 1) ? 3 - (M >> 1) : (M >> 1), k = ((M >> 1) & 1) ? 1 - (M & 1) : (M & 1);
        mma16<TT>(acc[pf][2 * n + k], f.w[wp][k], f.x[xp][pf]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (P::w_issue && M < 2) {
            f.w[(G + 2) % 3][M] = lds_read128<S16Geo<NT>::w_off(G + 2, M)>(b_addr);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (M >= 2 && M - 2 < P::x_count) {
            constexpr int pfn = P::x_first + M - 2;
            f.x[xp ^ 1][pfn] = lds_read128<s16_a_off<MODE, t + 1, pfn>()>(a_addr);
            __builtin_amdgcn_sched_barrier(0);
        }
        s16_mfmas<TT, NT, MODE, G, GE, M + 1>(acc, f, a_addr, b_addr);
    }
}
template <class TT, int NT, int MODE, int G, int GE>
__device__ __forceinline__ void s16_groups(f32x4 (&acc)[4][2 * NT], Frag16& f, uint32_t a_addr, uint32_t b_addr) {
    if constexpr (G < GE) {
        using P = S16Plan<NT, G, GE>;
        __builtin_amdgcn_sched_barrier(0);
        s16_mfmas<TT, NT, MODE, G, GE, 0>(acc, f, a_addr, b_addr);
        if constexpr (G + 1 < GE) {
            constexpr int wn = (G + 1) % 3, xn = ((G + 1) / NT) & 1;
            if constexpr ((G + 1) % NT == 0)  // the next group starts a new tap: its pixel fragments must be in
                wait_wx16<P::allow>(f.w[wn][0], f.w[wn][1], f.x[xn][0], f.x[xn][1], f.x[xn][2], f.x[xn][3]);
            else
                wait_w16<P::allow>(f.w[wn][0], f.w[wn][1]);
        }
        s16_groups<TT, NT, MODE, G + 1, GE>(acc, f, a_addr, b_addr);
    }
}
// first half of a chunk: a new halo image and the first weight half have just been published by the barrier
template <class TT, int NT, int MODE>
__device__ __forceinline__ void s16_front(f32x4 (&acc)[4][2 * NT], Frag16& f, uint32_t a_addr, uint32_t b_addr) {
    using S = S16Geo<NT>;
    f.x[0][0] = lds_read128<s16_a_off<MODE, 0, 0>()>(a_addr);
    f.x[0][1] = lds_read128<s16_a_off<MODE, 0, 1>()>(a_addr);
    f.x[0][2] = lds_read128<s16_a_off<MODE, 0, 2>()>(a_addr);
    f.x[0][3] = lds_read128<s16_a_off<MODE, 0, 3>()>(a_addr);
    f.w[0][0] = lds_read128<S::w_off(0, 0)>(b_addr);
    f.w[0][1] = lds_read128<S::w_off(0, 1)>(b_addr);
    f.w[1][0] = lds_read128<S::w_off(1, 0)>(b_addr);
    f.w[1][1] = lds_read128<S::w_off(1, 1)>(b_addr);
    wait_wx16<2>(f.w[0][0], f.w[0][1], f.x[0][0], f.x[0][1], f.x[0][2], f.x[0][3]);
    s16_groups<TT, NT, MODE, 0, S::G0>(acc, f, a_addr, b_addr);
}
// second half: only the weights are new; pixel fragments requested before the barrier are simply older in the queue
template <class TT, int NT, int MODE>
__device__ __forceinline__ void s16_back(f32x4 (&acc)[4][2 * NT], Frag16& f, uint32_t a_addr, uint32_t b_addr) {
    using S = S16Geo<NT>;
    constexpr int G0 = S::G0, w0 = G0 % 3, w1 = (G0 + 1) % 3, xn = (G0 / NT) & 1;
    f.w[w0][0] = lds_read128<S::w_off(G0, 0)>(b_addr);
    f.w[w0][1] = lds_read128<S::w_off(G0, 1)>(b_addr);
    f.w[w1][0] = lds_read128<S::w_off(G0 + 1, 0)>(b_addr);
    f.w[w1][1] = lds_read128<S::w_off(G0 + 1, 1)>(b_addr);
    wait_wx16<2>(f.w[w0][0], f.w[w0][1], f.x[xn][0], f.x[xn][1], f.x[xn][2], f.x[xn][3]);
    s16_groups<TT, NT, MODE, G0, S::NG>(acc, f, a_addr, b_addr);
}

// accumulators -> plane-major tensor.  Lane (g, c) holds channels 4g..4g+3 of pixel c of each 16-channel fragment;
// v_permlane16_swap between the two fragments of a group leaves lane g with one full 16-byte plane entry:
// fragment (g & 1) of the pair, plane (g >> 1) of that fragment.
// FILM (NO reference counterpart in the snapshot): a per-image, per-channel affine gamma * y + beta on the
// convolution result, ahead of the optional SiLU -- the shape of a FiLM / control-module modulation.
template <class TT, int NT, int MODE, int EPI, bool SILU, bool FILM = false>
__device__ __forceinline__ void store_frag16(const ConvArgs& a, f32x4 (&accpf)[2 * NT], const int pf, int lane, int w, int nbase,
                                             int b, int y0, int x0) {
    using G = Geo<MODE>;
    constexpr bool d2s = EPI == EPI_D2S;
    const int g = lane >> 4, c = lane & 15;
    const long long plane_o = d2s ? (long long)a.Hout * a.Wout * 16 : (long long)a.H * a.W * 16;
    char* const obase = (char*)a.out + (long long)b * a.p_out * plane_o;
    const int py = G::ROW_PER_WAVE == 2 ? y0 + 2 * w + (pf >> 1) : y0 + w;
    const int px = G::ROW_PER_WAVE == 2 ? x0 + 16 * (pf & 1) + c : x0 + 16 * pf + c;
    const bool inside = py < a.H && px < a.W;
    const int lane_cu = 2 * (g & 1) + (g >> 1);  // 16-byte unit of the lane inside a channel-fragment pair's 4 planes
    if constexpr (!d2s && !FILM) {
        // one 64-bit base per pixel fragment, then a uniform stride of four planes per pair (entry16(): mz_device.h)
        char* dst = obase + (long long)((nbase >> 3) + lane_cu) * plane_o + ((long long)py * a.W + px) * 16;
        const long long stride = 4 * plane_o;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const u32x4 o = entry16<TT, SILU>(accpf[2 * n], accpf[2 * n + 1]);
            const int nch = nbase + (4 * n + lane_cu) * 8;
            if (inside && nch < a.cp_out) *(u32x4*)dst = o;
            dst += stride;
        }
        return;
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ea = accpf[2 * n][j], eb = accpf[2 * n + 1][j];
            const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, ea), __builtin_bit_cast(uint32_t, eb),
                                                             false, false);
            const uint32_t s0 = sw[0], s1 = sw[1];
            v[j] = __builtin_bit_cast(float, s0);
            v[4 + j] = __builtin_bit_cast(float, s1);
        }
        const int nch = nbase + (4 * n + lane_cu) * 8;
        if constexpr (SILU && !FILM) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * sigmoidf_(v[j]);
        }
        if (!inside) continue;
        char* dst;
        if constexpr (d2s) {
            if (nch >= 4 * a.cp_out) continue;
            const int ij = nch / a.cp_out;
            const int ch = nch - ij * a.cp_out;
            const int Y = 2 * py + (ij >> 1), X = 2 * px + (ij & 1);
            dst = obase + (ch >> 3) * plane_o + ((long long)Y * a.Wout + X) * 16;
        } else {
            if (nch >= a.cp_out) continue;
            dst = obase + (nch >> 3) * plane_o + ((long long)py * a.W + px) * 16;
        }
        if constexpr (FILM) {  // gamma / beta: float [B][cp_out], pad channels zero (the host pads them)
            const float4* gp = (const float4*)(a.film_gamma + (long long)b * a.cp_out + nch);
            const float4* bp = (const float4*)(a.film_beta + (long long)b * a.cp_out + nch);
            const float4 g0 = gp[0], g1 = gp[1], b0 = bp[0], b1 = bp[1];
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[j] = gg[j] * v[j] + bb[j];
                if constexpr (SILU) v[j] = v[j] * sigmoidf_(v[j]);
            }
        }
        st_unit<TT>(dst, v);
    }
}
template <class TT, int NT, int MODE, int EPI, bool SILU, bool FILM = false>
__device__ __forceinline__ void store_epilogue16(const ConvArgs& a, f32x4 (&acc)[4][2 * NT], int lane, int w, int nbase, int b,
                                                 int y0, int x0) {
#pragma unroll
    for (int pf = 0; pf < 4; ++pf) store_frag16<TT, NT, MODE, EPI, SILU, FILM>(a, acc[pf], pf, lane, w, nbase, b, y0, x0);
}

// gate GEMM of the fused mix on the 16x16 layout: 2 NT K-steps of NF = 2 NT weight fragments each, walked in HALF
// steps of NT fragments: the next half step's fragments are requested before the current one's MFMAs are issued
// (LDS reads return in order: lgkmcnt(NT) = "everything but the NT reads just requested has landed").
template <int NT, int H, int I> __device__ __forceinline__ void gate_reads(u32x4 (&wv)[NT], uint32_t addr) {
    if constexpr (I < NT) {
        constexpr int ks = H >> 1, part = H & 1;
        wv[I] = lds_read128<(ks * 2 * NT + part * NT + I) * 1024>(addr);
        gate_reads<NT, H, I + 1>(wv, addr);
    }
}
template <int NT, int N> __device__ __forceinline__ void gate_wait(u32x4 (&wv)[NT]) {
    if constexpr (NT == 1) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(wv[0]) : "n"(N) : "memory");
    else if constexpr (NT == 2) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(wv[0]), "+v"(wv[1]) : "n"(N) : "memory");
    else asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(wv[0]), "+v"(wv[1]), "+v"(wv[2]) : "n"(N) : "memory");
}
template <class TT, int NT, int H>
__device__ __forceinline__ void gate_halves(f32x4 (&beta)[2 * NT], const u32x4 (&xf)[NT], const u32x4 (&zf)[NT], u32x4 (&wa)[NT],
                                            u32x4 (&wb)[NT], uint32_t addr) {
    if constexpr (H < 4 * NT) {
        constexpr int ks = H >> 1, part = H & 1;
        constexpr bool more = H + 1 < 4 * NT;
        if constexpr (more) gate_reads<NT, H + 1, 0>(wb, addr);  // wa = this half step's fragments, wb = the next one's
        gate_wait<NT, (more ? NT : 0)>(wa);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if constexpr (ks < NT) mma16<TT>(beta[part * NT + i], wa[i], xf[ks]);
            else mma16<TT>(beta[part * NT + i], wa[i], zf[ks - NT]);
        }
        __builtin_amdgcn_sched_barrier(0);
        gate_halves<TT, NT, H + 1>(beta, xf, zf, wb, wa, addr);
    }
}

// FUSE: conv2 + AdaptiveResidualMix (model.py:826-839) in one pass, as in conv3w_kernel<.., FUSE> but on the 16x16
// accumulator layout: after the K loop the wave packs z into MFMA B operands (two 16-channel accumulator fragments =
// one 32-wide K step; the gate weights were packed in that order, PK_GATE16), two extra barriers let the
// weight loader drop the 4 NT^2 KB of gate weights into the second weight slot (+ the LDS behind it) once every wave
// has left the K loop, x arrives as plain 16-byte loads (the plane-major layout IS the B-operand layout), and the
// blend x + sigmoid(alpha) sigmoid(beta) (z - x) runs in the accumulator registers before the common store.
template <class TT, int NT, int MODE, bool FUSE>
__global__ __launch_bounds__(640) void conv3s_kernel(const ConvArgs a) {
    using G = Geo<MODE>;
    constexpr int NF = 2 * NT;
    constexpr int MIX_PIECES = 4 * NT * NT;  // FUSE: gate weights = 2 NT K-steps x NF fragments of 1 KiB
    constexpr int BN = 32 * NT;
    constexpr int A_PLANE = G::PLANE;
    constexpr int A_SLOT = 4 * A_PLANE;
    constexpr int A_INSTR = 4 * G::PLANE_ENT / 64;
    using SG = S16Geo<NT>;
    constexpr int P0 = 2 * SG::G0, P1 = 2 * (SG::NG - SG::G0);  // DMA pieces of the two weight halves of a chunk
    constexpr int B_SLOT = SG::B_SLOT;
    constexpr int B_BASE = 2 * A_SLOT;  // LDS: [halo 0][halo 1][weights: first half][weights: second half]
    static_assert(P0 < 64 && A_INSTR < 64, "vmcnt is a 6-bit counter");
    static_assert((4 * G::PLANE_ENT) % 64 == 0, "halo image = whole DMA instructions");
    static_assert(2 * B_SLOT < 65536, "ds offset is 16 bits");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7 compute, 8 = halo loader, 9 = weight loader
    const int nchunks = a.nchunks16;                          // 32-channel chunks

    const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3, step = gridDim.x >> 3;
    const int q = a.grid >> 3, rem = a.grid & 7;
    const int cnt = q + (xcd < rem ? 1 : 0);
    const int base = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
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
        int tyi, txi;
        tile_rc(a, trem, tyi, txi);
        y0 = tyi * G::TH;
        x0 = txi * G::TW;
    };

    if (w >= 8) {
        int ntl = 0;
        {
            int mt_, nt_;
            for (int i = cur; i < cnt; i = seek(i + step, mt_, nt_)) ++ntl;
        }
        int l_pos = cur;
        bool l_ok = true;
        if (w == 9) {
            // ---- weight loader: the two halves of each chunk, one half ahead (two slots: half u + 1 goes where half
            //      u - 1 was, once everyone has passed barrier u) ----
            const size_t chunk_bytes = (size_t)(P0 + P1) * 1024;
            const char* wsrc = (const char*)a.wpk16 + (size_t)ntile * nchunks * chunk_bytes + lane * 16;
            int l_kc = 0, l_half = 0;
            auto issue = [&]() __attribute__((always_inline)) {
                if (!l_ok) return;
                const char* src = wsrc + (size_t)l_kc * chunk_bytes;
                if (l_half == 0) {
#pragma unroll
                    for (int j = 0; j < P0; ++j) glds16(src + j * 1024, smem + B_BASE + j * 1024);
                    l_half = 1;
                } else {
#pragma unroll
                    for (int j = 0; j < P1; ++j) glds16(src + (P0 + j) * 1024, smem + B_BASE + B_SLOT + j * 1024);
                    l_half = 0;
                    if (++l_kc == nchunks) {
                        l_kc = 0;
                        int mt_, nt_ = 0;
                        l_pos = seek(l_pos + step, mt_, nt_);
                        l_ok = l_pos < cnt;
                        wsrc = (const char*)a.wpk16 + (size_t)nt_ * nchunks * chunk_bytes + lane * 16;
                    }
                }
            };
            issue();
            int u = 0;
            for (int t = 0; t < ntl; ++t) {
                for (int hh = 0; hh < 2 * nchunks; ++hh, ++u) {
                    wait_vmcnt<0>();
                    __builtin_amdgcn_s_barrier();
                    issue();
                }
                if constexpr (FUSE) {
                    __builtin_amdgcn_s_barrier();  // E1: every wave has left the K loop: the second weight slot is free
                    const char* msrc = (const char*)a.wmix16 + lane * 16;
                    char* mdst = smem + B_BASE + B_SLOT;
#pragma unroll
                    for (int j = 0; j < MIX_PIECES; ++j) glds16(msrc + j * 1024, mdst + j * 1024);
                    wait_vmcnt<0>();
                    __builtin_amdgcn_s_barrier();  // E2: the gate weights have landed
                }
            }
        } else {
            // ---- halo loader: one 4-plane image per 32-channel chunk, one chunk ahead.  Buffer-addressed LDS-DMA: the
            //      descriptor covers exactly the planes of this chunk that exist (2 or 4), so halo pixels outside the
            //      image (offset 0xffffffff) and the missing planes of a half chunk read as zeros by the hardware's
            //      range check -- no zero page, no per-lane 64-bit address arithmetic in the issue loop ----
            const long long plane_in = (long long)a.H * a.W * 16;
            uint32_t aoff[A_INSTR];
            const char* img = nullptr;
            auto set_tile = [&](int mt) __attribute__((always_inline)) {
                int b, y0, x0;
                tile_origin(mt, b, y0, x0);
                img = (const char*)a.in0 + (long long)b * a.p0 * plane_in;
#pragma unroll
                for (int j = 0; j < A_INSTR; ++j) {
                    const int e = 64 * j + lane;
                    const int plane = e / G::PLANE_ENT;
                    const int p = e - plane * G::PLANE_ENT;
                    const int py = p / G::ROWW, px = p - py * G::ROWW;
                    const int gy = y0 - 1 + py, gx = x0 - 1 + px;
                    const bool ok = (p < G::NPIX) && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
                    aoff[j] = ok ? (((uint32_t)plane * (uint32_t)a.H + (uint32_t)gy) * (uint32_t)a.W + (uint32_t)gx) * 16u : 0xffffffffu;  // host: planes * H * W * 16 < 2^32
                }
            };
            set_tile(mtile);
            int l_kc = 0, l_slot = 0;
            auto issue = [&]() __attribute__((always_inline)) {
                if (!l_ok) return;
                const int planes = a.p0 - 4 * l_kc < 4 ? a.p0 - 4 * l_kc : 4;
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(img + 4LL * l_kc * plane_in), 0, (int)(uint32_t)(planes * plane_in), 0x00020000);
                char* dst = smem + l_slot * A_SLOT;
#pragma unroll
                for (int j = 0; j < A_INSTR; ++j)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(dst + j * 1024), 16,
                                                             (int)aoff[j], 0, 0, 0);
                l_slot ^= 1;
                if (++l_kc == nchunks) {
                    l_kc = 0;
                    int mt_ = 0, nt_;
                    l_pos = seek(l_pos + step, mt_, nt_);
                    l_ok = l_pos < cnt;
                    if (l_ok) set_tile(mt_);
                }
            };
            issue();
            int u = 0;
            for (int t = 0; t < ntl; ++t) {
                for (int hh = 0; hh < 2 * nchunks; ++hh, ++u) {
                    if ((hh & 1) == 0) wait_vmcnt<0>();  // a chunk's first barrier publishes its halo image
                    __builtin_amdgcn_s_barrier();
                    if ((hh & 1) == 0) issue();          // chunk c + 1 -> the slot chunk c - 1 was read from
                }
                if constexpr (FUSE) {
                    __builtin_amdgcn_s_barrier();  // E1
                    __builtin_amdgcn_s_barrier();  // E2
                }
            }
        }
        return;
    }

    // ------------------------- compute waves -------------------------
    const int g = lane >> 4, c = lane & 15;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const uint32_t a_lane = lds_base + g * A_PLANE + ((G::ROW_PER_WAVE * w) * G::ROWW + c) * 16;
    const uint32_t b_lane = lds_base + B_BASE + lane * 16;
    uint32_t a_cur = a_lane, a_oth = a_lane + A_SLOT;  // this lane's address in the current / the other halo image
    Frag16 f;
    while (cur < cnt) {
        int b, y0, x0;
        tile_origin(mtile, b, y0, x0);
        f32x4 acc[4][NF];
#pragma unroll
        for (int pf = 0; pf < 4; ++pf)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) acc[pf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < nchunks; ++kc) {
            __builtin_amdgcn_s_barrier();
            s16_front<TT, NT, MODE>(acc, f, a_cur, b_lane);
            __builtin_amdgcn_s_barrier();
            s16_back<TT, NT, MODE>(acc, f, a_cur, b_lane);
            const uint32_t tmp = a_cur; a_cur = a_oth; a_oth = tmp;
        }
        const int nbase = ntile * BN;
        if constexpr (FUSE) {
            // ---- AdaptiveResidualMix in registers: acc = z (conv2 output), x = a.in1 (the block input) ----
            u32x4 zb[4][NT];  // z as B operands: K step m = accumulator fragments 2m, 2m+1 (rounded to the storage type)
#pragma unroll
            for (int pf = 0; pf < 4; ++pf)
#pragma unroll
                for (int m = 0; m < NT; ++m) {
                    const f32x4 za = acc[pf][2 * m], zc = acc[pf][2 * m + 1];
                    u32x4 t;
                    t[0] = pack2<TT>(za[0], za[1]); t[1] = pack2<TT>(za[2], za[3]);
                    t[2] = pack2<TT>(zc[0], zc[1]); t[3] = pack2<TT>(zc[2], zc[3]);
                    asm volatile("" : "+v"(t));  // opaque: no pack -> unpack forwarding that would keep 96 floats alive
                    zb[pf][m] = t;
                }
            const long long hw = (long long)a.H * a.W;
            const char* const xim = (const char*)a.in1 + (long long)b * a.p1 * hw * 16;
            const uint32_t mix_lane = lds_base + B_BASE + B_SLOT + lane * 16;
            // x as B operands (plane 4 kc + g of the lane's pixel): requested one pixel fragment ahead of its use
            auto x_ptr = [&](int pf, bool& inside) __attribute__((always_inline)) {
                const int py = G::ROW_PER_WAVE == 2 ? y0 + 2 * w + (pf >> 1) : y0 + w;
                const int px = G::ROW_PER_WAVE == 2 ? x0 + 16 * (pf & 1) + c : x0 + 16 * pf + c;
                inside = py < a.H && px < a.W;
                return xim + ((long long)py * a.W + px) * 16;
            };
            auto load_xf = [&](int pf, u32x4 (&xf)[NT]) __attribute__((always_inline)) {
                bool inside;
                const char* const xp = x_ptr(pf, inside);
#pragma unroll
                for (int kc = 0; kc < NT; ++kc) {
                    xf[kc] = u32x4{0u, 0u, 0u, 0u};
                    if (inside && 4 * kc + g < a.p1) xf[kc] = *(const u32x4*)(xp + (long long)(4 * kc + g) * hw * 16);
                }
            };
            u32x4 xfa[NT], xfb[NT];
            load_xf(0, xfa);
            __builtin_amdgcn_s_barrier();  // E1
            __builtin_amdgcn_s_barrier();  // E2: gate weights are in LDS
#pragma unroll
            for (int pf = 0; pf < 4; ++pf) {
                __builtin_amdgcn_sched_barrier(0);
                u32x4 (&xf)[NT] = (pf & 1) ? xfb : xfa;
                if (pf + 1 < 4) load_xf(pf + 1, (pf & 1) ? xfa : xfb);
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) acc[pf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};
                // gate: beta = Wx . x + Wz . z   (K steps 0..NT-1 = x, NT..2NT-1 = z)
                u32x4 wa[NT], wb[NT];
                gate_reads<NT, 0, 0>(wa, mix_lane);
                gate_halves<TT, NT, 0>(acc[pf], xf, zb[pf], wa, wb, mix_lane);
                // x again, in accumulator layout (channels 16 nf + 4 g .. + 3): the lines were just fetched above
                bool inside;
                const char* const xp = x_ptr(pf, inside);
                uint2 xq[NF];
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    xq[nf] = make_uint2(0u, 0u);
                    if (inside && 2 * nf + (g >> 1) < a.p1) xq[nf] = *(const uint2*)(xp + (long long)(2 * nf + (g >> 1)) * hw * 16 + (g & 1) * 8);
                }
                // blend, in place: out = x + sigmoid(alpha) * sigmoid(beta) * (z - x)
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    float zv[4], xv[4];
                    unpack2<TT>(zb[pf][nf >> 1][(nf & 1) * 2], zv[0], zv[1]);
                    unpack2<TT>(zb[pf][nf >> 1][(nf & 1) * 2 + 1], zv[2], zv[3]);
                    unpack2<TT>(xq[nf].x, xv[0], xv[1]);
                    unpack2<TT>(xq[nf].y, xv[2], xv[3]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[pf][nf][j] = blend_(xv[j], zv[j], acc[pf][nf][j], a.inv_mix_scale);
                }
                store_frag16<TT, NT, MODE, EPI_STORE, false>(a, acc[pf], pf, lane, w, nbase, b, y0, x0);
            }
        } else
        if (a.epi == EPI_D2S) store_epilogue16<TT, NT, MODE, EPI_D2S, false>(a, acc, lane, w, nbase, b, y0, x0);
        else if (a.film_gamma) {
            if (a.silu) store_epilogue16<TT, NT, MODE, EPI_STORE, true, true>(a, acc, lane, w, nbase, b, y0, x0);
            else store_epilogue16<TT, NT, MODE, EPI_STORE, false, true>(a, acc, lane, w, nbase, b, y0, x0);
        }
        else if (a.silu) store_epilogue16<TT, NT, MODE, EPI_STORE, true>(a, acc, lane, w, nbase, b, y0, x0);
        else store_epilogue16<TT, NT, MODE, EPI_STORE, false>(a, acc, lane, w, nbase, b, y0, x0);
        cur = seek(cur + step, mtile, ntile);
    }
}

}  // namespace mz
