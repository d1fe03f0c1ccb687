// mix16_kernel / mix16b_kernel: AdaptiveResidualMix for C = k * 192 on the 16x16x32 MFMA, 16-bit types (launchers: mz_mix16.hip).
#pragma once
#include "mz_device.h"

namespace mz {

// ================================================================================================
// mix16_kernel: AdaptiveResidualMix (model.py:826-839) for C = k * 192 channels on the 16x16x32 MFMA (16-bit types).
//   out = x + sigmoid(alpha) * sigmoid(W [x ; z]) * (z - x),   W: [C, 2C]
// The 1x1 gate GEMM has no tap reuse, so it lives on activation traffic: the general 1x1 kernel stages x and z through
// LDS once per 96-channel N tile.  Here (a) an N tile is 192 channels (half the passes over x and z), and (b) x and z never
// touch LDS: in the plane-major layout a lane's 16 bytes of plane 4 ks + g of pixel c ARE its B-operand fragment of
// K step ks, so they are plain global loads, requested three K steps ahead.  Only the weights (12 KB per K step, shared
// by the 8 compute waves) go through LDS: a loader wave streams stages of 4 K steps into two slots.
// Workgroup = 256 pixels x 192 channels: wave w owns pixels 32 w .. 32 w + 31 (two 16-pixel fragments) x 12 channel
// fragments = 96 accumulator registers; weight pairs are read two 4-MFMA groups ahead with counted lgkmcnt.
// ================================================================================================
// blend_() of TWO values as one inline-asm block of two interleaved scalar-f32 chains (blend_()'s operations in blend_()'s order: identical
// bits).  Left to hipcc, the SLP vectoriser pairs the subtractions and fmas of neighbouring values into v_pk_add_f32 / v_pk_fma_f32, and
// packed-f32 instructions take ~40 cycles beside the MFMA stream of the SIMD's other wave instead of ~9 (tools/microbench/mb_coissue.hip,
// DESIGN.md 5.0) -- in mix16b_kernel a wave's blend runs beside its partner's K loop most of the time.
__device__ __forceinline__ void mix_blend_pair(float& o0, float& o1, const float b0, const float b1, const float x0, const float x1,
                                               const float z0, const float z1, const float inv_s) {
    float d0, d1;
    asm("v_mul_f32 %0, 0xbfb8aa3b, %4\n\t"
        "v_mul_f32 %1, 0xbfb8aa3b, %5\n\t"
        "v_exp_f32 %0, %0\n\t"
        "v_exp_f32 %1, %1\n\t"
        "v_fma_f32 %0, %0, %10, %10\n\t"
        "v_fma_f32 %1, %1, %10, %10\n\t"
        "v_rcp_f32 %0, %0\n\t"
        "v_rcp_f32 %1, %1\n\t"
        "v_sub_f32 %2, %8, %6\n\t"
        "v_sub_f32 %3, %9, %7\n\t"
        "v_fma_f32 %0, %0, %2, %6\n\t"
        "v_fma_f32 %1, %1, %3, %7"
        : "=&v"(o0), "=&v"(o1), "=&v"(d0), "=&v"(d1)
        : "v"(b0), "v"(b1), "v"(x0), "v"(x1), "v"(z0), "v"(z1), "s"(inv_s));
}

struct MixFrag {
    u32x4 w[3][2];
};
template <class TT, int G>  // group G of a stage: K step G / 6, channel-fragment pair G % 6
__device__ __forceinline__ void mix16_group(f32x4 (&acc)[2][12], MixFrag& f, const u32x4 (&xb)[2], uint32_t b_addr) {
    constexpr int n = G % 6, wp = G % 3;
    // request the pair of group G + 2 (same stage), then this group's four MFMAs
    if constexpr (G + 2 < 24) {
        f.w[(G + 2) % 3][0] = lds_read128<(((G + 2) / 6) * 12 + 2 * ((G + 2) % 6)) * 1024>(b_addr);
        f.w[(G + 2) % 3][1] = lds_read128<(((G + 2) / 6) * 12 + 2 * ((G + 2) % 6) + 1) * 1024>(b_addr);
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr int p0 = G & 1, p1 = p0 ^ 1;   // serpentine: one operand changes per MFMA; odd groups start on the other pixel fragment,
    mma16<TT>(acc[p0][2 * n], f.w[wp][0], xb[p0]);           // so the B operand also stays put across a group boundary
    mma16<TT>(acc[p0][2 * n + 1], f.w[wp][1], xb[p0]);
    mma16<TT>(acc[p1][2 * n + 1], f.w[wp][1], xb[p1]);
    mma16<TT>(acc[p1][2 * n], f.w[wp][0], xb[p1]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (G + 1 < 24) wait_w16<(G + 2 < 24 ? 2 : 0)>(f.w[(G + 1) % 3][0], f.w[(G + 1) % 3][1]);
}
template <class TT, int KS> __device__ __forceinline__ void mix16_kstep(f32x4 (&acc)[2][12], MixFrag& f, const u32x4 (&xb)[2], uint32_t b_addr) {
    mix16_group<TT, KS * 6 + 0>(acc, f, xb, b_addr);
    mix16_group<TT, KS * 6 + 1>(acc, f, xb, b_addr);
    mix16_group<TT, KS * 6 + 2>(acc, f, xb, b_addr);
    mix16_group<TT, KS * 6 + 3>(acc, f, xb, b_addr);
    mix16_group<TT, KS * 6 + 4>(acc, f, xb, b_addr);
    mix16_group<TT, KS * 6 + 5>(acc, f, xb, b_addr);
}

template <class TT>
__global__ __launch_bounds__(576) void mix16_kernel(const ConvArgs a) {
    constexpr int STAGE = 4 * 12 * 1024;  // 4 K steps x 12 fragments
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7 compute, 8 = weight loader
    int mtile, ntile;
    if (!map_tile(a, mtile, ntile)) return;
    const int nsteps = a.nchunks16;  // K steps of 32 channels over [x ; z]; a multiple of 4
    const int nstages = nsteps >> 2;

    if (w == 8) {
        const char* src = (const char*)a.wpk16 + (size_t)ntile * nsteps * (12 * 1024) + lane * 16;
        auto issue = [&](int st) __attribute__((always_inline)) {
            char* dst = smem + (st & 1) * STAGE;
#pragma unroll
            for (int j = 0; j < 48; ++j) glds16(src + (size_t)st * STAGE + j * 1024, dst + j * 1024);
        };
        issue(0);
        for (int st = 0; st < nstages; ++st) {
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();            // stage st landed; everyone has finished stage st - 1
            if (st + 1 < nstages) issue(st + 1);
        }
        return;
    }

    const int g = lane >> 4, c = lane & 15;
    const long long hw = (long long)a.Ho * a.Wo;
    const long long M = (long long)a.B * hw;
    const int half_steps = nsteps >> 1;  // K steps of x (= of z)
    // Buffer-addressed loads: one descriptor per tensor (the host guarantees < 4 GiB), this lane's pixel as a 32-bit byte
    // offset of its plane g (0xffffffff = beyond the tensor: the range check returns zeros), the K step as a scalar offset.
    const uint32_t tensor_bytes = (uint32_t)((long long)a.B * a.p0 * hw * 16);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.in0, 0, (int)tensor_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc((void*)a.in1, 0, (int)tensor_bytes, 0x00020000);
    uint32_t voff[2];   // (image, plane g, pixel) -> bytes
    uint32_t vpix[2];   // (image, plane 0, pixel) -> bytes, for the epilogue
#pragma unroll
    for (int pf = 0; pf < 2; ++pf) {
        const long long m = (long long)mtile * 256 + 32 * w + 16 * pf + c;
        const bool in = m < M;
        const long long mm = in ? m : 0;
        const int bimg = (int)(mm / hw);
        const long long pix = mm - (long long)bimg * hw;
        vpix[pf] = in ? (uint32_t)((((long long)bimg * a.p0) * hw + pix) * 16) : 0xffffffffu;
        voff[pf] = in ? (uint32_t)((((long long)bimg * a.p0 + g) * hw + pix) * 16) : 0xffffffffu;
    }
    const uint32_t step_bytes = (uint32_t)(4 * hw * 16);  // four planes per K step
    auto load_b = [&](int ks, u32x4 (&xb)[2]) __attribute__((always_inline)) {  // B operands of K step ks (zeros past the end)
        const bool isz = ks >= half_steps;
        const int kk = ks >= nsteps ? 0 : (isz ? ks - half_steps : ks);
        const int so = __builtin_amdgcn_readfirstlane((int)(kk * step_bytes));
#pragma unroll
        for (int pf = 0; pf < 2; ++pf)
            xb[pf] = isz ? __builtin_amdgcn_raw_buffer_load_b128(zr, (int)voff[pf], so, 0)
                         : __builtin_amdgcn_raw_buffer_load_b128(xr, (int)voff[pf], so, 0);
    };
    f32x4 acc[2][12];
#pragma unroll
    for (int pf = 0; pf < 2; ++pf)
#pragma unroll
        for (int nf = 0; nf < 12; ++nf) acc[pf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const uint32_t b_lane = lds_base + lane * 16;
    // B operands two K steps ahead in three rotating buffers; the stage loop is unrolled three times so that the
    // rotation (12 K steps = 4 turns) is static -- the K-step count is a multiple of 12 whenever C is one of 192
    u32x4 xb0[2], xb1[2], xb2[2];
    load_b(0, xb0);
    load_b(1, xb1);
    MixFrag f;
    auto stage_head = [&](uint32_t b_addr) __attribute__((always_inline)) {
        __builtin_amdgcn_s_barrier();
        f.w[0][0] = lds_read128<0>(b_addr);
        f.w[0][1] = lds_read128<1024>(b_addr);
        f.w[1][0] = lds_read128<2048>(b_addr);
        f.w[1][1] = lds_read128<3072>(b_addr);
        wait_w16<2>(f.w[0][0], f.w[0][1]);
    };
    for (int st = 0; st < nstages; st += 3) {
        const int ks = 4 * st;
        uint32_t b_addr = b_lane + (st & 1) * STAGE;
        stage_head(b_addr);
        load_b(ks + 2, xb2);  mix16_kstep<TT, 0>(acc, f, xb0, b_addr);
        load_b(ks + 3, xb0);  mix16_kstep<TT, 1>(acc, f, xb1, b_addr);
        load_b(ks + 4, xb1);  mix16_kstep<TT, 2>(acc, f, xb2, b_addr);
        load_b(ks + 5, xb2);  mix16_kstep<TT, 3>(acc, f, xb0, b_addr);
        b_addr = b_lane + ((st + 1) & 1) * STAGE;
        stage_head(b_addr);
        load_b(ks + 6, xb0);  mix16_kstep<TT, 0>(acc, f, xb1, b_addr);
        load_b(ks + 7, xb1);  mix16_kstep<TT, 1>(acc, f, xb2, b_addr);
        load_b(ks + 8, xb2);  mix16_kstep<TT, 2>(acc, f, xb0, b_addr);
        load_b(ks + 9, xb0);  mix16_kstep<TT, 3>(acc, f, xb1, b_addr);
        b_addr = b_lane + (st & 1) * STAGE;
        stage_head(b_addr);
        load_b(ks + 10, xb1); mix16_kstep<TT, 0>(acc, f, xb2, b_addr);
        load_b(ks + 11, xb2); mix16_kstep<TT, 1>(acc, f, xb0, b_addr);
        load_b(ks + 12, xb0); mix16_kstep<TT, 2>(acc, f, xb1, b_addr);
        load_b(ks + 13, xb1); mix16_kstep<TT, 3>(acc, f, xb2, b_addr);
    }
    // ---- blend and store, one pixel fragment and one channel-fragment pair at a time.  x and z come back in ACCUMULATOR layout
    //      (8 bytes per lane and fragment; L2 hits: the K loop has just read these lines); the loads of group i + 1 are requested
    //      before group i is blended -- left to itself hipcc requests them right before their use, twelve exposed L2 round trips
    //      per tile with nothing else in flight on the CU ----
    const int nbase = ntile * 192;
    const uint32_t plane_bytes = (uint32_t)(hw * 16);
    typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
    struct XZ { u32x2_ x[2], z[2]; };
    auto request = [&](int i, XZ& q) __attribute__((always_inline)) {
        const int pf = i / 6, n = i - 6 * pf;
        const bool in = vpix[pf] != 0xffffffffu;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int nf = 2 * n + k;
            const int plane = (nbase >> 3) + 2 * nf + (g >> 1);  // channels nbase + 16 nf + 4 g ..
            const uint32_t off = in ? vpix[pf] + (uint32_t)plane * plane_bytes + (g & 1) * 8 : 0xffffffffu;
            q.x[k] = __builtin_amdgcn_raw_buffer_load_b64(xr, (int)off, 0, 0);
            q.z[k] = __builtin_amdgcn_raw_buffer_load_b64(zr, (int)off, 0, 0);
        }
    };
    auto finish = [&](int i, const XZ& q) __attribute__((always_inline)) {
        const int pf = i / 6, n = i - 6 * pf;
        const bool in = vpix[pf] != 0xffffffffu;
        float v[8];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int nf = 2 * n + k;
            float xv[4], zv[4];
            unpack2<TT>(q.x[k][0], xv[0], xv[1]); unpack2<TT>(q.x[k][1], xv[2], xv[3]);
            unpack2<TT>(q.z[k][0], zv[0], zv[1]); unpack2<TT>(q.z[k][1], zv[2], zv[3]);
            float o0, o1, o2, o3;
            mix_blend_pair(o0, o1, acc[pf][nf][0], acc[pf][nf][1], xv[0], xv[1], zv[0], zv[1], a.inv_mix_scale);
            mix_blend_pair(o2, o3, acc[pf][nf][2], acc[pf][nf][3], xv[2], xv[3], zv[2], zv[3], a.inv_mix_scale);
            acc[pf][nf] = f32x4{o0, o1, o2, o3};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ea = acc[pf][2 * n][j], eb = acc[pf][2 * n + 1][j];
            const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, ea), __builtin_bit_cast(uint32_t, eb), false, false);
            const uint32_t s0 = sw[0], s1 = sw[1];
            v[j] = __builtin_bit_cast(float, s0);
            v[4 + j] = __builtin_bit_cast(float, s1);
        }
        const int cu = 2 * (2 * n + (g & 1)) + (g >> 1);
        if (in) st_unit<TT>((char*)a.out + vpix[pf] + (long long)((nbase >> 3) + cu) * plane_bytes, v);
    };
    XZ qa, qb;
    request(0, qa);
#pragma unroll
    for (int i = 0; i < 12; i += 2) {
        request(i + 1, qb);
        __builtin_amdgcn_sched_barrier(0);
        finish(i, qa);
        if (i + 2 < 12) request(i + 2, qa);
        __builtin_amdgcn_sched_barrier(0);
        finish(i + 1, qb);
    }
}

// ================================================================================================
// mix16b_kernel (round 3, second session): AdaptiveResidualMix for C = 192 without the second read of x and z, persistent.
// mix16_kernel blends in accumulator layout and therefore fetches x and z a second time (8-byte loads, L2 hit rate 0.38 at
// C = 192: counted traffic 2.79 GB against 1.79 GB algorithmic -- DESIGN 5.3), and its workgroup -- the only one its CU has room
// for -- alternates between a read-only K loop and a write-only epilogue.  Here
//   * the gate weights are packed (PK_MIX16B) so that accumulator row 4 g + j of channel fragment 2 m + h is channel
//     32 m + 8 g + 4 h + j: lane (g, c) then owns, as accumulators, exactly the eight channels of pixel c that it loaded as the B
//     operand of K step m -- x, z and beta of one 16-byte plane entry sit in ONE lane: the 24 B operands of a unit (96 registers)
//     are kept until the blend, no second read, no v_permlane16_swap, one 16-byte store per entry;
//   * the whole gate matrix (144 KB) stays in LDS for the life of the workgroup (one per CU, eight waves of 256 registers, no loader
//     wave): after the first barrier there is no barrier and no LDS-DMA at all; every WAVE walks its own 32-pixel units;
//   * the loads of a wave's NEXT unit are issued between the stores of the current one, entry by entry into the registers the blend
//     has just released: reads and writes of a CU overlap, and the next K loop finds its first operands on the way.
// C = 192 only (one N tile whose twelve K steps are all its own): for C > 192 the other K steps have to stream through rotating
// buffers next to the 96 kept registers and hipcc spills in that loop, so C = 384 / 768 stay on mix16_kernel.
// ================================================================================================
template <class TT>
__global__ __launch_bounds__(512) void mix16b_kernel(const ConvArgs a) {
    constexpr int STAGE = 4 * 12 * 1024;  // 4 K steps x 12 fragments
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
    {   // the gate matrix: 144 pieces of 1 KB, 18 per wave
        const char* wsrc = (const char*)a.wpk16 + lane * 16 + w * (18 * 1024);
        char* dst = smem + w * (18 * 1024);
#pragma unroll
        for (int j = 0; j < 18; ++j) glds16(wsrc + j * 1024, dst + j * 1024);
    }
    const int g = lane >> 4, c = lane & 15;
    const long long hw = (long long)a.Ho * a.Wo;
    const long long M = (long long)a.B * hw;
    const uint32_t tensor_bytes = (uint32_t)((long long)a.B * a.p0 * hw * 16);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.in0, 0, (int)tensor_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc((void*)a.in1, 0, (int)tensor_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc((void*)a.out, 0, (int)tensor_bytes, 0x00020000);
    const uint32_t step_bytes = (uint32_t)(4 * hw * 16);  // four planes per K step
    const float inv_hw = 1.0f / (float)hw;
    // (image, plane g, pixel) -> bytes for the lane's pixel of fragment pf of unit u; 0xffffffff beyond the tensor: the range check
    // returns zeros for such loads and drops such stores
    const int hwi = (int)hw, Mi = (int)M;   // the host guarantees B * p0 * hw * 16 < 2^32, so B * hw < 2^24
    auto offsets = [&](int u, uint32_t (&vo)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int pf = 0; pf < 2; ++pf) {
            const int m = u * 32 + 16 * pf + c;
            const bool in = m < Mi;
            const int mm = in ? m : 0;
            int bimg = (int)((float)mm * inv_hw);  // estimate (exact float of mm < 2^24), then corrected: no integer division per unit
            int pix = mm - bimg * hwi;
            if (pix < 0) { bimg -= 1; pix += hwi; }
            if (pix >= hwi) { bimg += 1; pix -= hwi; }
            vo[pf] = in ? ((uint32_t)(bimg * a.p0 + g) * (uint32_t)hwi + (uint32_t)pix) * 16u : 0xffffffffu;
        }
    };
    const int nunits = (Mi + 31) / 32;
    const int stride = (int)gridDim.x * 8;
    int u = (int)blockIdx.x * 8 + w;
    uint32_t voff[2];
    offsets(u, voff);
    u32x4 R[12][2];  // x K steps 0..5, z K steps 0..5 of the current unit
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int so = __builtin_amdgcn_readfirstlane((int)(i * step_bytes));
#pragma unroll
        for (int pf = 0; pf < 2; ++pf) R[i][pf] = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)voff[pf], so, 0);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int so = __builtin_amdgcn_readfirstlane((int)(i * step_bytes));
#pragma unroll
        for (int pf = 0; pf < 2; ++pf) R[6 + i][pf] = __builtin_amdgcn_raw_buffer_load_b128(zr, (int)voff[pf], so, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    wait_vmcnt<0>();                // this wave's 18 pieces of the gate matrix (once per workgroup: the first unit's loads may as well land)
    __builtin_amdgcn_s_barrier();   // the only barrier of the kernel: every wave reaches it, also one without a unit
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const uint32_t b_lane = lds_base + lane * 16;
    MixFrag f;
    auto stage_head = [&](uint32_t b_addr) __attribute__((always_inline)) {
        f.w[0][0] = lds_read128<0>(b_addr);
        f.w[0][1] = lds_read128<1024>(b_addr);
        f.w[1][0] = lds_read128<2048>(b_addr);
        f.w[1][1] = lds_read128<3072>(b_addr);
        wait_w16<2>(f.w[0][0], f.w[0][1]);
    };
    while (u < nunits) {
        // the next unit's offsets first: here the accumulators are dead and their registers hold the temporaries
        const int un = u + stride;
        uint32_t vnext[2];
        offsets(un, vnext);   // beyond the last unit: 0xffffffff, the loads return zeros and nobody uses them
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[2][12];
#pragma unroll
        for (int pf = 0; pf < 2; ++pf)
#pragma unroll
            for (int nf = 0; nf < 12; ++nf) acc[pf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};
        stage_head(b_lane);
        mix16_kstep<TT, 0>(acc, f, R[0], b_lane);
        mix16_kstep<TT, 1>(acc, f, R[1], b_lane);
        mix16_kstep<TT, 2>(acc, f, R[2], b_lane);
        mix16_kstep<TT, 3>(acc, f, R[3], b_lane);
        stage_head(b_lane + STAGE);
        mix16_kstep<TT, 0>(acc, f, R[4], b_lane + STAGE);
        mix16_kstep<TT, 1>(acc, f, R[5], b_lane + STAGE);
        mix16_kstep<TT, 2>(acc, f, R[6], b_lane + STAGE);
        mix16_kstep<TT, 3>(acc, f, R[7], b_lane + STAGE);
        stage_head(b_lane + 2 * STAGE);
        mix16_kstep<TT, 0>(acc, f, R[8], b_lane + 2 * STAGE);
        mix16_kstep<TT, 1>(acc, f, R[9], b_lane + 2 * STAGE);
        mix16_kstep<TT, 2>(acc, f, R[10], b_lane + 2 * STAGE);
        mix16_kstep<TT, 3>(acc, f, R[11], b_lane + 2 * STAGE);
        // ---- blend and store entry (K step m, pixel fragment pf) = plane 4 m + g of the lane's pixel; behind it, the same entry's
        //      x and z of the wave's next unit go into the registers just released ----
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            const int so = __builtin_amdgcn_readfirstlane((int)(m * step_bytes));
#pragma unroll
            for (int pf = 0; pf < 2; ++pf) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float xl, xh, zl, zh;
                    unpack2<TT>(R[m][pf][q], xl, xh);
                    unpack2<TT>(R[6 + m][pf][q], zl, zh);
                    mix_blend_pair(v[2 * q], v[2 * q + 1], acc[pf][2 * m + (q >> 1)][2 * (q & 1)], acc[pf][2 * m + (q >> 1)][2 * (q & 1) + 1], xl, xh, zl, zh,
                                   a.inv_mix_scale);
                }
                u32x4 t;
                if constexpr (TT::IS_BF16) {
                    t[0] = pack_bf16(v[0], v[1]); t[1] = pack_bf16(v[2], v[3]); t[2] = pack_bf16(v[4], v[5]); t[3] = pack_bf16(v[6], v[7]);
                } else {
                    t[0] = pack_f16(v[0], v[1]); t[1] = pack_f16(v[2], v[3]); t[2] = pack_f16(v[4], v[5]); t[3] = pack_f16(v[6], v[7]);
                }
                // (an SGPR-offset store: hipcc puts no wait state behind it and had placed the next entry's first v_mul into v[data + 2]
                // right there -- garbage in a third of the runs; store16_soff() pins the wait states, mz_device.h)
                store16_soff(t, orr, (int)voff[pf], so);
            }
#pragma unroll
            for (int pf = 0; pf < 2; ++pf) {
                R[m][pf] = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)vnext[pf], so, 0);
                R[6 + m][pf] = __builtin_amdgcn_raw_buffer_load_b128(zr, (int)vnext[pf], so, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        u = un;
        voff[0] = vnext[0];
        voff[1] = vnext[1];
    }
}

}  // namespace mz
