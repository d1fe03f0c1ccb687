// What the two "relay" kernels share (conv3r_kernel, mz_conv3r.h; conv3t_kernel, mz_conv3t.h): a workgroup of two TEAMS of four waves
// (waves w and w + 4 share a SIMD) that swap between the compute role and the loader + epilogue role from tile to tile.  Here: the
// device helpers of the helper role -- the lane index, the scalar-f32 activation / blend chains, the swap of packed words, the wait
// states behind the fused mix's gate GEMM.
//
// Everything here is inlined into kernels that live at their register cap (253 VGPRs, two waves per SIMD): a change must leave their
// listings as they are (tools/cmp_listings.py) or be measured as a change of the kernels.  That test also decided what is NOT here and
// exists once in each kernel, marked "twin:" at both copies: the tile walk over the host's table, the descriptor and inline-asm loads
// of the fused mix's x, the halo DMA offsets, the role driver, conv3t's accumulator clearing.  As a struct / as functions of this header
// each of them compiled to other code (register allocation, SGPR spills; the tile walk in all 22 kernels).
#pragma once
#include <type_traits>
#include "mz_device.h"

namespace mz {
namespace relay {

template <int V> using ic = std::integral_constant<int, V>;

// lane index, recomputed where it is needed (v_mbcnt): no register holds it across the K loop, whose 253 registers are all taken,
// and nothing derived from it can be hoisted out of the tile loop (and spilled)
__device__ __forceinline__ int lane_now() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

template <class TT> __device__ __forceinline__ void unpack2r(uint32_t v, float& lo, float& hi) {
    if constexpr (TT::IS_BF16) {
        lo = __builtin_bit_cast(float, v << 16);
        hi = __builtin_bit_cast(float, v & 0xffff0000u);
    } else {
        lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffff));
        hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16));
    }
}
template <class TT> __device__ __forceinline__ uint32_t pack2r(float lo, float hi) {
    if constexpr (TT::IS_BF16) return pack_bf16(lo, hi);
    else return pack_f16(lo, hi);
}

// v * sigmoid(v) of TWO values: v_mul, v_exp, v_add, v_rcp, v_mul each, as ONE inline-asm block with the two chains
// interleaved.  Inline asm because hipcc's SLP vectoriser pairs the multiplies and adds into v_pk_* (7 x slower beside the
// partner's MFMA stream); one block because hipcc's hazard recogniser does not look inside inline asm: a VALU instruction that
// reads the result of a transcendental one needs ONE wait state, which the other chain's instruction provides (no s_nop).
// The same operations in the same order as silu2() / sigmoidf_(): identical bits.
// OUT of place (the inputs stay untouched: accumulator elements need no copy into scratch registers first; the results double as
// the chains' temporaries)
__device__ __forceinline__ void silu_pair_to(float& ra, float& rb, const float a, const float b) {
    asm("v_mul_f32 %0, 0xbfb8aa3b, %2\n\t"
        "v_mul_f32 %1, 0xbfb8aa3b, %3\n\t"
        "v_exp_f32 %0, %0\n\t"
        "v_exp_f32 %1, %1\n\t"
        "v_add_f32 %0, 1.0, %0\n\t"
        "v_add_f32 %1, 1.0, %1\n\t"
        "v_rcp_f32 %0, %0\n\t"
        "v_rcp_f32 %1, %1\n\t"
        "v_mul_f32 %0, %2, %0\n\t"
        "v_mul_f32 %1, %3, %1"
        : "=&v"(ra), "=&v"(rb)
        : "v"(a), "v"(b));
}

// x + sigmoid(alpha) sigmoid(beta) (z - x) of TWO values, out of place: blend_()'s operations in blend_()'s order
// (mz_device.h: v_mul, v_exp, v_fma, v_rcp, v_sub, v_fma; identical bits), as one inline-asm block of two interleaved chains for the
// same reasons as silu_pair_to() -- left to hipcc, the SLP vectoriser pairs the adds and fmas into v_pk_add_f32 / v_pk_fma_f32.
__device__ __forceinline__ void blend_pair_to(float& o0, float& o1, const float b0, const float b1, const float x0, const float x1,
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

// clears a wave's accumulators.  Only the fused variants do: a plain tile's first tap WRITES them (mma16_first(), mz_device.h); with
// that form in the fused variants hipcc spills around the tile loop.  (conv3r_kernel; conv3t_kernel's fused variant orders its
// register moves differently with this function in place of its inline loops, and keeps those.)
template <int P, int N> __device__ __forceinline__ void zero_acc(f32x4 (&acc)[P][N]) {
#pragma unroll
    for (int pf = 0; pf < P; ++pf)
#pragma unroll
        for (int nf = 0; nf < N; ++nf) acc[pf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Behind the gate GEMM of the fused mix.  MFMA result -> VALU read is a SOFTWARE hazard on this chip (8 passes: 11 wait states), and
// hipcc's hazard recogniser does not look inside inline asm: the blend (blend_pair_to()) reads the gate beta from inline-asm chains.
// Without these wait states the first pair of a unit now and then blended with a stale beta (intermittent, under the partner's MFMA
// stream only: conv3t_kernel met it; in conv3r_kernel's tile loop a whole step lies between gate and blend, in its final epilogue
// they follow each other directly).
__device__ __forceinline__ void gate_settle() {
    asm volatile("s_nop 7\n\ts_nop 4" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// The 16 bytes of an epilogue entry from the PACKED words of two accumulator fragments: v_permlane16_swap pairs the fragments' quads
// into the lane's 8 channels (as entry16(), mz_device.h) -- two swaps per entry instead of four on unpacked values, on fresh registers:
// no accumulator copies, no hazard s_nops.  The swap only moves lanes: identical bits.
__device__ __forceinline__ u32x4 swap_packed(const uint32_t (&pa)[2], const uint32_t (&pb)[2]) {
    u32x4 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const auto sw = __builtin_amdgcn_permlane16_swap(pa[h], pb[h], false, false);
        o[h] = sw[0];
        o[2 + h] = sw[1];
    }
    return o;
}

}  // namespace relay
}  // namespace mz
