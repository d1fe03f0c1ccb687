// gfx950 (MI355X / CDNA4): weight packing and the small kernels of the MewZoom upscale path (stem, border, QA reduction).
// The convolution and mix kernels live one family per unit: mz_conv32 (conv_kernel, conv3w, conv3p), mz_conv3s, mz_conv3r, mz_conv3t, mz_mix16.
#include "mz_device.h"
#include "mz_pack.h"

namespace mz {

// ================================================================================================
// weight packing: OIHW float32 -> [ntile][kchunk][tap][nt][lane][16 bytes] in the compute dtype
// ================================================================================================
template <class TT> __global__ void pack_kernel(const PackArgs a, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long long src = pack_source<TT::SZ>(a, idx);  // mz_pack.h
    st1<TT>((char*)a.dst + idx * TT::SZ, src >= 0 ? a.w[src] : 0.0f);
}

hipError_t launch_pack(const PackArgs& a, hipStream_t s) {
    const int sz = dtype_size(a.dtype);
    const long long total = (long long)packed_bytes(a.taps, a.frags, a.ntiles, a.nchunks) / sz;
    const int blocks = (int)((total + 255) / 256);
    switch (a.dtype) {
        case DT_F32: hipLaunchKernelGGL(pack_kernel<TF32>, dim3(blocks), dim3(256), 0, s, a, total); break;
        case DT_BF16: hipLaunchKernelGGL(pack_kernel<TBF16>, dim3(blocks), dim3(256), 0, s, a, total); break;
        case DT_F16: hipLaunchKernelGGL(pack_kernel<TF16>, dim3(blocks), dim3(256), 0, s, a, total); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ================================================================================================
// small kernels
// ================================================================================================
__global__ void pack_stem_kernel(const float* w, const float* b, float* dst, int c, int cp) {
    // dst: float4 per channel {w0, w1, w2, bias}; zero-initialised by the caller; either of w / b may be null
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cp) return;
    float4 v = ((float4*)dst)[i];
    if (i < c) {
        if (w) { v.x = w[i * 3 + 0]; v.y = w[i * 3 + 1]; v.z = w[i * 3 + 2]; }
        if (b) v.w = b[i];
    } else {
        v = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    ((float4*)dst)[i] = v;
}
hipError_t launch_pack_stem(const float* w, const float* b, float* dst, int c, int cp, hipStream_t s) {
    hipLaunchKernelGGL(pack_stem_kernel, dim3((cp + 63) / 64), dim3(64), 0, s, w, b, dst, c, cp);
    return hipGetLastError();
}

// FanOutProjection (reference model.py:239-242): per-pixel 3 -> C affine, NCHW image -> plane-major features.
// channels 8 g .. 8 g + 7 of pixel p of image b from its three colour values
template <class TT> __device__ __forceinline__ void stem_project(const float4* w4, void* out, long long b, int g, long long p, long long HW,
                                                                 int groups, float r0, float r1, float r2) {
    constexpr int SZ = TT::SZ;
    constexpr int NPL = SZ / 2;  // planes per group of 8 channels
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 wv = w4[g * 8 + j];
        v[j] = wv.w + wv.x * r0 + wv.y * r1 + wv.z * r2;
    }
    char* op = (char*)out + ((b * groups * NPL + (long long)g * NPL) * HW + p) * 16;
    if (SZ == 2) {
        st4<TT>(op, v);
        st4<TT>(op + 4 * SZ, v + 4);
    } else {
        st4<TT>(op, v);
        st4<TT>(op + HW * 16, v + 4);
    }
}
template <class TT, bool U8> __global__ void stem_kernel(const void* x, const float4* w4, void* out, long long total,
                                                          long long HW, int groups) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long long p = idx % HW;  // pixel fastest: loads and stores are contiguous along p
    const long long t = idx / HW;
    const int g = (int)(t % groups);
    const long long b = t / groups;
    const long long xi = b * 3 * HW + p;
    const float r0 = ld_img<TT, U8>(x, xi), r1 = ld_img<TT, U8>(x, xi + HW), r2 = ld_img<TT, U8>(x, xi + 2 * HW);
    stem_project<TT>(w4, out, b, g, p, HW, groups, r0, r1, r2);
}
// The same from an image view: element (b, c, y, x) at x[b s0 + c s1 + y s2 + x s3] (element strides, signed).  The plane-major store
// is the dense kernel's.
struct StemView {
    long long s[4];
    int W;
};
template <class TT, bool U8> __global__ void stem_view_kernel(const void* x, const float4* w4, void* out, long long total,
                                                               long long HW, int groups, const StemView v) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long long p = idx % HW;
    const long long t = idx / HW;
    const int g = (int)(t % groups);
    const long long b = t / groups;
    const long long py = p / v.W, px = p - py * v.W;
    const long long xi = b * v.s[0] + py * v.s[2] + px * v.s[3];
    const float r0 = ld_img<TT, U8>(x, xi), r1 = ld_img<TT, U8>(x, xi + v.s[1]), r2 = ld_img<TT, U8>(x, xi + 2 * v.s[1]);
    stem_project<TT>(w4, out, b, g, p, HW, groups, r0, r1, r2);
}
hipError_t launch_stem(int dtype, const void* x, const float* w4, void* out, int B, int H, int W, int cp, hipStream_t s,
                       int u8, const long long* vin) {
    const long long HW = (long long)H * W;
    const int groups = cp / 8;
    const long long total = HW * B * groups;
    const int blocks = (int)((total + 255) / 256);
    if (vin) {
        const StemView v = {{vin[0], vin[1], vin[2], vin[3]}, W};
        auto go = [&](auto tt) {
            using TT = decltype(tt);
            if (u8) hipLaunchKernelGGL((stem_view_kernel<TT, true>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups, v);
            else hipLaunchKernelGGL((stem_view_kernel<TT, false>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups, v);
        };
        switch (dtype) {
            case DT_F32: go(TF32{}); break;
            case DT_BF16: go(TBF16{}); break;
            case DT_F16: go(TF16{}); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (dtype) {
        case DT_F32: if (u8) hipLaunchKernelGGL((stem_kernel<TF32, true>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups); else hipLaunchKernelGGL((stem_kernel<TF32, false>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups); break;
        case DT_BF16: if (u8) hipLaunchKernelGGL((stem_kernel<TBF16, true>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups); else hipLaunchKernelGGL((stem_kernel<TBF16, false>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups); break;
        case DT_F16: if (u8) hipLaunchKernelGGL((stem_kernel<TF16, true>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups); else hipLaunchKernelGGL((stem_kernel<TF16, false>), dim3(blocks), dim3(256), 0, s, x, (const float4*)w4, out, total, HW, groups); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// Decoder.crop_feature_maps zero padding (reference model.py:667-673, 681-687): bottom rows / right columns.
__global__ void zero_border_kernel(char* t, int B, int Hout, int Wout, int planes, int Hv, int Wv) {
    // one thread per border pixel of one plane; border = rows >= Hv (all columns) and columns >= Wv (rows < Hv)
    const long long nb_rows = (long long)(Hout - Hv) * Wout;
    const long long nb_cols = (long long)Hv * (Wout - Wv);
    const long long per_plane = nb_rows + nb_cols;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = per_plane * B * planes;
    if (idx >= total) return;
    long long k = idx % per_plane;
    const long long bp = idx / per_plane;  // b * planes + plane
    int y, x;
    if (k < nb_rows) {
        y = Hv + (int)(k / Wout);
        x = (int)(k % Wout);
    } else {
        k -= nb_rows;
        const int wc = Wout - Wv;
        y = (int)(k / wc);
        x = Wv + (int)(k % wc);
    }
    *(uint4*)(t + ((bp * Hout + y) * Wout + x) * 16) = make_uint4(0, 0, 0, 0);
}
hipError_t launch_zero_border(int dtype, void* t, int B, int Hout, int Wout, int cp, int Hv, int Wv, hipStream_t s) {
    if (Hv >= Hout && Wv >= Wout) return hipSuccess;
    const int planes = cp * dtype_size(dtype) / 16;
    const long long per_plane = (long long)(Hout - Hv) * Wout + (long long)Hv * (Wout - Wv);
    const long long total = per_plane * B * planes;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(zero_border_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (char*)t, B, Hout, Wout,
                       planes, Hv, Wv);
    return hipGetLastError();
}

// QualityAssessor pooling (reference model.py:1028-1030): spatial mean of the conv output, plus the conv bias.
template <class TT> __global__ void qa_reduce_kernel(const void* feat, const float* bias, float* qa, int P, int cp, int F) {
    constexpr int SZ = TT::SZ;
    __shared__ float red[256];
    constexpr int PPU = 16 / SZ;  // channels per plane
    const int b = blockIdx.x, f = blockIdx.y;
    const int planes = cp / PPU;
    const char* base = (const char*)feat + (((long long)b * planes + f / PPU) * P) * 16 + (f % PPU) * SZ;
    float sum = 0.0f;
    for (int p = threadIdx.x; p < P; p += 256) sum += ld1<TT>(base + (long long)p * 16);
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) qa[b * F + f] = red[0] / (float)P + bias[f];
}
hipError_t launch_qa_reduce(int dtype, const void* feat, const float* bias, float* qa, int B, int P, int cp, int F,
                            hipStream_t s) {
    switch (dtype) {
        case DT_F32: hipLaunchKernelGGL(qa_reduce_kernel<TF32>, dim3(B, F), dim3(256), 0, s, feat, bias, qa, P, cp, F); break;
        case DT_BF16: hipLaunchKernelGGL(qa_reduce_kernel<TBF16>, dim3(B, F), dim3(256), 0, s, feat, bias, qa, P, cp, F); break;
        case DT_F16: hipLaunchKernelGGL(qa_reduce_kernel<TF16>, dim3(B, F), dim3(256), 0, s, feat, bias, qa, P, cp, F); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_fill_zero(void* p, size_t bytes, hipStream_t s) { return hipMemsetAsync(p, 0, bytes, s); }

}  // namespace mz
