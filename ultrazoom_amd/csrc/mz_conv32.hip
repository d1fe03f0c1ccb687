// Instantiations and launchers of the 32x32-MFMA convolution families: conv_kernel (mz_conv256.h), conv3w_kernel and conv3p_kernel
// (mz_conv3w.h).  ONE unit on purpose, conv_kernel first: the three share the epilogues of mz_conv_common.h, and hipcc's code for
// conv3w_kernel<.., NT = 3, ..> depends on whether those helpers enter the module ahead of the kernel (under conv_kernel) or behind it
// -- in a unit of its own the twelve instantiations came out with other address arithmetic than in the listing they were tuned with.
#include "mz_conv256.h"
#include "mz_conv3w.h"

namespace mz {

hipError_t launch_conv256(int dtype, int mode, int nt, const ConvArgs& a, hipStream_t s) {
    if (!walk_ok(a)) return hipErrorInvalidValue;
    if (a.view) {  // the image head on image views: 12 output channels, one 32-channel N tile
        if (mode != MODE_CONV3 || nt != 1 || a.epi != EPI_FINAL) return hipErrorInvalidValue;
        switch (dtype) {
            case DT_F32: return launch_lds<conv_kernel<TF32, 1, MODE_CONV3, true>>(a.grid, 256, conv_lds_bytes<MODE_CONV3>(1), a, s);
            case DT_BF16: return launch_lds<conv_kernel<TBF16, 1, MODE_CONV3, true>>(a.grid, 256, conv_lds_bytes<MODE_CONV3>(1), a, s);
            case DT_F16: return launch_lds<conv_kernel<TF16, 1, MODE_CONV3, true>>(a.grid, 256, conv_lds_bytes<MODE_CONV3>(1), a, s);
        }
        return hipErrorInvalidValue;
    }
    return dispatch<4, MODE_CONV3, MODE_GEMM1>(dtype, nt, mode, [&](auto tt, auto n, auto m) {
        using TT = decltype(tt);
        constexpr int NT = decltype(n)::value, MODE = decltype(m)::value;
        return launch_lds<conv_kernel<TT, NT, MODE>>(a.grid, 256, conv_lds_bytes<MODE>(NT), a, s);
    });
}

// one workgroup per tile; EPI_FUSEDMIX: the fused variant (a.wmix / a.mix_pieces = the gate packed with SRC_MIXF)
hipError_t launch_conv3w(int dtype, int mode, int nt, const ConvArgs& a, hipStream_t s) {
    if (!walk_ok(a)) return hipErrorInvalidValue;
    if (a.view) {  // the f32 image head on image views (choose_conv3 keeps the 16-bit heads on conv_kernel)
        if (dtype != DT_F32 || nt != 1 || a.epi != EPI_FINAL) return hipErrorInvalidValue;
        if (mode == MODE_C3W16) return launch_lds<conv3w_kernel<TF32, 1, MODE_C3W16, false, true>>(a.grid, 576, conv_lds_bytes<MODE_C3W16>(1), a, s);
        if (mode == MODE_C3W8) return launch_lds<conv3w_kernel<TF32, 1, MODE_C3W8, false, true>>(a.grid, 576, conv_lds_bytes<MODE_C3W8>(1), a, s);
        return hipErrorInvalidValue;
    }
    return dispatch<3, MODE_C3W16, MODE_C3W8>(dtype, nt, mode, [&](auto tt, auto n, auto m) {
        using TT = decltype(tt);
        constexpr int NT = decltype(n)::value, MODE = decltype(m)::value;
        if (a.epi == EPI_FUSEDMIX) return launch_lds<conv3w_kernel<TT, NT, MODE, true>>(a.grid, 576, conv_lds_bytes<MODE>(NT), a, s);
        return launch_lds<conv3w_kernel<TT, NT, MODE, false>>(a.grid, 576, conv_lds_bytes<MODE>(NT), a, s);
    });
}

// persistent: a.persist workgroups; store epilogues only
hipError_t launch_conv3p(int dtype, int mode, int nt, const ConvArgs& a, hipStream_t s) {
    if (!walk_ok(a) || a.persist <= 0 || (a.epi != EPI_STORE && a.epi != EPI_D2S)) return hipErrorInvalidValue;
    return dispatch<3, MODE_C3W16, MODE_C3W8>(dtype, nt, mode, [&](auto tt, auto n, auto m) {
        using TT = decltype(tt);
        constexpr int NT = decltype(n)::value, MODE = decltype(m)::value;
        return launch_lds<conv3p_kernel<TT, NT, MODE>>(a.persist, 640, conv_lds_bytes<MODE>(NT), a, s);
    });
}

}  // namespace mz
