// conv3s_kernel instantiations and launcher (the kernel: mz_conv3s.h).
#include "mz_conv3s.h"

namespace mz {

// persistent: a.persist workgroups; 16-bit types; EPI_STORE / EPI_D2S, or EPI_FUSEDMIX: the fused variant (a.wmix16 = PK_GATE16)
hipError_t launch_conv3s(int dtype, int mode, int nt, const ConvArgs& a, hipStream_t s) {
    if (!walk_ok(a) || a.persist <= 0 || (a.epi != EPI_STORE && a.epi != EPI_D2S && a.epi != EPI_FUSEDMIX)) return hipErrorInvalidValue;
    return dispatch<3, MODE_C3W16, MODE_C3W8>(dtype, nt, mode, [&](auto tt, auto n, auto m) {
        using TT = decltype(tt);
        constexpr int NT = decltype(n)::value, MODE = decltype(m)::value;
        if constexpr (TT::SZ == 2) {
            if (a.epi == EPI_FUSEDMIX) return launch_lds<conv3s_kernel<TT, NT, MODE, true>>(a.persist, 640, conv16_lds_bytes<MODE>(NT, true), a, s);
            return launch_lds<conv3s_kernel<TT, NT, MODE, false>>(a.persist, 640, conv16_lds_bytes<MODE>(NT, false), a, s);
        } else {
            return hipErrorInvalidValue;
        }
    });
}

}  // namespace mz
