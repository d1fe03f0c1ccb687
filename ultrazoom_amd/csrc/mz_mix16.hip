// mix16_kernel / mix16b_kernel instantiations and launchers (the kernels: mz_mix16.h).
#include "mz_mix16.h"

namespace mz {

hipError_t launch_mix16(int dtype, const ConvArgs& a, hipStream_t s) {
    if (!walk_ok(a)) return hipErrorInvalidValue;
    if (a.nchunks16 <= 0 || a.nchunks16 % 12) return hipErrorInvalidValue;  // three stages of four K steps per loop turn
    const size_t lds = 2 * 4 * 12 * 1024;
    switch (dtype) {
        case DT_BF16: return launch_lds<mix16_kernel<TBF16>>(a.grid, 576, lds, a, s);
        case DT_F16: return launch_lds<mix16_kernel<TF16>>(a.grid, 576, lds, a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_mix16b(int dtype, const ConvArgs& a, hipStream_t s, int workgroups) {
    if (a.mtiles <= 0 || a.ntiles != 1 || workgroups <= 0) return hipErrorInvalidValue;
    if (a.nchunks16 != 12) return hipErrorInvalidValue;  // C = 192: twelve K steps over [x ; z], all of them the N tile's own
    const size_t lds = 3 * 4 * 12 * 1024;  // the whole gate matrix
    const int grid = a.mtiles < workgroups ? a.mtiles : workgroups;   // a.mtiles = 256-pixel tiles = 8 units each
    switch (dtype) {
        case DT_BF16: return launch_lds<mix16b_kernel<TBF16>>(grid, 512, lds, a, s);
        case DT_F16: return launch_lds<mix16b_kernel<TF16>>(grid, 512, lds, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mz
