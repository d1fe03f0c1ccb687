// What the host units of libmewzoom_hip.so share: this thread's error and last-kernel state (defined in mz_debug.cpp, read through
// mz_last_error() / mz_debug_last_kernel()) and the current device's CU count.
#pragma once
#include <hip/hip_runtime.h>

#include "mz_view_check.h"

namespace mz {

// kernel family of this thread's most recent convolution / mix launch (mz_debug_last_kernel(): the tests assert WHICH kernel they compare)
extern thread_local const char* g_last_kernel;

// writes mz_last_error()'s message and returns code
__attribute__((format(printf, 2, 3))) int fail(int code, const char* fmt, ...);
inline int fail(const Refusal& r) { return fail(r.code, "%s", r.msg); }  // what a check of mz_view_check.h, or a choice, refused
inline int hip_rc(hipError_t e, const char* what) { return e == hipSuccess ? MZ_OK : fail(MZ_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }
#define HIPCHK(expr) do { if (int rc_ = hip_rc((expr), #expr " failed")) return rc_; } while (0)

// The CUs of the CURRENT device, a multiple of 8 (one equal share per XCD; 0 if unknown), or the (negative) code of why there is
// none.  Asked once per device ordinal (kMaxDevices: mz_kernels.h; the launchers raise their kernels' dynamic-LDS limits themselves).
int device_cus();

}  // namespace mz
