// Host-only check of ultrazoom_amd/csrc/mz_feather.h (tests/test_feather_main_cpu.py builds it with plain g++ and the address and
// undefined-behaviour sanitizers and runs it; nothing of it is loaded into Python).  The header's host part compiled without HIP: for
// EVERY ramp length up to 2^20 the last weight is below 1, the first is rho itself and the weights grow; the ramp bounds at the ends
// of int; the blend and the uint8 code at their extremes.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "../ultrazoom_amd/csrc/mz_feather.h"

using namespace mz;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // ---- the ramp bounds ----
    CHECK(feather_ramp_ok(0) && feather_ramp_ok(1) && feather_ramp_ok(kFeatherMaxRamp) && kFeatherMaxRamp == 1 << 20);
    CHECK(!feather_ramp_ok(-1) && !feather_ramp_ok(kFeatherMaxRamp + 1) && !feather_ramp_ok(imax) && !feather_ramp_ok(imin));
    CHECK(feather_rho(0) == 0.0 && feather_rho(1) == 0.5 && feather_rho(kFeatherMaxRamp) == 1.0 / 2097152.0);

    // ---- no ramp, and behind a ramp: positions up to the largest side and the end of int ----
    CHECK(feather_omega(0, feather_rho(0), 0) == 1.0 && feather_omega(0, feather_rho(0), imax) == 1.0);
    CHECK(feather_omega(1, 0.5, 0) == 0.5 && feather_omega(1, 0.5, 1) == 1.0 && feather_omega(1, 0.5, 1 << 28) == 1.0 && feather_omega(1, 0.5, imax) == 1.0);
    CHECK(feather_omega(kFeatherMaxRamp, feather_rho(kFeatherMaxRamp), kFeatherMaxRamp) == 1.0);
    CHECK(feather_omega(kFeatherMaxRamp, feather_rho(kFeatherMaxRamp), imax) == 1.0);

    // ---- every ramp: omega(n, n - 1) < 1, omega(n, 0) = rho, monotone; the whole ramp is walked for n <= 4096 and for the largest ones,
    // 65 positions from end to end for the rest ----
    double largest = 0.0;
    long long walked = 0;
    for (int n = 1; n <= kFeatherMaxRamp; ++n) {
        const double rho = feather_rho(n);
        const double last = feather_omega(n, rho, n - 1);
        if (last > largest) largest = last;
        if (!(last < 1.0) || !(feather_omega(n, rho, 0) == rho) || !(rho > 0.0) || feather_omega(n, rho, n) != 1.0) {
            printf("FAILED: ramp %d: last %.17g first %.17g rho %.17g\n", n, last, feather_omega(n, rho, 0), rho);
            ++failures;
            break;
        }
        const int samples = (n <= 4096 || n > kFeatherMaxRamp - 16) ? n : 65;
        int prev_k = -1;
        double prev = 0.0;
        for (int i = 0; i < samples; ++i) {
            const int k = samples == n ? i : (int)((long long)i * (n - 1) / 64);
            if (k == prev_k) continue;
            const double w = feather_omega(n, rho, k);
            ++walked;
            if (!(w > prev) || !(w < 1.0)) {
                printf("FAILED: ramp %d position %d: %.17g after %.17g\n", n, k, w, prev);
                ++failures;
                n = kFeatherMaxRamp;
                break;
            }
            prev = w;
            prev_k = k;
        }
    }
    CHECK(largest == 1.0 - 1.0 / 2097152.0);  // 0.99999952..: ramp 2^20, whose weights are exact
    CHECK(walked > 70000000);
    // the product of two weights is 1 only outside both ramps
    CHECK(feather_weight(largest, largest) < 1.0 && feather_weight(1.0, largest) == largest && feather_weight(1.0, 1.0) == 1.0);

    // ---- the blend and the code ----
    CHECK(feather_mix(1.0, 0.0, 0.25) == 0.25 && feather_mix(0.0, 1.0, 0.25) == 0.75 && feather_mix(0.5, 0.5, 0.3) == 0.5);
    CHECK(feather_mix(255.0, 0.0, largest) < 255.0 && feather_mix(0.0, 255.0, largest) > 0.0);
    CHECK(feather_mix(nan, 0.0, 0.5) != feather_mix(nan, 0.0, 0.5) && feather_mix(0.0, nan, 0.5) != feather_mix(0.0, nan, 0.5));
    {
        const double tiny = std::numeric_limits<double>::denorm_min();
        CHECK(feather_mix(tiny, 0.0, 0.5) == 0.0 && feather_mix(tiny, 0.0, largest) == tiny);  // below the subnormals: a zero, not a trap
    }
    CHECK(feather_code(0.0) == 0 && feather_code(0.49999) == 0 && feather_code(0.5) == 1 && feather_code(254.5) == 255 && feather_code(255.0) == 255);
    CHECK(feather_code(feather_mix(3.0, 1.0, 0.25)) == 2 && feather_code(feather_mix(1.0, 3.0, 0.25)) == 3);  // 1.5 and 2.5: a tie goes up
    if (failures) return 1;
    printf("feather header OK (%lld weights walked, the largest %.8f)\n", walked, largest);
    return 0;
}
