// Stand-alone host program around csrc/blur_taps.h (tests/test_blur_cpu.py builds it plain and
// with the address / undefined-behaviour sanitizers).  A built-in sweep: every kind from -1 to 3,
// every ksize from 0 to 9, and per kind a parameter list that holds each refusal; for motion, every
// pair of end points of the grid.  The table goes into a heap buffer of exactly 49 entries, and one
// line is printed per case:
//   kind ksize p0 p1 p2 p3 code sum weighted_sum
// (code: blur_taps' return value; the weighted sum moves when an entry moves).
#include <math.h>
#include <stdio.h>

#include <vector>

#include "blur_taps.h"

static int one(int kind, int k, double p0, double p1, double p2, double p3) {
    const double params[4] = {p0, p1, p2, p3};
    std::vector<int32_t> taps(49, -7);
    const int code = isr::blur_taps(kind, k, params, taps.data());
    long long sum = 0, wsum = 0;
    if (code == 0) {
        for (size_t i = 0; i < taps.size(); ++i) {
            if (taps[i] < 0) return 2;  // what the contract promises
            sum += taps[i];
            wsum += (long long)taps[i] * (long long)(i + 1);
        }
        if (sum != 65536) return 3;
    } else {
        for (int32_t t : taps)
            if (t != -7) return 4;  // a refused call writes nothing
    }
    printf("%d %d %g %g %g %g %d %lld %lld\n", kind, k, p0, p1, p2, p3, code, sum, wsum);
    return 0;
}

int main() {
    static const double gauss[][3] = {{0.8, 0.8, 0.0}, {1.1, 1.1, 0.0}, {3.0, 0.6, 0.7},  {1.4, 1.4, 0.0}, {10.0, 10.0, 0.0},
                                      {0.0, 0.0, 0.0}, {-1.0, 2.0, 3.0}, {0.2, 3.0, 3.1}, {1e-3, 1e-3, 0.5}, {1e300, 1e-300, 1.0},
                                      {NAN, 1.0, 0.0}, {1.0, INFINITY, 0.0}, {1.0, 1.0, NAN}};
    for (int kind = -1; kind <= 3; ++kind)
        for (int k = 0; k <= 9; ++k) {
            if (kind == 1) {
                for (const auto& g : gauss)
                    if (int rc = one(kind, k, g[0], g[1], g[2], 0.0)) return rc;
            } else if (kind == 2) {
                const int n = k < 1 ? 1 : k;
                for (int a = -1; a <= n * n; ++a)
                    for (int b = -1; b <= n * n; ++b)
                        if (int rc = one(kind, k, a < 0 ? -1.0 : a % n, a < 0 ? 0.0 : a / n, b < 0 ? 0.5 : b % n,
                                         b < 0 ? 0.0 : (b == n * n ? n : b / n)))
                            return rc;
            } else if (int rc = one(kind, k, 0.0, 0.0, 0.0, 0.0)) {
                return rc;
            }
        }
    return 0;
}
