// Stand-alone host program around csrc/resample_tables.h (tests/test_resample_cpu.py builds it
// plain and with the address / undefined-behaviour sanitizers).  Arguments: triples
// "filter in_size out_size"; without arguments, a built-in sweep.  For every triple the tables go
// into heap buffers of exactly the documented size, and one line is printed:
//   filter in out check ksize bounds_sum coeffs_sum
// (check: resample_check's code; the sums are weighted by position so a moved entry shows).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "resample_tables.h"

static long long wsum(const std::vector<int32_t>& v) {
    long long s = 0;
    for (size_t i = 0; i < v.size(); ++i) s += (long long)v[i] * (long long)(i % 97 + 1);
    return s;
}

static int one(int f, int in, int out) {
    const int chk = isr::resample_check(f, in, out);
    if (chk != 0) {
        printf("%d %d %d %d 0 0 0\n", f, in, out, chk);
        return 0;
    }
    const int ks = isr::resample_ksize(f, in, out);
    if (ks < 1 || ks > isr::RESAMPLE_MAX_KSIZE) return 1;
    std::vector<int32_t> bounds((size_t)out * 2, -1), coeffs((size_t)out * ks, -1);
    isr::resample_tables(f, in, out, bounds.data(), coeffs.data());
    for (int x = 0; x < out; ++x) {  // what the kernel relies on
        const int first = bounds[(size_t)x * 2], count = bounds[(size_t)x * 2 + 1];
        if (first < 0 || count < 1 || count > ks || first + count > in) return 2;
    }
    printf("%d %d %d 0 %d %lld %lld\n", f, in, out, ks, wsum(bounds), wsum(coeffs));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        if ((argc - 1) % 3) return 64;
        for (int i = 1; i + 2 < argc; i += 3) {
            const int rc = one(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]));
            if (rc) return rc;
        }
        return 0;
    }
    static const int sizes[][2] = {{96, 24}, {96, 32}, {96, 48}, {70, 23}, {50, 17}, {32, 128}, {47, 141}, {53, 53},
                                   {53, 20}, {8, 1}, {1, 8}, {1, 1}, {7, 5}, {2, 7}, {16384, 2048}, {2048, 16384},
                                   {9, 1}, {1, 9}, {0, 4}, {4, 0}, {16385, 16385}};
    for (int f = -1; f <= 6; ++f)
        for (const auto& s : sizes) {
            const int rc = one(f, s[0], s[1]);
            if (rc) return rc;
        }
    return 0;
}
