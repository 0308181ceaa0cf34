// Stand-alone host program around csrc/yuv_coeffs.h (tests/test_yuv_cpu.py builds it plain and with
// the address / undefined-behaviour sanitizers).  A built-in sweep: every matrix id from -1 to 2 in
// limited and full range (full_range 0, 1 and 7: any non-zero value is full).  The coefficients go
// into heap buffers of exactly 9 and 5 entries, and one line is printed per case:
//   matrix full_range code fwd[0..8] inv[0..4]
// (code: yuv_coeffs' return value).
#include <stdio.h>

#include <vector>

#include "yuv_coeffs.h"

static int one(int matrix, int full_range) {
    std::vector<int32_t> fwd(9, -7), inv(5, -7);
    const int code = isr::yuv_coeffs(matrix, full_range, fwd.data(), inv.data());
    if (code == 0) {
        // what the contract promises: the chroma rows sum to 0, and the luma row to fix(sy)
        if (fwd[3] + fwd[4] + fwd[5] != 0 || fwd[6] + fwd[7] + fwd[8] != 0) return 2;
        if (fwd[0] + fwd[1] + fwd[2] != (full_range ? 65536 : 56284)) return 3;
    } else {
        for (int32_t v : fwd)
            if (v != -7) return 4;  // a refused call writes nothing
        for (int32_t v : inv)
            if (v != -7) return 4;
    }
    printf("%d %d %d", matrix, full_range, code);
    for (int32_t v : fwd) printf(" %d", v);
    for (int32_t v : inv) printf(" %d", v);
    printf("\n");
    return 0;
}

int main() {
    for (int matrix = -1; matrix <= 2; ++matrix)
        for (int full_range : {0, 1, 7})
            if (int rc = one(matrix, full_range)) return rc;
    return 0;
}
