// Host-side coefficients of isr_yuv420_to_rgb_u8 / isr_rgb_to_yuv420_u8 and of the 16-bit-word pair
// (plain C++, no HIP, no allocation): the BT.601 / BT.709 matrices in limited or full range as 16-bit
// fixed point, for samples of `depth` bits.  fp64 throughout, one rounding per operation (no contraction
// into fused multiply-adds), so that every host gets the same integers.  Included by capi.hip;
// include/isr.h states the rules.
#pragma once
#include <math.h>
#include <stdint.h>

namespace isr {

constexpr int YUV_BITS = 16;

// 0 = coefficients made; 1 unknown matrix; 2 a depth that is neither 8 nor 10.  Depth 8: the limited-range
// scales are 219 * 1 / 255 and 224 * 1 / 255, the doubles 219.0 / 255.0 and 224.0 / 255.0 exactly.
inline int yuv_coeffs_depth(int matrix, int full_range, int depth, int32_t* fwd, int32_t* inv) {
#ifdef __clang__  // hipcc contracts a * b + c into an fma by default; another compiler gets -ffp-contract=off
#pragma clang fp contract(off)
#endif
    if (matrix != 0 && matrix != 1) return 1;
    if (depth != 8 && depth != 10) return 2;
    const double up = (double)(1 << (depth - 8)), top = (double)((1 << depth) - 1);
    const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722;
    const double kg = 1.0 - kr - kb;
    const double sy = full_range ? 1.0 : 219.0 * up / top, sc = full_range ? 1.0 : 224.0 * up / top;
    const double one = (double)(1 << YUV_BITS);
    auto fix = [one](double v) { return (int32_t)floor(v * one + 0.5); };
    const double db = 2.0 * (1.0 - kb), dr = 2.0 * (1.0 - kr);
    int32_t f[9], v[5];
    // R and B entries rounded; G closes the row: Y sums to fix(sy), the chroma rows to 0
    f[0] = fix(sy * kr);
    f[2] = fix(sy * kb);
    f[1] = fix(sy) - f[0] - f[2];
    f[3] = fix(sc * -kr / db);
    f[5] = fix(sc * (1.0 - kb) / db);
    f[4] = -f[3] - f[5];
    f[6] = fix(sc * (1.0 - kr) / dr);
    f[8] = fix(sc * -kb / dr);
    f[7] = -f[6] - f[8];
    const double crv = dr / sc, cbu = db / sc;
    v[0] = fix(1.0 / sy);
    v[1] = fix(crv);
    v[2] = fix(cbu);
    v[3] = fix(-cbu * kb / kg);
    v[4] = fix(-crv * kr / kg);
    for (int i = 0; i < 9; ++i) fwd[i] = f[i];
    for (int i = 0; i < 5; ++i) inv[i] = v[i];
    return 0;
}

// 0 = coefficients made; 1 unknown matrix
inline int yuv_coeffs(int matrix, int full_range, int32_t* fwd, int32_t* inv) {
    return yuv_coeffs_depth(matrix, full_range, 8, fwd, inv);
}

}  // namespace isr
