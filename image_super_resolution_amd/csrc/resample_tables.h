// Host-side coefficient tables of isr_resample_u8 (plain C++, no HIP, no allocation): Pillow's
// Imaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc restated in its order of
// operations, in double, so that every host gets the integers Pillow gets.  Included by capi.hip
// and by the stand-alone sanitizer program of tests/test_resample_cpu.py.
#pragma once
#include <math.h>
#include <stdint.h>

namespace isr {

constexpr int RESAMPLE_PRECISION_BITS = 32 - 8 - 2;  // 22 fractional bits
constexpr int RESAMPLE_MAX_SIZE = 16384;
constexpr int RESAMPLE_MAX_RATIO = 8;   // in/out and out/in <= 8
constexpr int RESAMPLE_MAX_KSIZE = 49;  // lanczos at ratio 8: ceil(3 * 8) * 2 + 1

inline double resample_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

inline double resample_support(int filter) {
    switch (filter) {
        case 1: return 0.5;
        case 2: return 1.0;
        case 3: return 1.0;
        case 4: return 2.0;
        case 5: return 3.0;
        default: return 0.0;
    }
}

inline double resample_weight(int filter, double x) {
    switch (filter) {
        case 1: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
        case 2:
            if (x < 0.0) x = -x;
            return x < 1.0 ? 1.0 - x : 0.0;
        case 3:
            if (x < 0.0) x = -x;
            if (x == 0.0) return 1.0;
            if (x >= 1.0) return 0.0;
            x = x * M_PI;
            return sin(x) / x * (0.54 + 0.46 * cos(x));
        case 4: {
            const double a = -0.5;
            if (x < 0.0) x = -x;
            if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
            if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
            return 0.0;
        }
        case 5: return (-3.0 <= x && x < 3.0) ? resample_sinc(x) * resample_sinc(x / 3) : 0.0;
        default: return 0.0;
    }
}

// 0 = supported; 1 unknown filter, 2 size out of [1, RESAMPLE_MAX_SIZE], 3 ratio out of [1/8, 8]
inline int resample_check(int filter, int in_size, int out_size) {
    if (filter < 0 || filter > 5) return 1;
    if (in_size < 1 || out_size < 1 || in_size > RESAMPLE_MAX_SIZE || out_size > RESAMPLE_MAX_SIZE) return 2;
    if ((long long)in_size > (long long)out_size * RESAMPLE_MAX_RATIO ||
        (long long)out_size > (long long)in_size * RESAMPLE_MAX_RATIO)
        return 3;
    return 0;
}

// taps per output pixel (the row length of the coefficient table); arguments already checked
inline int resample_ksize(int filter, int in_size, int out_size) {
    if (filter == 0) return 1;
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(resample_support(filter) * filterscale) * 2 + 1;
}

// bounds [out][2] = first source index, tap count; coeffs [out][ksize], rows zero-padded
inline void resample_tables(int filter, int in_size, int out_size, int32_t* bounds, int32_t* coeffs) {
    const int ksize = resample_ksize(filter, in_size, out_size);
    const double scale = (double)in_size / out_size;
    if (filter == 0) {
        // src = floor((dst + 0.5) * in / out) as Pillow's ImagingScaleAffine forms it: the source
        // coordinate starts at half a step and advances by repeated addition
        double xo = scale * 0.5;
        for (int xx = 0; xx < out_size; ++xx) {
            int xin = (int)xo;
            if (xin > in_size - 1) xin = in_size - 1;
            bounds[xx * 2 + 0] = xin;
            bounds[xx * 2 + 1] = 1;
            coeffs[xx] = 1 << RESAMPLE_PRECISION_BITS;
            xo += scale;
        }
        return;
    }
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = resample_support(filter) * filterscale;
    const double ss = 1.0 / filterscale;
    double k[RESAMPLE_MAX_KSIZE];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax > ksize) xmax = ksize;  // cannot happen (ksize = 2 ceil(support) + 1); keeps k[] in bounds
        for (int x = 0; x < xmax; ++x) {
            const double w = resample_weight(filter, (x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        int32_t* row = coeffs + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            double w = k[x];
            if (ww != 0.0) w /= ww;
            row[x] = w < 0 ? (int)(-0.5 + w * (1 << RESAMPLE_PRECISION_BITS))
                           : (int)(0.5 + w * (1 << RESAMPLE_PRECISION_BITS));
        }
        for (int x = xmax; x < ksize; ++x) row[x] = 0;
        bounds[xx * 2 + 0] = xmin;
        bounds[xx * 2 + 1] = xmax;
    }
}

}  // namespace isr
