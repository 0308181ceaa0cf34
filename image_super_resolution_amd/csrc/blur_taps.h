// Host-side tap tables of isr_blur_u8 (plain C++, no HIP, no allocation): the box, Gaussian and
// motion kernels of albumentations' Blur / GaussianBlur / MotionBlur as 7 x 7 tables of 16-bit
// fixed-point taps that sum to exactly 1 << 16.  fp64 throughout, one rounding per operation (no
// contraction into fused multiply-adds), so that every host gets the same integers.  Included by
// capi.hip; include/isr.h states the rules.
#pragma once
#include <math.h>
#include <stdint.h>

namespace isr {

constexpr int BLUR_MAX_K = 7;
constexpr int BLUR_BITS = 16;

// 0 = table made; 1 unknown kind, 2 bad ksize, 3 bad sigma / angle (not finite), 4 motion end points
// not integers inside the grid, 5 motion end points equal, 6 the centre tap would be negative
inline int blur_taps(int kind, int ksize, const double* params, int32_t* taps) {
#ifdef __clang__  // hipcc contracts a * b + c into an fma by default; another compiler gets -ffp-contract=off
#pragma clang fp contract(off)
#endif
    if (kind < 0 || kind > 2) return 1;
    if (ksize != 3 && ksize != 5 && ksize != 7) return 2;
    const int k = ksize, c = k / 2, off = (BLUR_MAX_K - k) / 2;
    double w[BLUR_MAX_K * BLUR_MAX_K];
    for (int i = 0; i < k * k; ++i) w[i] = 0.0;
    if (kind == 0) {
        for (int i = 0; i < k * k; ++i) w[i] = 1.0;
    } else if (kind == 1) {
        double sx = params[0], sy = params[1];
        const double angle = params[2];
        if (!isfinite(sx) || !isfinite(sy) || !isfinite(angle)) return 3;
        const double rule = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8;  // cv2's sigma for a given ksize
        if (sx <= 0.0) sx = rule;
        if (sy <= 0.0) sy = rule;
        const double ca = cos(angle), sa = sin(angle);
        for (int y = 0; y < k; ++y)
            for (int x = 0; x < k; ++x) {
                const double dx = x - c, dy = y - c;
                const double u = (dx * ca + dy * sa) / sx, v = (dy * ca - dx * sa) / sy;
                w[y * k + x] = exp(-0.5 * (u * u + v * v));
            }
    } else {
        int p[4];
        for (int i = 0; i < 4; ++i) {
            const double v = params[i];
            if (!(v >= 0.0 && v <= k - 1) || v != floor(v)) return 4;
            p[i] = (int)v;
        }
        if (p[0] == p[2] && p[1] == p[3]) return 5;
        // integer all-octant Bresenham from (x1, y1) to (x2, y2), both end points drawn
        int x = p[0], y = p[1];
        const int x2 = p[2], y2 = p[3];
        const int dx = x2 > x ? x2 - x : x - x2, dy = -(y2 > y ? y2 - y : y - y2);
        const int sx = x < x2 ? 1 : -1, sy = y < y2 ? 1 : -1;
        int err = dx + dy;
        for (;;) {
            w[y * k + x] = 1.0;
            if (x == x2 && y == y2) break;
            const int e2 = 2 * err;
            if (e2 >= dy) { err += dy; x += sx; }
            if (e2 <= dx) { err += dx; y += sy; }
        }
    }
    double sum = 0.0;
    for (int i = 0; i < k * k; ++i) sum += w[i];
    int32_t t[BLUR_MAX_K * BLUR_MAX_K];
    long long total = 0;
    for (int i = 0; i < k * k; ++i) {
        t[i] = (int32_t)floor(w[i] / sum * (double)(1 << BLUR_BITS) + 0.5);
        total += t[i];
    }
    const long long centre = t[c * k + c] + ((1ll << BLUR_BITS) - total);
    if (centre < 0) return 6;
    t[c * k + c] = (int32_t)centre;
    for (int i = 0; i < BLUR_MAX_K * BLUR_MAX_K; ++i) taps[i] = 0;
    for (int y = 0; y < k; ++y)
        for (int x = 0; x < k; ++x) taps[(y + off) * BLUR_MAX_K + x + off] = t[y * k + x];
    return 0;
}

}  // namespace isr
