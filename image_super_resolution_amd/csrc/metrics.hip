// Image-quality metrics on the device: squared error on RGB and on BT.601 luma, and SSIM on luma
// (isr_image_metrics, include/isr.h).  The reference has no metric code beyond the luma + crop of
// Ychannel (utils/datasets.py:159-166); the definitions are the literature's (Wang et al. 2004).
//
// One pass over both images.  A 512-thread block owns a 32 x 32 tile of SSIM window positions of
// one image: it stages the (32 + 10)^2 luma halo of both inputs in LDS (converted once: affine,
// clamp, quantise, luma), accumulating the squared errors of the pixels it owns on the way (each
// pixel belongs to exactly one block), then runs the separable 11-tap Gaussian over the five
// moment planes (x, y, x^2, y^2, xy), horizontal into LDS, vertical into registers, in two halves
// of 16 output rows so the horizontal planes take 33 KB instead of 54 KB (two blocks per CU).
//
// Everything after the load is fp64: E[x^2] - mu^2 at x ~ 200 cancels 4-5 digits, which fp32
// moments turn into 1e-4 on the SSIM of flat images.  No atomics: each block writes its three
// sums to its own workspace slot, a second launch adds them per image in a fixed order.
#include <math.h>

#include "isr_common.h"
#include "dispatch.h"

namespace isr {

namespace {

constexpr int MT = 32;            // window positions per tile side
constexpr int MW = 11;            // SSIM window
constexpr int MH = MT + MW - 1;   // 42: halo side
constexpr int MHALF = 16;         // output rows per vertical half
constexpr int MHR = MHALF + MW - 1;  // 26: horizontal rows a half needs
constexpr int MSLOT = 4;          // doubles per workspace slot (3 used; 32-byte slots)
constexpr int NT = 512;           // threads per block: 8 waves, two blocks per CU = 4 waves per SIMD

struct MetricsArgs {
    const void* a;
    const void* b;
    double* ws;
    int h, w, border, hc, wc;     // hc / wc: cropped extent
    int tiles_x, tiles_y;
    int clamp, quantize, exact;   // exact: both uint8 at scale 1/255, shift 0 → integer RGB sums
    double a_scale[3], a_shift[3], b_scale[3], b_shift[3];
    double g[MW];                 // the 1-D Gaussian, normalised to sum 1
};

struct ReduceArgs {
    const double* ws;
    double* out;
    int tiles;
    double px_rgb, px_y, windows;  // divisors: 3*hc*wc (x 255^2 when exact), hc*wc, valid windows
};

// one raw sample as a float (a uint8 value is exact in it)
template <bool U8>
__device__ __forceinline__ float load_px(const void* p, size_t i) {
    if constexpr (U8) return (float)reinterpret_cast<const uint8_t*>(p)[i];
    else return reinterpret_cast<const float*>(p)[i];
}

__device__ __forceinline__ double to_unit(double v, double scale, double shift, int clamp, int quantize) {
    double x = v * scale + shift;
    if (clamp) x = fmin(fmax(x, 0.0), 1.0);
    if (quantize) x = rint(x * 255.0) / 255.0;  // round half even: the value of the saved image
    return x;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

template <bool AU8, bool BU8>
__global__ __launch_bounds__(NT, 4) void image_metrics_kernel(MetricsArgs p) {
    __shared__ double X[MH][MH];         // luma * 255 of a
    __shared__ double Y[MH][MH];         // luma * 255 of b
    __shared__ double Hm[5][MHR][MT];    // horizontal pass of x, y, x^2, y^2, xy
    __shared__ double red[3][NT / 64];

    const int t = threadIdx.x;
    const int tx = blockIdx.x, ty = blockIdx.y, img = blockIdx.z;
    const int oy = ty * MT, ox = tx * MT;  // tile origin in cropped coordinates
    // pixels this block owns for the squared errors: its 32 x 32, and the last tile of a row /
    // column of tiles also the 10 + remainder pixels behind it (all inside its halo)
    const int own_h = ty == p.tiles_y - 1 ? MH : MT;
    const int own_w = tx == p.tiles_x - 1 ? MH : MT;
    const size_t plane = (size_t)p.h * p.w;
    const size_t base = (size_t)img * 3 * plane;

    // Stage the halo.  All 6 x NI loads of a thread are issued before the first is used, not one
    // pixel's loads per loop trip (dependent HBM round trips).
    // The address of a halo pixel outside the cropped image (ragged last tiles, the idle threads
    // of the last trip) is clamped into it, so every load is in bounds and unconditional; such
    // a pixel is then staged as 0 and counted nowhere.
    constexpr int NI = (MH * MH + NT - 1) / NT;  // 4 halo pixels per thread
    float va[NI][3], vb[NI][3];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int i = t + NT * j, r = i / MH, c = i - r * MH;
        const int gy = min(oy + r, p.hc - 1), gx = min(ox + c, p.wc - 1);
        const size_t o = base + (size_t)(gy + p.border) * p.w + (size_t)(gx + p.border);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            va[j][ch] = load_px<AU8>(p.a, o + ch * plane);
            vb[j][ch] = load_px<BU8>(p.b, o + ch * plane);
        }
    }
    double se_rgb = 0.0, se_y = 0.0;
    uint32_t se_int = 0;  // exact mode: at most NI pixels x 3 x 255^2 per thread
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int i = t + NT * j, r = i / MH, c = i - r * MH;
        if (i >= MH * MH) break;
        const int gy = oy + r, gx = ox + c;
        double ya = 0.0, yb = 0.0;
        if (gy < p.hc && gx < p.wc) {
            const double ar = to_unit(va[j][0], p.a_scale[0], p.a_shift[0], p.clamp, p.quantize);
            const double ag = to_unit(va[j][1], p.a_scale[1], p.a_shift[1], p.clamp, p.quantize);
            const double ab = to_unit(va[j][2], p.a_scale[2], p.a_shift[2], p.clamp, p.quantize);
            const double br = to_unit(vb[j][0], p.b_scale[0], p.b_shift[0], p.clamp, p.quantize);
            const double bg = to_unit(vb[j][1], p.b_scale[1], p.b_shift[1], p.clamp, p.quantize);
            const double bb = to_unit(vb[j][2], p.b_scale[2], p.b_shift[2], p.clamp, p.quantize);
            ya = 65.481 * ar + 128.553 * ag + 24.966 * ab + 16.0;
            yb = 65.481 * br + 128.553 * bg + 24.966 * bb + 16.0;
            if (r < own_h && c < own_w) {
                const double dr = ar - br, dg = ag - bg, db = ab - bb;
                // the luma difference from the channel differences: the +16 cancels, and two
                // rounded lumas are never subtracted
                const double dy = (65.481 * dr + 128.553 * dg + 24.966 * db) * (1.0 / 255.0);
                se_y += dy * dy;
                if (p.exact) {
                    const int ir = (int)va[j][0] - (int)vb[j][0], ig = (int)va[j][1] - (int)vb[j][1],
                              ib = (int)va[j][2] - (int)vb[j][2];
                    se_int += (uint32_t)(ir * ir + ig * ig + ib * ib);
                } else {
                    se_rgb += dr * dr + dg * dg + db * db;
                }
            }
        }
        X[r][c] = ya;
        Y[r][c] = yb;
    }
    if (p.exact) se_rgb = (double)se_int;  // an integer below 2^53 from here on: every sum is exact
    __syncthreads();

    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const int wy = p.hc - (MW - 1) - oy, wx = p.wc - (MW - 1) - ox;  // valid window positions from the origin
    double ssim = 0.0;
    for (int half = 0; half < 2; ++half) {
        const int r0 = half * MHALF;
        if (half) __syncthreads();  // the first half's vertical reads are done
        for (int i = t; i < MHR * MT; i += NT) {
            const int r = i / MT, c = i - r * MT;
            double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
            for (int k = 0; k < MW; ++k) {
                const double x = X[r0 + r][c + k], y = Y[r0 + r][c + k], g = p.g[k];
                const double gx_ = g * x, gy_ = g * y;
                m0 += gx_;
                m1 += gy_;
                m2 += gx_ * x;
                m3 += gy_ * y;
                m4 += gx_ * y;
            }
            Hm[0][r][c] = m0;
            Hm[1][r][c] = m1;
            Hm[2][r][c] = m2;
            Hm[3][r][c] = m3;
            Hm[4][r][c] = m4;
        }
        __syncthreads();
        static_assert(MHALF * MT % NT == 0, "whole trips over a half's window positions");
#pragma unroll
        for (int j = 0; j < MHALF * MT / NT; ++j) {
            const int r = (t >> 5) + (NT / MT) * j, c = t & 31;  // output row within the half, column
            if (r0 + r < wy && c < wx) {
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
                for (int k = 0; k < MW; ++k) {
                    const double g = p.g[k];
                    m0 += g * Hm[0][r + k][c];
                    m1 += g * Hm[1][r + k][c];
                    m2 += g * Hm[2][r + k][c];
                    m3 += g * Hm[3][r + k][c];
                    m4 += g * Hm[4][r + k][c];
                }
                const double vx = m2 - m0 * m0, vy = m3 - m1 * m1, cxy = m4 - m0 * m1;  // biased, window-weighted
                ssim += ((2.0 * m0 * m1 + C1) * (2.0 * cxy + C2)) / ((m0 * m0 + m1 * m1 + C1) * (vx + vy + C2));
            }
        }
    }

    // block reduction: wave shuffles, then LDS; one thread writes the block's slot
    se_rgb = wave_sum(se_rgb);
    se_y = wave_sum(se_y);
    ssim = wave_sum(ssim);
    if ((t & 63) == 0) {
        red[0][t >> 6] = se_rgb;
        red[1][t >> 6] = se_y;
        red[2][t >> 6] = ssim;
    }
    __syncthreads();
    if (t < 3) {
        double v = red[t][0];
#pragma unroll
        for (int k = 1; k < NT / 64; ++k) v += red[t][k];  // fixed order
        const size_t slot = ((size_t)img * p.tiles_y + ty) * p.tiles_x + tx;
        p.ws[slot * MSLOT + t] = v;
    }
}

// Per image: lane l adds slots l, l + 64, ... in order, then a fixed shuffle tree; same bits every call.
__global__ __launch_bounds__(64) void image_metrics_reduce_kernel(ReduceArgs p) {
    const int img = blockIdx.x, l = threadIdx.x;
    const double* ws = p.ws + (size_t)img * p.tiles * MSLOT;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = l; i < p.tiles; i += 64) {
        s0 += ws[(size_t)i * MSLOT + 0];
        s1 += ws[(size_t)i * MSLOT + 1];
        s2 += ws[(size_t)i * MSLOT + 2];
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (l == 0) {
        double* o = p.out + (size_t)img * 4;
        o[0] = s0 / p.px_rgb;
        o[1] = s1 / p.px_y;
        o[2] = s2 / p.windows;
        o[3] = p.windows;
    }
}

inline int tiles_of(int valid) { return (valid - (MW - 1) + MT - 1) / MT; }

}  // namespace

size_t image_metrics_workspace_bytes(const isr_metrics_desc* d) {
    const int hc = d->h - 2 * d->border, wc = d->w - 2 * d->border;
    return (size_t)d->n * tiles_of(hc) * tiles_of(wc) * MSLOT * sizeof(double);
}

int image_metrics_dispatch(const isr_metrics_desc* d, void* ws, size_t ws_bytes, hipStream_t s) {
    if (ws_bytes < image_metrics_workspace_bytes(d)) return DISPATCH_WS_TOO_SMALL;
    MetricsArgs p;
    p.a = d->a;
    p.b = d->b;
    p.ws = (double*)ws;
    p.h = d->h;
    p.w = d->w;
    p.border = d->border;
    p.hc = d->h - 2 * d->border;
    p.wc = d->w - 2 * d->border;
    p.tiles_y = tiles_of(p.hc);
    p.tiles_x = tiles_of(p.wc);
    p.clamp = d->clamp != 0;
    p.quantize = d->quantize != 0;
    bool unit_u8 = d->a_u8 && d->b_u8;
    for (int c = 0; c < 3; ++c) {
        p.a_scale[c] = d->a_scale[c];
        p.a_shift[c] = d->a_shift[c];
        p.b_scale[c] = d->b_scale[c];
        p.b_shift[c] = d->b_shift[c];
        unit_u8 = unit_u8 && d->a_scale[c] == 1.f / 255.f && d->b_scale[c] == 1.f / 255.f && d->a_shift[c] == 0.f &&
                  d->b_shift[c] == 0.f;
    }
    p.exact = unit_u8;  // values k/255: clamp and quantise leave them alone, (a - b)^2 * 255^2 is an integer
    double sum = 0.0;
    for (int k = 0; k < MW; ++k) {
        const double x = k - (MW - 1) / 2;
        p.g[k] = exp(-(x * x) / (2.0 * 1.5 * 1.5));
        sum += p.g[k];
    }
    for (int k = 0; k < MW; ++k) p.g[k] /= sum;

    const dim3 grid(p.tiles_x, p.tiles_y, d->n);
    if (d->a_u8 && d->b_u8) hipLaunchKernelGGL((image_metrics_kernel<true, true>), grid, dim3(NT), 0, s, p);
    else if (d->a_u8) hipLaunchKernelGGL((image_metrics_kernel<true, false>), grid, dim3(NT), 0, s, p);
    else if (d->b_u8) hipLaunchKernelGGL((image_metrics_kernel<false, true>), grid, dim3(NT), 0, s, p);
    else hipLaunchKernelGGL((image_metrics_kernel<false, false>), grid, dim3(NT), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -1;

    ReduceArgs r;
    r.ws = (const double*)ws;
    r.out = d->out;
    r.tiles = p.tiles_x * p.tiles_y;
    const double px = (double)p.hc * (double)p.wc;
    r.px_rgb = p.exact ? 3.0 * px * 65025.0 : 3.0 * px;
    r.px_y = px;
    r.windows = (double)(p.hc - (MW - 1)) * (double)(p.wc - (MW - 1));
    hipLaunchKernelGGL(image_metrics_reduce_kernel, dim3(d->n), dim3(64), 0, s, r);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
