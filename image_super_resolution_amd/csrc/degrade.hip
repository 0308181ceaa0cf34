// Training-data degradations on the device, on planar uint8 RGB crops [n][3][h][w] (include/isr.h):
// the decoded pixels of a baseline 4:2:0 JPEG round trip (isr_jpeg_roundtrip), the moments of HLS
// lightness (isr_hls_l_moments) and ISO noise in HLS space (isr_iso_noise).  They are the second and
// third stage of the reference's Noisy_dataset (utils/datasets.py:374-377: albumentations ISONoise and
// ImageCompression), which there run on host workers through cv2.
//
// JPEG.  The decoded image is fully determined by libjpeg's colour conversion, chroma subsampling,
// DCT, quantisation, IDCT and chroma upsampling; no entropy coding is needed.  Two launches:
//   1. codec: one 8x8 block of one component per 8 lanes (a 64-lane wave holds eight blocks, a lane
//      one row in registers).  Colour-convert (and for chroma average 2x2) on the load, row DCT in
//      registers, transpose through LDS, column DCT, quantise + dequantise, column IDCT, transpose
//      back, row IDCT, round, and store Y and the quarter-size Cb / Cr planes to the workspace.
//   2. finish: libjpeg's "fancy" triangle upsample of Cb / Cr (it crosses block and MCU borders,
//      hence the second launch), fixed-point YCbCr -> RGB, 8 pixels per thread.
// An image whose quality is 0 is skipped by 1 and copied from the source by 2.
//
// The coefficients (u, v) in {0, 4}^2 have cosines +-1/sqrt(2) only: they are integer sums / 8, land
// exactly on quantisation ties in flat regions, and a float product breaks those ties at random.
// Both transforms carry these four as integers (exact in fp32), everything else is fp32.  The work
// is bound by bytes and launches, so there is no MFMA here.
#include <math.h>

#include "isr_common.h"
#include "dispatch.h"

namespace isr {

namespace {

// ---- JPEG round trip ---------------------------------------------------------------------------

constexpr int JT = 256;      // threads per workgroup of the codec: 4 waves
constexpr int JB = JT / 8;   // 8x8 blocks per workgroup
constexpr int JS = 72;       // floats per block in LDS: 64 + 8, so the column reads of a wave hit 64 banks

// IJG base tables (JPEG Annex K), natural order: [0] luminance, [1] chrominance
__constant__ uint8_t kBase[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
     14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
     24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct JpegArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* quality;
    uint8_t* ws;       // Y [n][h][w], Cb [n][h/2][w/2], Cr [n][h/2][w/2]
    int n, h, w;
    float m[8][8];     // m[u][x] = C(u)/2 cos((2x + 1) u pi / 16)
};

__device__ __forceinline__ int byte_of(uint32_t v, int k) { return (int)((v >> (8 * k)) & 255u); }
__device__ __forceinline__ float s4f(int k) { return ((k + 1) & 2) ? -1.f : 1.f; }  // sign of cos((2k+1) pi/4)

// quantiser step of coefficient (v, u): jpeg_quality_scaling + jpeg_add_quant_table (baseline)
__device__ __forceinline__ float quant_step(int chroma, int v, int u, int q) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int e = ((int)kBase[chroma][v * 8 + u] * s + 50) / 100;
    return (float)min(max(e, 1), 255);
}

__global__ __launch_bounds__(JT) void jpeg_codec_kernel(JpegArgs p) {
    __shared__ __attribute__((aligned(16))) float T[JB][JS];
    __shared__ float X[JB][8][2];

    const int img = blockIdx.y;
    int q = p.quality[img];
    if (q <= 0) return;  // uniform over the workgroup: the finish launch copies the source
    q = min(q, 100);

    const int t = threadIdx.x, lb = t >> 3, r = t & 7;
    const int bx8 = p.w >> 3, nY = (p.h >> 3) * bx8, nC = nY >> 2, total = nY + 2 * nC;
    const int blk = blockIdx.x * JB + lb;
    const bool live = blk < total;
    int comp = 0, bi = live ? blk : 0;
    if (bi >= nY) {
        comp = bi - nY >= nC ? 2 : 1;
        bi -= nY + (comp - 1) * nC;
    }
    const int pw = comp ? bx8 >> 1 : bx8;  // blocks per row of this component's plane
    const int byi = bi / pw, bxi = bi - byi * pw;
    const size_t plane = (size_t)p.h * p.w;
    const uint8_t* s = p.src + (size_t)img * 3 * plane;

    // one row of the block, level-shifted: integers in [-128, 127]
    int v[8];
    if (comp == 0) {
        const size_t o = (size_t)(byi * 8 + r) * p.w + (size_t)bxi * 8;
        const uint2 R = *reinterpret_cast<const uint2*>(s + o);
        const uint2 G = *reinterpret_cast<const uint2*>(s + plane + o);
        const uint2 B = *reinterpret_cast<const uint2*>(s + 2 * plane + o);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int rr = byte_of(x < 4 ? R.x : R.y, x & 3), gg = byte_of(x < 4 ? G.x : G.y, x & 3),
                      bb = byte_of(x < 4 ? B.x : B.y, x & 3);
            v[x] = ((19595 * rr + 38470 * gg + 7471 * bb + 32768) >> 16) - 128;
        }
    } else {
        // Cb / Cr of 2 x 16 source pixels, then h2v2: (sum of four + bias 1, 2, 1, 2, ...) >> 2
        const int cr_ = comp == 2;
        const int kr = cr_ ? 32768 : -11059, kg = cr_ ? -27439 : -21709, kb = cr_ ? -5329 : 32768;
        int sum[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) sum[x] = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const size_t o = (size_t)((byi * 8 + r) * 2 + dy) * p.w + (size_t)bxi * 16;
            const uint4 R = *reinterpret_cast<const uint4*>(s + o);
            const uint4 G = *reinterpret_cast<const uint4*>(s + plane + o);
            const uint4 B = *reinterpret_cast<const uint4*>(s + 2 * plane + o);
            const uint32_t Rw[4] = {R.x, R.y, R.z, R.w}, Gw[4] = {G.x, G.y, G.z, G.w}, Bw[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int rr = byte_of(Rw[x >> 2], x & 3), gg = byte_of(Gw[x >> 2], x & 3), bb = byte_of(Bw[x >> 2], x & 3);
                sum[x >> 1] += (kr * rr + kg * gg + kb * bb + (128 << 16) + 32767) >> 16;
            }
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = ((sum[x] + 1 + (x & 1)) >> 2) - 128;
    }

    // row DCT; columns 0 and 4 stay the raw integer sums (exact in fp32)
    {
        float g[8];
        int r0 = 0, r4 = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            r0 += v[x];
            r4 += ((x + 1) & 2) ? -v[x] : v[x];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float a = 0.f;
#pragma unroll
            for (int x = 0; x < 8; ++x) a += p.m[u][x] * (float)v[x];
            g[u] = a;
        }
        g[0] = (float)r0;
        g[4] = (float)r4;
        *reinterpret_cast<f32x4*>(&T[lb][r * 8]) = f32x4{g[0], g[1], g[2], g[3]};
        *reinterpret_cast<f32x4*>(&T[lb][r * 8 + 4]) = f32x4{g[4], g[5], g[6], g[7]};
    }
    __syncthreads();

    // column DCT of column u = r, quantise, dequantise, column IDCT
    {
        const int u = r;
        const bool exact = (u & 3) == 0;
        float g[8], F[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) g[y] = T[lb][y * 8 + u];
        float e0 = 0.f, e4 = 0.f;
        if (exact) {
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                e0 += g[y];            // integers below 2^14: exact
                e4 += s4f(y) * g[y];
                g[y] *= p.m[0][0];     // 1 / (2 sqrt 2): the row transform's scale for u = 0 and 4
            }
        }
#pragma unroll
        for (int vv = 0; vv < 8; ++vv) {
            float a = 0.f;
#pragma unroll
            for (int y = 0; y < 8; ++y) a += p.m[vv][y] * g[y];
            F[vv] = a;
        }
        if (exact) {
            F[0] = e0 * 0.125f;
            F[4] = e4 * 0.125f;
        }
#pragma unroll
        for (int vv = 0; vv < 8; ++vv) {
            const float step = quant_step(comp != 0, vv, u, q);
            F[vv] = roundf(F[vv] / step) * step;  // half away from zero; the product is an integer
        }
        __syncthreads();  // every column read of T is done
        if (exact) {
            // the four exact terms leave the float transform: pixel (y, x) gets (A(y) + s4(x) B(y)) / 8,
            // A from column 0 and B from column 4
#pragma unroll
            for (int y = 0; y < 8; ++y) X[lb][y][u >> 2] = F[0] + s4f(y) * F[4];
            F[0] = 0.f;
            F[4] = 0.f;
        }
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            float a = 0.f;
#pragma unroll
            for (int vv = 0; vv < 8; ++vv) a += p.m[vv][y] * F[vv];
            T[lb][y * 8 + u] = a;
        }
    }
    __syncthreads();

    // row IDCT of row r, + 128, round, clamp, store
    {
        const f32x4 h0 = *reinterpret_cast<const f32x4*>(&T[lb][r * 8]);
        const f32x4 h1 = *reinterpret_cast<const f32x4*>(&T[lb][r * 8 + 4]);
        const float hr[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        const float A = X[lb][r][0], B = X[lb][r][1];
        uint32_t w0 = 0, w1 = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) a += p.m[u][x] * hr[u];
            a += (A + s4f(x) * B) * 0.125f;
            const uint32_t o = (uint32_t)fminf(fmaxf(floorf(a + 128.5f), 0.f), 255.f);
            if (x < 4) w0 |= o << (8 * x);
            else w1 |= o << (8 * (x - 4));
        }
        if (live) {
            uint8_t* d;
            if (comp == 0) d = p.ws + (size_t)img * plane + (size_t)(byi * 8 + r) * p.w + (size_t)bxi * 8;
            else d = p.ws + (size_t)p.n * plane + (size_t)(comp - 1) * p.n * (plane >> 2) + (size_t)img * (plane >> 2) +
                     (size_t)(byi * 8 + r) * (p.w >> 1) + (size_t)bxi * 8;
            *reinterpret_cast<uint2*>(d) = uint2{w0, w1};
        }
    }
}

// 8 output pixels of one row per thread
__global__ __launch_bounds__(256) void jpeg_finish_kernel(JpegArgs p) {
    const int img = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x, w8 = p.w >> 3;
    if (idx >= p.h * w8) return;
    const int y = idx / w8, x0 = (idx - y * w8) * 8;
    const size_t plane = (size_t)p.h * p.w;
    const size_t o = (size_t)img * 3 * plane + (size_t)y * p.w + x0;
    if (p.quality[img] <= 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<uint2*>(p.dst + o + c * plane) = *reinterpret_cast<const uint2*>(p.src + o + c * plane);
        return;
    }
    const uint2 Y = *reinterpret_cast<const uint2*>(p.ws + (size_t)img * plane + (size_t)y * p.w + x0);
    const int hc = p.h >> 1, wc = p.w >> 1, cy = y >> 1, cx0 = x0 >> 1;
    // libjpeg h2v2_fancy_upsample: 3:1 with the nearer chroma row, then 3:1 with the nearer column;
    // the row / column beyond the component's edge is the edge itself
    const int fy = (y & 1) ? min(cy + 1, hc - 1) : max(cy - 1, 0);
    const int xl = max(cx0 - 1, 0), xr = min(cx0 + 4, wc - 1);
    int c2[2][8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint8_t* C = p.ws + (size_t)p.n * plane + (size_t)c * p.n * (plane >> 2) + (size_t)img * (plane >> 2);
        const uint8_t* near = C + (size_t)cy * wc;
        const uint8_t* far = C + (size_t)fy * wc;
        const uint32_t nw = *reinterpret_cast<const uint32_t*>(near + cx0);
        const uint32_t fw = *reinterpret_cast<const uint32_t*>(far + cx0);
        int sm[6];
        sm[0] = 3 * near[xl] + far[xl];
        sm[5] = 3 * near[xr] + far[xr];
#pragma unroll
        for (int j = 0; j < 4; ++j) sm[1 + j] = 3 * byte_of(nw, j) + byte_of(fw, j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c2[c][2 * j] = (3 * sm[1 + j] + sm[j] + 8) >> 4;
            c2[c][2 * j + 1] = (3 * sm[1 + j] + sm[2 + j] + 7) >> 4;
        }
    }
    uint32_t out[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        const int yy = byte_of(x < 4 ? Y.x : Y.y, x & 3), cb = c2[0][x] - 128, cr = c2[1][x] - 128;
        // jdcolor's tables; >> of a negative int is arithmetic, as libjpeg's RIGHT_SHIFT
        const int rr = yy + ((91881 * cr + 32768) >> 16);
        const int gg = yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        const int bb = yy + ((116130 * cb + 32768) >> 16);
        out[0][x >> 2] |= (uint32_t)min(max(rr, 0), 255) << (8 * (x & 3));
        out[1][x >> 2] |= (uint32_t)min(max(gg, 0), 255) << (8 * (x & 3));
        out[2][x >> 2] |= (uint32_t)min(max(bb, 0), 255) << (8 * (x & 3));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<uint2*>(p.dst + o + c * plane) = uint2{out[c][0], out[c][1]};
}

// ---- HLS lightness moments ---------------------------------------------------------------------

constexpr int HT = 256;  // threads per block

struct MomentArgs {
    const uint8_t* src;
    unsigned long long* partials;  // [n][ISR_HLS_PARTIAL_BLOCKS][2]
    double* out;
    long long hw;
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum and sum of squares of max + min (an integer <= 510) over a grid-strided share of one image
__global__ __launch_bounds__(HT) void hls_moments_kernel(MomentArgs p) {
    __shared__ unsigned long long red[2][HT / 64];
    const int img = blockIdx.y, t = threadIdx.x;
    const uint8_t* s = p.src + (size_t)img * 3 * (size_t)p.hw;
    unsigned long long s1 = 0, s2 = 0;
    for (long long i = (long long)blockIdx.x * HT + t; i < p.hw; i += (long long)ISR_HLS_PARTIAL_BLOCKS * HT) {
        const int r = s[i], g = s[p.hw + i], b = s[2 * p.hw + i];
        const unsigned v = (unsigned)(max(max(r, g), b) + min(min(r, g), b));
        s1 += v;
        s2 += v * v;
    }
    s1 = wave_sum_u64(s1);
    s2 = wave_sum_u64(s2);
    if ((t & 63) == 0) {
        red[0][t >> 6] = s1;
        red[1][t >> 6] = s2;
    }
    __syncthreads();
    if (t < 2) {
        unsigned long long v = 0;
#pragma unroll
        for (int k = 0; k < HT / 64; ++k) v += red[t][k];
        p.partials[((size_t)img * ISR_HLS_PARTIAL_BLOCKS + blockIdx.x) * 2 + t] = v;
    }
}

// Per image: add the partials (integers: any order gives the same sums), then
// mean = S1 / (510 N), var = (N S2 - S1^2) / (510 N)^2 with the numerator formed in 128-bit integers.
__global__ __launch_bounds__(64) void hls_moments_finish_kernel(MomentArgs p) {
    const int img = blockIdx.x, l = threadIdx.x;
    const unsigned long long* q = p.partials + (size_t)img * ISR_HLS_PARTIAL_BLOCKS * 2;
    unsigned long long s1 = 0, s2 = 0;
    for (int i = l; i < ISR_HLS_PARTIAL_BLOCKS; i += 64) {
        s1 += q[2 * i];
        s2 += q[2 * i + 1];
    }
    s1 = wave_sum_u64(s1);
    s2 = wave_sum_u64(s2);
    if (l == 0) {
        const unsigned long long n = (unsigned long long)p.hw;
        const unsigned long long alo = n * s2, ahi = __umul64hi(n, s2);
        const unsigned long long blo = s1 * s1, bhi = __umul64hi(s1, s1);
        const unsigned long long dlo = alo - blo, dhi = ahi - bhi - (alo < blo ? 1ull : 0ull);  // >= 0 (Cauchy-Schwarz)
        const double num = (double)dhi * 18446744073709551616.0 + (double)dlo;
        const double den = 510.0 * (double)n;
        p.out[2 * img] = (double)s1 / den;
        p.out[2 * img + 1] = sqrt(num) / den;
    }
}

// ---- ISO noise ---------------------------------------------------------------------------------

struct IsoArgs {
    const uint8_t* src;
    uint8_t* dst;
    const float* lum;
    const float* hue;
    const int32_t* apply;
    long long hw;
};

// One pixel, every operation a single fp32 rounding in this order (the contract of include/isr.h;
// contraction into FMAs is off so that a restatement can follow it operation for operation).
__device__ __forceinline__ void iso_pixel(int ri, int gi, int bi, float lum, float hue, int& ro, int& go, int& bo) {
#pragma clang fp contract(off)
    const float r = (float)ri / 255.f, g = (float)gi / 255.f, b = (float)bi / 255.f;
    const float vmax = fmaxf(fmaxf(r, g), b), vmin = fminf(fminf(r, g), b);
    const float sm = vmax + vmin, d = vmax - vmin;
    float l = sm * 0.5f, h = 0.f, s = 0.f;
    if (d != 0.f) {
        s = l < 0.5f ? d / sm : d / (2.f - sm);
        const float k = 60.f / d;
        if (vmax == r) h = (g - b) * k;
        else if (vmax == g) h = (b - r) * k + 120.f;
        else h = (r - g) * k + 240.f;
        if (h < 0.f) h += 360.f;
    }
    h += hue;
    if (h < 0.f) h += 360.f;
    if (h > 360.f) h -= 360.f;
    l = l + (lum / 255.f) * (1.f - l);

    float rr = l, gg = l, bb = l;
    if (s != 0.f) {
        const float p2 = l <= 0.5f ? l * (1.f + s) : (l + s) - l * s;
        const float p1 = 2.f * l - p2;
        float hh = h * (1.f / 60.f);
        hh = hh - 6.f * floorf(hh * (1.f / 6.f));
        const float sec = fminf(fmaxf(floorf(hh), 0.f), 5.f);  // NaN -> 0: the index below stays in the table
        const float fr = hh - sec, dp = p2 - p1;
        const float fall = p1 + dp * (1.f - fr), rise = p1 + dp * fr;
        switch ((int)sec) {
            case 0: rr = p2; gg = rise; bb = p1; break;
            case 1: rr = fall; gg = p2; bb = p1; break;
            case 2: rr = p1; gg = p2; bb = rise; break;
            case 3: rr = p1; gg = fall; bb = p2; break;
            case 4: rr = rise; gg = p1; bb = p2; break;
            default: rr = p2; gg = p1; bb = fall; break;
        }
    }
    // clamp, then truncate toward zero (numpy's astype(uint8) after clip); NaN -> 0
    ro = (int)fminf(fmaxf(rr * 255.f, 0.f), 255.f);
    go = (int)fminf(fmaxf(gg * 255.f, 0.f), 255.f);
    bo = (int)fminf(fmaxf(bb * 255.f, 0.f), 255.f);
}

template <int V>  // pixels per thread: 4 (hw % 4 == 0, aligned buffers) or 1
__global__ __launch_bounds__(256) void iso_noise_kernel(IsoArgs p) {
    const int img = blockIdx.y;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= p.hw) return;
    const size_t base = (size_t)img * 3 * (size_t)p.hw + (size_t)i;
    const size_t nb = (size_t)img * (size_t)p.hw + (size_t)i;
    const bool on = p.apply[img] != 0;
    if constexpr (V == 4) {
        uint32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = *reinterpret_cast<const uint32_t*>(p.src + base + (size_t)k * p.hw);
        if (on) {
            const f32x4 lum = *reinterpret_cast<const f32x4*>(p.lum + nb);
            const f32x4 hue = *reinterpret_cast<const f32x4*>(p.hue + nb);
            uint32_t o[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int ro, go, bo;
                iso_pixel(byte_of(c[0], j), byte_of(c[1], j), byte_of(c[2], j), lum[j], hue[j], ro, go, bo);
                o[0] |= (uint32_t)ro << (8 * j);
                o[1] |= (uint32_t)go << (8 * j);
                o[2] |= (uint32_t)bo << (8 * j);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = o[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<uint32_t*>(p.dst + base + (size_t)k * p.hw) = c[k];
    } else {
        int r = p.src[base], g = p.src[base + p.hw], b = p.src[base + 2 * p.hw];
        if (on) iso_pixel(r, g, b, p.lum[nb], p.hue[nb], r, g, b);
        p.dst[base] = (uint8_t)r;
        p.dst[base + p.hw] = (uint8_t)g;
        p.dst[base + 2 * p.hw] = (uint8_t)b;
    }
}

}  // namespace

size_t jpeg_roundtrip_workspace_bytes(const isr_jpeg_desc* d) {
    return (size_t)d->n * d->h * d->w * 3 / 2;  // Y plus two quarter-size chroma planes, uint8
}

int jpeg_roundtrip_dispatch(const isr_jpeg_desc* d, void* ws, size_t ws_bytes, hipStream_t s) {
    if (ws_bytes < jpeg_roundtrip_workspace_bytes(d)) return DISPATCH_WS_TOO_SMALL;
    JpegArgs p;
    p.src = d->src;
    p.dst = d->dst;
    p.quality = d->quality;
    p.ws = (uint8_t*)ws;
    p.n = d->n;
    p.h = d->h;
    p.w = d->w;
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) p.m[u][x] = (float)((u ? 0.5 : 0.5 * sqrt(0.5)) * cos((2 * x + 1) * u * pi / 16.0));
    const int blocks = (d->h / 16) * (d->w / 16) * 6;  // 4 Y + Cb + Cr per MCU
    hipLaunchKernelGGL(jpeg_codec_kernel, dim3((blocks + JB - 1) / JB, d->n), dim3(JT), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -1;
    const int items = d->h * (d->w / 8);
    hipLaunchKernelGGL(jpeg_finish_kernel, dim3((items + 255) / 256, d->n), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int hls_l_moments_dispatch(const isr_hls_moments_desc* d, hipStream_t s) {
    MomentArgs p;
    p.src = d->src;
    p.partials = (unsigned long long*)d->partials;
    p.out = d->out;
    p.hw = (long long)d->h * d->w;
    hipLaunchKernelGGL(hls_moments_kernel, dim3(ISR_HLS_PARTIAL_BLOCKS, d->n), dim3(HT), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(hls_moments_finish_kernel, dim3(d->n), dim3(64), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int iso_noise_dispatch(const isr_iso_noise_desc* d, hipStream_t s) {
    IsoArgs p;
    p.src = d->src;
    p.dst = d->dst;
    p.lum = d->lum_noise;
    p.hue = d->hue_noise;
    p.apply = d->apply;
    p.hw = (long long)d->h * d->w;
    const bool vec = p.hw % 4 == 0 && ((uintptr_t)d->src | (uintptr_t)d->dst) % 4 == 0 &&
                     ((uintptr_t)d->lum_noise | (uintptr_t)d->hue_noise) % 16 == 0;
    if (vec) {
        const long long items = p.hw / 4;
        hipLaunchKernelGGL(iso_noise_kernel<4>, dim3((unsigned)((items + 255) / 256), d->n), dim3(256), 0, s, p);
    } else {
        hipLaunchKernelGGL(iso_noise_kernel<1>, dim3((unsigned)((p.hw + 255) / 256), d->n), dim3(256), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
