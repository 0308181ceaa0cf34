// isr_blur_u8: the blur family of the LR degradation chain on uint8 planar RGB (include/isr.h): a
// k x k integer correlation with host-made 16-bit fixed-point taps (blur_taps.h; box, Gaussian,
// motion, or any table a C caller brings) under a reflect-101 border, or the exact k x k median
// under a replicated border, k in {3, 5, 7} per image; any other k copies the image through.
// One launch; one 256-thread block per (image, 32 x 32 output tile, all 3 channels):
//
//   1. the image's 49 taps go to LDS, and the tile plus a 3-pixel halo goes to LDS as uint8, the
//      border rule of the image's mode applied here (every source index is clamped to the image
//      after the rule, so nothing the per-image arrays hold can index outside it);
//   2. a thread makes 4 adjacent pixels of one row: per window row three LDS dwords (12 bytes, of
//      which it needs 4 + 2 * (k / 2)), int32 accumulators summed in unsigned arithmetic, one
//      dword store (bytes at a ragged right edge and where w % 4 != 0).  The loops are unrolled
//      over the image's own k (one instantiation per k, chosen by a block-uniform branch), the
//      k * k taps held in registers across the thread's three quads;
//   3. median: an 8-step binary search on the value per pixel, counting the window's bytes below
//      the probe; the window stays in registers as 3 * k dwords, no per-thread array is indexed
//      at run time.
//
// LDS: 3 * 38 rows * 40 B + 49 taps = 4.8 KB.  Rows are 10 dwords: a 32-lane half reads quads
// 0..7 of rows r, r + 4, r + 8, r + 12, whose first dwords are 40, 80, 120 dwords = 8, 16, 24
// banks apart (ds_read_b32 banks are dword mod 32), so the three reads per row are conflict-free.
#include "isr_common.h"
#include "dispatch.h"

namespace isr {

namespace {

constexpr int BL_TH = 32, BL_TW = 32, BL_QW = BL_TW / 4;
constexpr int BL_HALO = ISR_BLUR_MAX_K / 2;
constexpr int BL_ROWS = BL_TH + 2 * BL_HALO;
constexpr int BL_ROWDW = (BL_TW + 8) / 4;  // LDS byte column = x - x0 + 4: a quad's window starts on a dword
constexpr int BL_TAPS = ISR_BLUR_MAX_K * ISR_BLUR_MAX_K;

// source index of coordinate v on an axis of n >= 7 pixels; |v - [0, n)| <= 3 wherever the result is used
__device__ __forceinline__ int border(int v, int n, bool replicate) {
    if (!replicate) v = v < 0 ? -v : (v > n - 1 ? 2 * (n - 1) - v : v);
    return v < 0 ? 0 : (v > n - 1 ? n - 1 : v);
}

// byte p of the 12 bytes (d0, d1, d2); p is a constant wherever this is called
__device__ __forceinline__ uint32_t byte12(uint32_t d0, uint32_t d1, uint32_t d2, int p) {
    const uint32_t d = p < 4 ? d0 : (p < 8 ? d1 : d2);
    return (d >> (8 * (p & 3))) & 255u;
}

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
    const int v = (int)(acc + (1u << (ISR_BLUR_BITS - 1))) >> ISR_BLUR_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// 4 adjacent outputs from the window whose top-left dword is p[0]; t: the k x k taps
template <int K>
__device__ __forceinline__ uint32_t linear_quad(const uint32_t* p, const uint32_t* t) {
    constexpr int R = K / 2;
    uint32_t a[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
        const uint32_t d0 = p[dy * BL_ROWDW], d1 = p[dy * BL_ROWDW + 1], d2 = p[dy * BL_ROWDW + 2];
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += t[dy * K + dx] * byte12(d0, d1, d2, j + 4 + dx - R);
        }
    }
    return clip8(a[0]) | (clip8(a[1]) << 8) | (clip8(a[2]) << 16) | (clip8(a[3]) << 24);
}

// the median of each of the 4 windows: the smallest v with #(window <= v) >= K * K / 2 + 1, built
// bit by bit from the top (v keeps a bit while fewer than that many bytes lie below the probe)
template <int K>
__device__ __forceinline__ uint32_t median_quad(const uint32_t* p) {
    constexpr int R = K / 2, NEED = K * K / 2 + 1;
    uint32_t d[K][3];
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
        d[dy][0] = p[dy * BL_ROWDW];
        d[dy][1] = p[dy * BL_ROWDW + 1];
        d[dy][2] = p[dy * BL_ROWDW + 2];
    }
    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int bit = 7; bit >= 0; --bit) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t probe = v[j] | (1u << bit);
            int below = 0;
#pragma unroll
            for (int dy = 0; dy < K; ++dy) {
#pragma unroll
                for (int dx = 0; dx < K; ++dx) below += byte12(d[dy][0], d[dy][1], d[dy][2], j + 4 + dx - R) < probe;
            }
            v[j] = below < NEED ? probe : v[j];
        }
    }
    return v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
}

// K = 1: the copy-through of an image whose ksize is none of 3, 5, 7
template <int K, bool MEDIAN>
__device__ __forceinline__ void blur_tile(const uint32_t* tile, const int32_t* tp, uint8_t* dst, size_t plane, int x0,
                                          int y0, int h, int w, bool vec) {
    constexpr int R = K / 2;
    uint32_t t[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) t[i] = (uint32_t)tp[(i / K + BL_HALO - R) * ISR_BLUR_MAX_K + i % K + BL_HALO - R];
    for (int i = threadIdx.x; i < 3 * BL_TH * BL_QW; i += 256) {
        // lanes 0..31 of a wave: quads 0..7 of rows r, r + 4, r + 8, r + 12 (the bank layout above)
        const int q = i & 7, rest = i >> 5, c = rest >> 3;
        const int ly = ((rest >> 2) & 1) * 16 + ((i >> 3) & 3) * 4 + (rest & 3);
        const int y = y0 + ly, x = x0 + q * 4;
        if (y >= h || x >= w) continue;
        const uint32_t* p = tile + (c * BL_ROWS + ly + BL_HALO - R) * BL_ROWDW + q;
        uint32_t out;
        if (K == 1)
            out = p[1];
        else if (MEDIAN)
            out = median_quad<K>(p);
        else
            out = linear_quad<K>(p, t);
        const size_t o = (size_t)c * plane + (size_t)y * w + x;
        if (vec) {
            *reinterpret_cast<uint32_t*>(dst + o) = out;  // w % 4 == 0: the whole quad is inside
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < w) dst[o + j] = (uint8_t)(out >> (8 * j));
        }
    }
}

}  // namespace

__global__ __launch_bounds__(256) void blur_u8_kernel(isr_blur_desc d, int tiles_x, int tiles_y, int vec_out) {
    __shared__ uint32_t tile[3 * BL_ROWS * BL_ROWDW];
    __shared__ int32_t tp[BL_TAPS];

    const int tid = threadIdx.x;
    const int txi = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
    const int tyi = rest % tiles_y, img = rest / tiles_y;
    const int x0 = txi * BL_TW, y0 = tyi * BL_TH;
    const int h = d.h, w = d.w;

    int k = d.ksize[img];
    const bool median = d.median[img] != 0;
    if (k != 3 && k != 5 && k != 7) k = 1;
    if (tid < BL_TAPS) tp[tid] = d.taps[(size_t)img * BL_TAPS + tid];

    const size_t plane = (size_t)h * w;
    const uint8_t* src = d.src + (size_t)img * 3 * plane;
    for (int i = tid; i < 3 * BL_ROWS * BL_ROWDW; i += 256) {
        const int dq = i % BL_ROWDW, cr = i / BL_ROWDW, r = cr % BL_ROWS, c = cr / BL_ROWS;
        const uint8_t* row = src + (size_t)c * plane + (size_t)border(y0 + r - BL_HALO, h, median) * w;
        const int xs = x0 + dq * 4 - 4;
        uint32_t v;
        if (xs >= 0 && xs + 3 < w && ((uintptr_t)(row + xs) & 3) == 0) {
            v = *reinterpret_cast<const uint32_t*>(row + xs);
        } else {
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (uint32_t)row[border(xs + j, w, median)] << (8 * j);
        }
        tile[i] = v;
    }
    __syncthreads();

    uint8_t* dst = d.dst + (size_t)img * 3 * plane;
    const bool vec = vec_out != 0;
    if (k == 1) {
        blur_tile<1, false>(tile, tp, dst, plane, x0, y0, h, w, vec);
    } else if (median) {
        if (k == 3) blur_tile<3, true>(tile, tp, dst, plane, x0, y0, h, w, vec);
        else if (k == 5) blur_tile<5, true>(tile, tp, dst, plane, x0, y0, h, w, vec);
        else blur_tile<7, true>(tile, tp, dst, plane, x0, y0, h, w, vec);
    } else {
        if (k == 3) blur_tile<3, false>(tile, tp, dst, plane, x0, y0, h, w, vec);
        else if (k == 5) blur_tile<5, false>(tile, tp, dst, plane, x0, y0, h, w, vec);
        else blur_tile<7, false>(tile, tp, dst, plane, x0, y0, h, w, vec);
    }
}

int blur_u8_dispatch(const isr_blur_desc* d, hipStream_t s) {
    const int tiles_x = (d->w + BL_TW - 1) / BL_TW, tiles_y = (d->h + BL_TH - 1) / BL_TH;
    const long long blocks = (long long)d->n * tiles_x * tiles_y;
    if (blocks >= (1ll << 31)) return DISPATCH_UNSUPPORTED;
    const int vec_out = (d->w & 3) == 0 && ((uintptr_t)d->dst & 3) == 0;
    hipLaunchKernelGGL(blur_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, *d, tiles_x, tiles_y, vec_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
