// isr_yuv420_to_rgb_u8 / isr_rgb_to_yuv420_u8: 8-bit 4:2:0 Y'CbCr video frames (I420 or NV12)
// <-> planar uint8 RGB, in the integer arithmetic include/isr.h states (coefficients by value in
// the descriptor, yuv_coeffs.h).  Pure streaming, no LDS, no table, one launch each.
//
// A thread owns 2 luma rows x 16 columns = one chroma row segment of 8 samples.  Consecutive
// threads own consecutive segments of a row, so a wave reads and writes 1 KiB runs of the luma and
// RGB rows (16 B per lane) and 512 B runs of the I420 chroma rows (8 B per lane; NV12: 16 B).
//   yuv -> rgb  reads 2 x 16 B of luma and, for the vertical filter, chroma rows i-1, i, i+1 of both
//               planes; the horizontal filter needs one more chroma column on each side (center
//               siting; left siting only the right one), which are byte loads of lines the
//               neighbouring lanes fetch anyway.  Writes 3 planes x 2 rows x 16 B.
//   rgb -> yuv  reads 3 planes x 2 rows x 16 B (left siting: and column x0 - 1, byte loads), writes
//               2 x 16 B of luma and 8 + 8 B (NV12: 16 B) of chroma.
// The 16- and 8-byte accesses are used per plane where w % 16 == 0 and that plane's address allows
// (the host passes one bit per plane); otherwise that plane moves as bytes, each guarded by the
// row's end, and partial segments at a ragged right edge take that path too.  Every index is formed
// from h, w and the thread's position, chroma neighbours are clamped to the plane: nothing a caller
// puts into the coefficients can move an access.
#include "isr_common.h"
#include "dispatch.h"

namespace isr {

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr int YUV_SEG = 16;  // luma columns per thread
constexpr int YUV_THREADS = 256;
constexpr int VEC_LUMA = 1, VEC_CHROMA = 2, VEC_RGB = 4;

__device__ __forceinline__ int byte16(u32x4 v, int k) { return (int)((v[k >> 2] >> (8 * (k & 3))) & 255u); }
__device__ __forceinline__ int byte8(u32x2 v, int k) { return (int)((v[k >> 2] >> (8 * (k & 3))) & 255u); }

// clamp8((int)acc >> SH) of a sum formed in unsigned arithmetic, clamped BEFORE the shift (the same
// value: the flooring shift is monotone).  Written this way on purpose: from clamp(x >> 16, 0, 255) on
// pairs hipcc (ROCm 7's LLVM) forms v_ashr_pk_u8_i32 and then ORs the next byte into bits 16..23 of its
// result as if they were zero, but on the MI355X that instruction leaves the destination's upper half as
// it was, so byte 2 of a packed word came out ORed with stale bits.  tests/test_yuv_resources.py checks
// that the instruction is not in this file's assembly.
template <int SH>
__device__ __forceinline__ uint32_t shift_clamp8(uint32_t acc) {
    constexpr int HI = (256 << SH) - 1;
    int v = (int)acc;
    v = v < 0 ? 0 : (v > HI ? HI : v);
    return (uint32_t)v >> SH;
}

// 16 bytes at p, of which the first `cols` exist (vec: all 16, p 16-byte aligned)
__device__ __forceinline__ u32x4 load_seg(const uint8_t* p, int cols, bool vec) {
    if (vec) return *reinterpret_cast<const u32x4*>(p);
    u32x4 r = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < YUV_SEG; ++k)
        if (k < cols) r[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return r;
}

__device__ __forceinline__ void store_seg(uint8_t* p, u32x4 v, int cols, bool vec) {
    if (vec) {
        *reinterpret_cast<u32x4*>(p) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < YUV_SEG; ++k)
        if (k < cols) p[k] = (uint8_t)byte16(v, k);
}

struct Geometry {
    int i, x0, cols;  // chroma row, first luma column, luma columns of this segment (even, 2..16)
};

__device__ __forceinline__ bool geometry(const isr_yuv_desc& d, int groups, Geometry& g) {
    const int t = blockIdx.x * YUV_THREADS + threadIdx.x;
    if (t >= (d.h >> 1) * groups) return false;
    g.i = t / groups;
    g.x0 = (t - g.i * groups) * YUV_SEG;
    g.cols = d.w - g.x0 < YUV_SEG ? d.w - g.x0 : YUV_SEG;
    return true;
}

// Chroma row `row` of frame f: samples j0-1 .. j0+8 of both planes, columns clamped to the plane.
__device__ __forceinline__ void load_chroma(const uint8_t* f, const isr_yuv_desc& d, int row, int j0, bool vec,
                                            int* cu, int* cv) {
    const int wc = d.w >> 1, hw = d.h * d.w;
    const int jl = j0 > 0 ? j0 - 1 : 0, jr = j0 + 8 < wc ? j0 + 8 : wc - 1;
    if (d.layout == ISR_YUV_NV12) {
        const uint8_t* p = f + hw + (size_t)row * d.w;
        if (vec) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(p + 2 * j0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                cu[k + 1] = byte16(v, 2 * k);
                cv[k + 1] = byte16(v, 2 * k + 1);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = j0 + k < wc ? j0 + k : wc - 1;
                cu[k + 1] = p[2 * j];
                cv[k + 1] = p[2 * j + 1];
            }
        }
        cu[0] = p[2 * jl];
        cv[0] = p[2 * jl + 1];
        cu[9] = p[2 * jr];
        cv[9] = p[2 * jr + 1];
    } else {
        const uint8_t* pu = f + hw + (size_t)row * wc;
        const uint8_t* pv = pu + (hw >> 2);
        if (vec) {
            const u32x2 u = *reinterpret_cast<const u32x2*>(pu + j0), v = *reinterpret_cast<const u32x2*>(pv + j0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                cu[k + 1] = byte8(u, k);
                cv[k + 1] = byte8(v, k);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = j0 + k < wc ? j0 + k : wc - 1;
                cu[k + 1] = pu[j];
                cv[k + 1] = pv[j];
            }
        }
        cu[0] = pu[jl];
        cv[0] = pv[jl];
        cu[9] = pu[jr];
        cv[9] = pv[jr];
    }
}

// numerator of luma column x (0..15) of the segment from the vertically filtered samples a[0..9]
// (a[k] = chroma column j0 - 1 + k)
template <int SITING>
__device__ __forceinline__ int chroma_h(const int* a, int x) {
    const int k = (x >> 1) + 1;
    if constexpr (SITING == ISR_YUV_SITING_LEFT) return (x & 1) ? a[k] + a[k + 1] : 2 * a[k];
    else return 3 * a[k] + ((x & 1) ? a[k + 1] : a[k - 1]);
}

template <int SITING>
__global__ __launch_bounds__(YUV_THREADS) void yuv420_to_rgb_kernel(const isr_yuv_desc d, const int groups,
                                                                    const int vec) {
    Geometry g;
    if (!geometry(d, groups, g)) return;
    constexpr int LOGD = SITING == ISR_YUV_SITING_LEFT ? 3 : 4, D = 1 << LOGD;
    const int hc = d.h >> 1, hw = d.h * d.w;
    const bool whole = g.cols == YUV_SEG;
    const uint8_t* f = d.src + (size_t)blockIdx.y * ((size_t)hw + (hw >> 1));
    uint8_t* out = d.dst + (size_t)blockIdx.y * 3 * (size_t)hw;
    const int j0 = g.x0 >> 1;
    const int im = g.i > 0 ? g.i - 1 : 0, ip = g.i + 1 < hc ? g.i + 1 : hc - 1;
    const bool vc = whole && (vec & VEC_CHROMA);

    u32x4 luma[2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
        luma[r] = load_seg(f + (size_t)(2 * g.i + r) * d.w + g.x0, g.cols, whole && (vec & VEC_LUMA));
    int um[10], vm[10], u0[10], v0[10], up[10], vp[10];
    load_chroma(f, d, im, j0, vc, um, vm);
    load_chroma(f, d, g.i, j0, vc, u0, v0);
    load_chroma(f, d, ip, j0, vc, up, vp);

    const int oy = d.full_range ? 0 : 16;
    const uint32_t cy = (uint32_t)d.inv[0], crv = (uint32_t)d.inv[1], cbu = (uint32_t)d.inv[2],
                   cgu = (uint32_t)d.inv[3], cgv = (uint32_t)d.inv[4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int au[10], av[10];  // the vertical filter: row 2i takes row i-1, row 2i+1 takes row i+1
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            au[k] = 3 * u0[k] + (r ? up[k] : um[k]);
            av[k] = 3 * v0[k] + (r ? vp[k] : vm[k]);
        }
        u32x4 o[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
        for (int x = 0; x < YUV_SEG; ++x) {
            const uint32_t us = (uint32_t)(chroma_h<SITING>(au, x) - 128 * D);
            const uint32_t vs = (uint32_t)(chroma_h<SITING>(av, x) - 128 * D);
            // sums in unsigned arithmetic (coefficients that are not isr_yuv_coeffs' wrap), read as int32
            const uint32_t base = cy * (uint32_t)(D * (byte16(luma[r], x) - oy)) + (uint32_t)(32768 * D);
            o[0][x >> 2] |= shift_clamp8<ISR_YUV_BITS + LOGD>(base + crv * vs) << (8 * (x & 3));
            o[1][x >> 2] |= shift_clamp8<ISR_YUV_BITS + LOGD>(base + cgu * us + cgv * vs) << (8 * (x & 3));
            o[2][x >> 2] |= shift_clamp8<ISR_YUV_BITS + LOGD>(base + cbu * us) << (8 * (x & 3));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            store_seg(out + ((size_t)c * d.h + 2 * g.i + r) * d.w + g.x0, o[c], g.cols, whole && (vec & VEC_RGB));
    }
}

template <int SITING>
__global__ __launch_bounds__(YUV_THREADS) void rgb_to_yuv420_kernel(const isr_yuv_desc d, const int groups,
                                                                    const int vec) {
    Geometry g;
    if (!geometry(d, groups, g)) return;
    constexpr int LOGD = SITING == ISR_YUV_SITING_LEFT ? 3 : 2, D = 1 << LOGD;
    const int wc = d.w >> 1, hw = d.h * d.w;
    const bool whole = g.cols == YUV_SEG;
    const uint8_t* in = d.src + (size_t)blockIdx.y * 3 * (size_t)hw;
    uint8_t* f = d.dst + (size_t)blockIdx.y * ((size_t)hw + (hw >> 1));
    const int j0 = g.x0 >> 1, nc = g.cols >> 1;
    const int xl = g.x0 > 0 ? g.x0 - 1 : 0;

    u32x4 p[3][2];
    int left[3];  // column x0 - 1 summed over the two rows (left siting)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t* row = in + ((size_t)c * d.h + 2 * g.i) * d.w;
        p[c][0] = load_seg(row + g.x0, g.cols, whole && (vec & VEC_RGB));
        p[c][1] = load_seg(row + d.w + g.x0, g.cols, whole && (vec & VEC_RGB));
        left[c] = SITING == ISR_YUV_SITING_LEFT ? (int)row[xl] + (int)row[d.w + xl] : 0;
    }

    const uint32_t oy = d.full_range ? 0u : 16u;
    uint32_t fw[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fw[k] = (uint32_t)d.fwd[k];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int x = 0; x < YUV_SEG; ++x) {
            const uint32_t acc = fw[0] * (uint32_t)byte16(p[0][r], x) + fw[1] * (uint32_t)byte16(p[1][r], x) +
                                 fw[2] * (uint32_t)byte16(p[2][r], x) + (oy << ISR_YUV_BITS) + 32768u;
            o[x >> 2] |= shift_clamp8<ISR_YUV_BITS>(acc) << (8 * (x & 3));
        }
        store_seg(f + (size_t)(2 * g.i + r) * d.w + g.x0, o, g.cols, whole && (vec & VEC_LUMA));
    }

    uint32_t cu[8], cv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int a = byte16(p[c][0], 2 * j) + byte16(p[c][1], 2 * j);
            const int b = byte16(p[c][0], 2 * j + 1) + byte16(p[c][1], 2 * j + 1);
            if constexpr (SITING == ISR_YUV_SITING_LEFT) {
                const int before = j == 0 ? left[c] : byte16(p[c][0], 2 * j - 1) + byte16(p[c][1], 2 * j - 1);
                s[c] = (uint32_t)(before + 2 * a + b);
            } else {
                s[c] = (uint32_t)(a + b);
            }
        }
        const uint32_t bias = (uint32_t)(128 * 65536 * D + 32768 * D);
        cu[j] = shift_clamp8<ISR_YUV_BITS + LOGD>(fw[3] * s[0] + fw[4] * s[1] + fw[5] * s[2] + bias);
        cv[j] = shift_clamp8<ISR_YUV_BITS + LOGD>(fw[6] * s[0] + fw[7] * s[1] + fw[8] * s[2] + bias);
    }
    const bool vc = whole && (vec & VEC_CHROMA);
    if (d.layout == ISR_YUV_NV12) {
        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j >> 1] |= (cu[j] | (cv[j] << 8)) << (16 * (j & 1));
        store_seg(f + hw + (size_t)g.i * d.w + g.x0, o, g.cols, vc);
    } else {
        u32x2 ou = {0u, 0u}, ov = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ou[j >> 2] |= cu[j] << (8 * (j & 3));
            ov[j >> 2] |= cv[j] << (8 * (j & 3));
        }
        uint8_t* pu = f + hw + (size_t)g.i * wc + j0;
        uint8_t* pv = pu + (hw >> 2);
        if (vc) {
            *reinterpret_cast<u32x2*>(pu) = ou;
            *reinterpret_cast<u32x2*>(pv) = ov;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nc) {
                    pu[j] = (uint8_t)byte8(ou, j);
                    pv[j] = (uint8_t)byte8(ov, j);
                }
        }
    }
}

// one bit per plane kind: 16-byte luma / RGB segments, 8-byte (I420) or 16-byte (NV12) chroma segments.
// With w % 16 == 0 every row, plane and frame stride keeps the alignment of the plane's first byte.
int vec_bits(const isr_yuv_desc* d, const uint8_t* frames, const uint8_t* rgb) {
    if (d->w % YUV_SEG) return 0;
    const size_t hw = (size_t)d->h * d->w;
    const uintptr_t y = (uintptr_t)frames, u = y + hw, v = u + hw / 4;
    int bits = 0;
    if (y % 16 == 0) bits |= VEC_LUMA;
    if (d->layout == ISR_YUV_NV12 ? u % 16 == 0 : (u % 8 == 0 && v % 8 == 0)) bits |= VEC_CHROMA;
    if ((uintptr_t)rgb % 16 == 0) bits |= VEC_RGB;
    return bits;
}

}  // namespace

int yuv_dispatch(const isr_yuv_desc* d, int to_rgb, hipStream_t s) {
    const int groups = (d->w + YUV_SEG - 1) / YUV_SEG;
    const long long items = (long long)(d->h / 2) * groups;
    const dim3 grid((unsigned)((items + YUV_THREADS - 1) / YUV_THREADS), (unsigned)d->n), block(YUV_THREADS);
    const bool left = d->siting == ISR_YUV_SITING_LEFT;
    if (to_rgb) {
        const int vec = vec_bits(d, d->src, d->dst);
        if (left) hipLaunchKernelGGL(yuv420_to_rgb_kernel<ISR_YUV_SITING_LEFT>, grid, block, 0, s, *d, groups, vec);
        else hipLaunchKernelGGL(yuv420_to_rgb_kernel<ISR_YUV_SITING_CENTER>, grid, block, 0, s, *d, groups, vec);
    } else {
        const int vec = vec_bits(d, d->dst, d->src);
        if (left) hipLaunchKernelGGL(rgb_to_yuv420_kernel<ISR_YUV_SITING_LEFT>, grid, block, 0, s, *d, groups, vec);
        else hipLaunchKernelGGL(rgb_to_yuv420_kernel<ISR_YUV_SITING_CENTER>, grid, block, 0, s, *d, groups, vec);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
