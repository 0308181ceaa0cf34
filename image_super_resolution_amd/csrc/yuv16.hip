// isr_yuv420_to_rgb_16 / isr_rgb_to_yuv420_16: 10-bit 4:2:0 Y'CbCr video frames in 16-bit words (I420 or
// NV12 order; the sample at bit `shift` of its word: yuv420p10le, p010le) <-> planar RGB as uint16, as the
// head's normalised fp32 input (yuv -> rgb) or from the tail's fp32 tanh (rgb -> yuv), in the integer
// arithmetic include/isr.h states (coefficients by value in the descriptor, yuv_coeffs.h).  Pure
// streaming, no LDS, no table, one launch each; yuv.hip's form with words for bytes.
//
// A thread owns 2 luma rows x 16 columns = one chroma row segment of 8 samples.  Consecutive threads own
// consecutive segments of a row, so a wave reads and writes 2 KiB runs of the luma and uint16 RGB rows
// (2 x 16 B per lane), 4 KiB runs of fp32 RGB rows (4 x 16 B per lane) and 1 KiB runs of the I420 chroma
// rows (16 B per lane; NV12: 2 x 16 B).
//   yuv -> rgb  reads 2 x 32 B of luma and, for the vertical filter, chroma rows i-1, i, i+1 of both
//               planes; the horizontal filter needs one more chroma column on each side, which are word
//               loads of lines the neighbouring lanes fetch anyway.  Writes 3 planes x 2 rows.
//   rgb -> yuv  reads 3 planes x 2 rows (left siting: and column x0 - 1, element loads), writes 2 x 32 B
//               of luma and 16 + 16 B (NV12: 32 B) of chroma.
// The 16-byte accesses are used per plane where w % 16 == 0 and that plane's address allows (the host
// passes one bit per plane); otherwise that plane moves as 2- or 4-byte elements, each guarded by the
// row's end, and partial segments at a ragged right edge take that path too.  Every index is formed from
// h, w and the thread's position, chroma neighbours are clamped to the plane and every sample is masked
// to its 10 bits: nothing a caller puts into the words or the coefficients can move an access.
#include "isr_common.h"
#include "dispatch.h"

namespace isr {

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int SEG = 16;  // luma columns per thread
constexpr int THREADS = 256;
constexpr int VEC_LUMA = 1, VEC_CHROMA = 2, VEC_RGB = 4;
constexpr int DEPTH = 10;  // the host refuses any other
constexpr int TOP = (1 << DEPTH) - 1, MID = 1 << (DEPTH - 1);
constexpr uint32_t MASK = (uint32_t)TOP;

// 16 words of a row segment, two to a dword
struct Seg {
    u32x4 v[2];
};

// bits [sh, sh + 10) of word k (0..15)
__device__ __forceinline__ int sample(const Seg& s, int k, int sh) {
    return (int)((s.v[k >> 3][(k >> 1) & 3] >> (16 * (k & 1) + sh)) & MASK);
}
__device__ __forceinline__ int sample8(u32x4 v, int k, int sh) {
    return (int)((v[k >> 1] >> (16 * (k & 1) + sh)) & MASK);
}

// clampd(acc >> SH), clamped BEFORE the shift (the same value: the flooring shift is monotone), as
// yuv.hip's shift_clamp8 and for its reason: clamp(x >> n, 0, top) on pairs is what hipcc turns into a
// packed shift-and-saturate instruction, which gave wrong bytes on the MI355X.
template <int SH>
__device__ __forceinline__ uint32_t shift_clamp(int v) {
    constexpr int HI = ((TOP + 1) << SH) - 1;  // SH <= 20: below 2^30
    v = v < 0 ? 0 : (v > HI ? HI : v);
    return (uint32_t)v >> SH;
}
template <int SH>
__device__ __forceinline__ uint32_t shift_clamp(long long v) {
    constexpr long long HI = ((long long)(TOP + 1) << SH) - 1;
    v = v < 0 ? 0 : (v > HI ? HI : v);
    return (uint32_t)v >> SH;
}

// ISR_RGB_NORM_F32: one division, one subtraction, one multiplication.  No multiplication feeds an
// addition here, so there is nothing to contract into a fused multiply-add; the pragma says so anyway.
__device__ __forceinline__ float normalise(int v, float mean, float inv_std) {
#pragma clang fp contract(off)
    const float q = (float)v / (float)TOP;
    const float c = q - mean;
    return c * inv_std;
}

// ISR_RGB_TANH_F32: the tail's uint8 quantiser at 10 bits.  add, mul, mul: again nothing to contract.
__device__ __forceinline__ uint32_t quantise(float t) {
#pragma clang fp contract(off)
    if (!(t > -1.f)) return 0u;  // NaN and -inf too
    if (t >= 1.f) return (uint32_t)TOP;
    const float a = t + 1.0f;
    const float b = a * 0.5f;
    const float q = rintf(b * (float)TOP);
    return (uint32_t)fminf(fmaxf(q, 0.f), (float)TOP);
}

// 16 words at p, of which the first `cols` exist (vec: all 16, p 16-byte aligned)
__device__ __forceinline__ Seg load_words(const uint16_t* p, int cols, bool vec) {
    Seg r;
    if (vec) {
        r.v[0] = reinterpret_cast<const u32x4*>(p)[0];
        r.v[1] = reinterpret_cast<const u32x4*>(p)[1];
        return r;
    }
    r.v[0] = r.v[1] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < SEG; ++k)
        if (k < cols) r.v[k >> 3][(k >> 1) & 3] |= (uint32_t)p[k] << (16 * (k & 1));
    return r;
}

__device__ __forceinline__ void store_words(uint16_t* p, const Seg& s, int cols, bool vec) {
    if (vec) {
        reinterpret_cast<u32x4*>(p)[0] = s.v[0];
        reinterpret_cast<u32x4*>(p)[1] = s.v[1];
        return;
    }
#pragma unroll
    for (int k = 0; k < SEG; ++k)
        if (k < cols) p[k] = (uint16_t)((s.v[k >> 3][(k >> 1) & 3] >> (16 * (k & 1))) & 0xffffu);
}

// 16 floats at p quantised to 10-bit values, two to a dword (a Seg with shift 0)
__device__ __forceinline__ Seg load_tanh(const float* p, int cols, bool vec) {
    Seg r;
    r.v[0] = r.v[1] = u32x4{0u, 0u, 0u, 0u};
    if (vec) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 t = reinterpret_cast<const f32x4*>(p)[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * q + e;
                r.v[k >> 3][(k >> 1) & 3] |= quantise(t[e]) << (16 * (k & 1));
            }
        }
        return r;
    }
#pragma unroll
    for (int k = 0; k < SEG; ++k)
        if (k < cols) r.v[k >> 3][(k >> 1) & 3] |= quantise(p[k]) << (16 * (k & 1));
    return r;
}

struct Geometry {
    int i, x0, cols;  // chroma row, first luma column, luma columns of this segment (even, 2..16)
};

__device__ __forceinline__ bool geometry(const isr_yuv16_desc& d, int groups, Geometry& g) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= (d.h >> 1) * groups) return false;
    g.i = t / groups;
    g.x0 = (t - g.i * groups) * SEG;
    g.cols = d.w - g.x0 < SEG ? d.w - g.x0 : SEG;
    return true;
}

// Chroma row `row` of frame f (words): samples j0-1 .. j0+8 of both planes, columns clamped to the plane.
__device__ __forceinline__ void load_chroma(const uint16_t* f, const isr_yuv16_desc& d, int row, int j0, bool vec,
                                            int* cu, int* cv) {
    const int wc = d.w >> 1, hw = d.h * d.w, sh = d.shift;
    const int jl = j0 > 0 ? j0 - 1 : 0, jr = j0 + 8 < wc ? j0 + 8 : wc - 1;
    if (d.layout == ISR_YUV_NV12) {
        const uint16_t* p = f + hw + (size_t)row * d.w;
        if (vec) {
            const u32x4 a = reinterpret_cast<const u32x4*>(p + 2 * j0)[0];
            const u32x4 b = reinterpret_cast<const u32x4*>(p + 2 * j0)[1];
#pragma unroll
            for (int k = 0; k < 8; ++k) {  // one dword = U (low word), V (high word)
                const uint32_t uv = k < 4 ? a[k & 3] : b[k & 3];
                cu[k + 1] = (int)((uv >> sh) & MASK);
                cv[k + 1] = (int)((uv >> (16 + sh)) & MASK);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = j0 + k < wc ? j0 + k : wc - 1;
                cu[k + 1] = (int)(((uint32_t)p[2 * j] >> sh) & MASK);
                cv[k + 1] = (int)(((uint32_t)p[2 * j + 1] >> sh) & MASK);
            }
        }
        cu[0] = (int)(((uint32_t)p[2 * jl] >> sh) & MASK);
        cv[0] = (int)(((uint32_t)p[2 * jl + 1] >> sh) & MASK);
        cu[9] = (int)(((uint32_t)p[2 * jr] >> sh) & MASK);
        cv[9] = (int)(((uint32_t)p[2 * jr + 1] >> sh) & MASK);
    } else {
        const uint16_t* pu = f + hw + (size_t)row * wc;
        const uint16_t* pv = pu + (hw >> 2);
        if (vec) {
            const u32x4 u = *reinterpret_cast<const u32x4*>(pu + j0), v = *reinterpret_cast<const u32x4*>(pv + j0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                cu[k + 1] = sample8(u, k, sh);
                cv[k + 1] = sample8(v, k, sh);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = j0 + k < wc ? j0 + k : wc - 1;
                cu[k + 1] = (int)(((uint32_t)pu[j] >> sh) & MASK);
                cv[k + 1] = (int)(((uint32_t)pv[j] >> sh) & MASK);
            }
        }
        cu[0] = (int)(((uint32_t)pu[jl] >> sh) & MASK);
        cv[0] = (int)(((uint32_t)pv[jl] >> sh) & MASK);
        cu[9] = (int)(((uint32_t)pu[jr] >> sh) & MASK);
        cv[9] = (int)(((uint32_t)pv[jr] >> sh) & MASK);
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

template <int SITING, int KIND>
__global__ __launch_bounds__(THREADS) void yuv420_to_rgb16_kernel(const isr_yuv16_desc d, const int groups,
                                                                  const int vec) {
    Geometry g;
    if (!geometry(d, groups, g)) return;
    constexpr int LOGD = SITING == ISR_YUV_SITING_LEFT ? 3 : 4, D = 1 << LOGD;
    const int hc = d.h >> 1, hw = d.h * d.w, sh = d.shift;
    const bool whole = g.cols == SEG;
    const uint16_t* f = (const uint16_t*)d.src + (size_t)blockIdx.y * ((size_t)hw + (hw >> 1));
    const size_t out0 = (size_t)blockIdx.y * 3 * (size_t)hw;  // in elements of either RGB kind
    const int j0 = g.x0 >> 1;
    const int im = g.i > 0 ? g.i - 1 : 0, ip = g.i + 1 < hc ? g.i + 1 : hc - 1;
    const bool vc = whole && (vec & VEC_CHROMA), vr = whole && (vec & VEC_RGB);

    Seg luma[2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
        luma[r] = load_words(f + (size_t)(2 * g.i + r) * d.w + g.x0, g.cols, whole && (vec & VEC_LUMA));
    int um[10], vm[10], u0[10], v0[10], up[10], vp[10];
    load_chroma(f, d, im, j0, vc, um, vm);
    load_chroma(f, d, g.i, j0, vc, u0, v0);
    load_chroma(f, d, ip, j0, vc, up, vp);

    const int oy = d.full_range ? 0 : 16 << (DEPTH - 8);
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
        const size_t row0 = out0 + (size_t)(2 * g.i + r) * d.w + g.x0;
        Seg words[3];  // ISR_RGB_U16: the row's 16 values per plane, stored after the loop
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // four columns at a time: one 16-byte fp32 store per plane
            uint32_t o[3][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = 4 * q + e;
                const uint32_t us = (uint32_t)(chroma_h<SITING>(au, x) - MID * D);
                const uint32_t vs = (uint32_t)(chroma_h<SITING>(av, x) - MID * D);
                // Each term in unsigned arithmetic (coefficients that are not isr_yuv_coeffs_depth's wrap)
                // and read as int32, which holds it (isr.h); the red and the blue sum pass 2^31 and are
                // formed in 64 bits, the green one fits int32.
                const int base = (int)(cy * (uint32_t)(D * (sample(luma[r], x, sh) - oy)) + (uint32_t)(32768 * D));
                o[0][e] = shift_clamp<ISR_YUV_BITS + LOGD>((long long)base + (long long)(int)(crv * vs));
                o[1][e] = shift_clamp<ISR_YUV_BITS + LOGD>((int)((uint32_t)base + cgu * us + cgv * vs));
                o[2][e] = shift_clamp<ISR_YUV_BITS + LOGD>((long long)base + (long long)(int)(cbu * us));
            }
            if constexpr (KIND == ISR_RGB_NORM_F32) {
                float* out = (float*)d.dst;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float* p = out + row0 + (size_t)c * hw + 4 * q;
                    f32x4 x4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) x4[e] = normalise((int)o[c][e], d.mean[c], d.inv_std[c]);
                    if (vr) {
                        *reinterpret_cast<f32x4*>(p) = x4;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (4 * q + e < g.cols) p[e] = x4[e];
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    words[c].v[q >> 1][2 * (q & 1)] = o[c][0] | (o[c][1] << 16);
                    words[c].v[q >> 1][2 * (q & 1) + 1] = o[c][2] | (o[c][3] << 16);
                }
            }
        }
        if constexpr (KIND == ISR_RGB_U16) {
#pragma unroll
            for (int c = 0; c < 3; ++c) store_words((uint16_t*)d.dst + row0 + (size_t)c * hw, words[c], g.cols, vr);
        }
    }
}

template <int SITING, int KIND>
__global__ __launch_bounds__(THREADS) void rgb_to_yuv420_16_kernel(const isr_yuv16_desc d, const int groups,
                                                                   const int vec) {
    Geometry g;
    if (!geometry(d, groups, g)) return;
    constexpr int LOGD = SITING == ISR_YUV_SITING_LEFT ? 3 : 2, D = 1 << LOGD;
    const int wc = d.w >> 1, hw = d.h * d.w, sh = d.shift;
    const bool whole = g.cols == SEG;
    const size_t in0 = (size_t)blockIdx.y * 3 * (size_t)hw;  // in elements of either RGB kind
    uint16_t* f = (uint16_t*)d.dst + (size_t)blockIdx.y * ((size_t)hw + (hw >> 1));
    const int j0 = g.x0 >> 1, nc = g.cols >> 1;
    const int xl = g.x0 > 0 ? g.x0 - 1 : 0;
    const bool vr = whole && (vec & VEC_RGB);

    Seg p[3][2];   // 10-bit values in the low bits of each word
    int left[3];   // column x0 - 1 summed over the two rows (left siting)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t row = in0 + ((size_t)c * d.h + 2 * g.i) * d.w;
        if constexpr (KIND == ISR_RGB_TANH_F32) {
            const float* in = (const float*)d.src + row;
            p[c][0] = load_tanh(in + g.x0, g.cols, vr);
            p[c][1] = load_tanh(in + d.w + g.x0, g.cols, vr);
            left[c] = SITING == ISR_YUV_SITING_LEFT ? (int)quantise(in[xl]) + (int)quantise(in[d.w + xl]) : 0;
        } else {
            const uint16_t* in = (const uint16_t*)d.src + row;
            p[c][0] = load_words(in + g.x0, g.cols, vr);
            p[c][1] = load_words(in + d.w + g.x0, g.cols, vr);
            left[c] = SITING == ISR_YUV_SITING_LEFT ? (int)(in[xl] & MASK) + (int)(in[d.w + xl] & MASK) : 0;
        }
    }

    const uint32_t oy = d.full_range ? 0u : 16u << (DEPTH - 8);
    uint32_t fw[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fw[k] = (uint32_t)d.fwd[k];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        Seg o;
        o.v[0] = o.v[1] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int x = 0; x < SEG; ++x) {
            const uint32_t acc = fw[0] * (uint32_t)sample(p[0][r], x, 0) + fw[1] * (uint32_t)sample(p[1][r], x, 0) +
                                 fw[2] * (uint32_t)sample(p[2][r], x, 0) + (oy << ISR_YUV_BITS) + 32768u;
            o.v[x >> 3][(x >> 1) & 3] |= (shift_clamp<ISR_YUV_BITS>((int)acc) << sh) << (16 * (x & 1));
        }
        store_words(f + (size_t)(2 * g.i + r) * d.w + g.x0, o, g.cols, whole && (vec & VEC_LUMA));
    }

    uint32_t cu[8], cv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int a = sample(p[c][0], 2 * j, 0) + sample(p[c][1], 2 * j, 0);
            const int b = sample(p[c][0], 2 * j + 1, 0) + sample(p[c][1], 2 * j + 1, 0);
            if constexpr (SITING == ISR_YUV_SITING_LEFT) {
                const int before = j == 0 ? left[c] : sample(p[c][0], 2 * j - 1, 0) + sample(p[c][1], 2 * j - 1, 0);
                s[c] = (uint32_t)(before + 2 * a + b);
            } else {
                s[c] = (uint32_t)(a + b);
            }
        }
        const uint32_t bias = (uint32_t)(MID * 65536 * D + 32768 * D);
        cu[j] = shift_clamp<ISR_YUV_BITS + LOGD>((int)(fw[3] * s[0] + fw[4] * s[1] + fw[5] * s[2] + bias)) << sh;
        cv[j] = shift_clamp<ISR_YUV_BITS + LOGD>((int)(fw[6] * s[0] + fw[7] * s[1] + fw[8] * s[2] + bias)) << sh;
    }
    const bool vc = whole && (vec & VEC_CHROMA);
    if (d.layout == ISR_YUV_NV12) {
        Seg o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j >> 2][j & 3] = cu[j] | (cv[j] << 16);
        store_words(f + hw + (size_t)g.i * d.w + g.x0, o, g.cols, vc);
    } else {
        u32x4 ou, ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ou[j] = cu[2 * j] | (cu[2 * j + 1] << 16);
            ov[j] = cv[2 * j] | (cv[2 * j + 1] << 16);
        }
        uint16_t* pu = f + hw + (size_t)g.i * wc + j0;
        uint16_t* pv = pu + (hw >> 2);
        if (vc) {
            *reinterpret_cast<u32x4*>(pu) = ou;
            *reinterpret_cast<u32x4*>(pv) = ov;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nc) {
                    pu[j] = (uint16_t)cu[j];
                    pv[j] = (uint16_t)cv[j];
                }
        }
    }
}

// one bit per plane kind: 16-byte accesses on the luma rows, the chroma rows and the RGB rows.  With
// w % 16 == 0 every row, plane and frame stride is a multiple of 16 bytes, so a plane keeps the alignment
// of its first byte.
int vec_bits(const isr_yuv16_desc* d, const void* frames, const void* rgb) {
    if (d->w % SEG) return 0;
    const size_t hw = (size_t)d->h * d->w;
    const uintptr_t y = (uintptr_t)frames, u = y + 2 * hw, v = u + hw / 2;
    int bits = 0;
    if (y % 16 == 0) bits |= VEC_LUMA;
    if (d->layout == ISR_YUV_NV12 ? u % 16 == 0 : (u % 16 == 0 && v % 16 == 0)) bits |= VEC_CHROMA;
    if ((uintptr_t)rgb % 16 == 0) bits |= VEC_RGB;
    return bits;
}

template <int KIND>
void launch_to_rgb(const isr_yuv16_desc* d, dim3 grid, int groups, int vec, hipStream_t s) {
    if (d->siting == ISR_YUV_SITING_LEFT)
        hipLaunchKernelGGL((yuv420_to_rgb16_kernel<ISR_YUV_SITING_LEFT, KIND>), grid, dim3(THREADS), 0, s, *d, groups, vec);
    else
        hipLaunchKernelGGL((yuv420_to_rgb16_kernel<ISR_YUV_SITING_CENTER, KIND>), grid, dim3(THREADS), 0, s, *d, groups,
                           vec);
}

template <int KIND>
void launch_to_yuv(const isr_yuv16_desc* d, dim3 grid, int groups, int vec, hipStream_t s) {
    if (d->siting == ISR_YUV_SITING_LEFT)
        hipLaunchKernelGGL((rgb_to_yuv420_16_kernel<ISR_YUV_SITING_LEFT, KIND>), grid, dim3(THREADS), 0, s, *d, groups, vec);
    else
        hipLaunchKernelGGL((rgb_to_yuv420_16_kernel<ISR_YUV_SITING_CENTER, KIND>), grid, dim3(THREADS), 0, s, *d, groups,
                           vec);
}

}  // namespace

// capi.hip has checked the descriptor: the kind belongs to the direction, depth is DEPTH
int yuv16_dispatch(const isr_yuv16_desc* d, int to_rgb, hipStream_t s) {
    const int groups = (d->w + SEG - 1) / SEG;
    const long long items = (long long)(d->h / 2) * groups;
    const dim3 grid((unsigned)((items + THREADS - 1) / THREADS), (unsigned)d->n);
    if (to_rgb) {
        const int vec = vec_bits(d, d->src, d->dst);
        if (d->rgb_kind == ISR_RGB_NORM_F32) launch_to_rgb<ISR_RGB_NORM_F32>(d, grid, groups, vec, s);
        else launch_to_rgb<ISR_RGB_U16>(d, grid, groups, vec, s);
    } else {
        const int vec = vec_bits(d, d->dst, d->src);
        if (d->rgb_kind == ISR_RGB_TANH_F32) launch_to_yuv<ISR_RGB_TANH_F32>(d, grid, groups, vec, s);
        else launch_to_yuv<ISR_RGB_U16>(d, grid, groups, vec, s);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
