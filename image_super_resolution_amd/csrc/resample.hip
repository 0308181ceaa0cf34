// isr_resample_u8: Pillow's 8-bit Image.resize (Imaging/Resample.c) on the device, bit for bit,
// from host-made coefficient tables (resample_tables.h), with the training transform's epilogue
// fused in.  One launch; one 256-thread block per (image, 16 x 32 output tile, all 3 channels):
//
//   1. the tile's bounds and coefficients (of the image's filter variant) go to LDS, clamped to
//      the image, so nothing below can index outside it whatever the tables hold;
//   2. horizontal pass over the source rows the tile's y-bounds name, global uint8 -> LDS uint8
//      (the intermediate's rounding and clipping are part of Pillow's result).  A thread makes 4
//      adjacent pixels of one row and stores them as one dword;
//   3. vertical pass from LDS: a thread makes 4 adjacent output pixels, one dword read per tap
//      row, int32 accumulators as Pillow's;
//   4. epilogue: dst_u8 and / or Normalize -> lr_f32, and (integer ratio only) the HR tensor of
//      the s x s source region the tile owns, sr_transform_kernel's expressions.
//
// LDS: 3 * 176 rows * 36 B of intermediate (rows padded to 9 dwords: an odd stride, so the
// vertical pass's lanes, which start `ratio` rows apart, spread over the banks) + the tile's
// coefficient rows at an odd dword stride: 28.7 KB static, five blocks per CU.  The row bound 176
// covers the worst supported case, lanczos at ratio 8: 15 * 8 + 2 * 24 + 2 = 170 rows.
#include "isr_common.h"
#include "dispatch.h"

namespace isr {

namespace {

constexpr int RS_TH = 16, RS_TW = 32, RS_QW = RS_TW / 4;
constexpr int RS_MAXROWS = 176;
constexpr int RS_ROWDW = RS_QW + 1;  // intermediate row stride in dwords (odd)
constexpr int RS_MAXK = ISR_RESAMPLE_MAX_KSIZE;

__device__ __forceinline__ uint32_t clip8(int acc) {
    const int v = acc >> 22;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// mean / std of channel c by selects: a runtime index into the kernel argument would put the
// descriptor into scratch
__device__ __forceinline__ float pick3(const float* v, int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }

// one axis of the tile: `cnt` outputs from `o0` of variant tables (b, k) into LDS, clamped
__device__ __forceinline__ void stage_axis(const int32_t* b, const int32_t* k, int o0, int tile, int out_size,
                                           int in_size, int ksize, int kst, int32_t* lb, int32_t* lk) {
    for (int i = threadIdx.x; i < tile; i += 256) {
        int first = 0, count = 0;
        if (o0 + i < out_size) {
            first = b[(size_t)(o0 + i) * 2];
            count = b[(size_t)(o0 + i) * 2 + 1];
            first = first < 0 ? 0 : (first > in_size - 1 ? in_size - 1 : first);
            const int room = in_size - first < ksize ? in_size - first : ksize;
            count = count < 0 ? 0 : (count > room ? room : count);
        }
        lb[i * 2] = first;
        lb[i * 2 + 1] = count;
    }
    for (int i = threadIdx.x; i < tile * ksize; i += 256) {
        const int o = i / ksize, t = i - o * ksize;
        lk[o * kst + t] = o0 + o < out_size ? k[(size_t)(o0 + o) * ksize + t] : 0;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void resample_u8_kernel(isr_resample_desc d, int tiles_x, int tiles_y) {
    __shared__ uint32_t mid[3 * RS_MAXROWS * RS_ROWDW];
    __shared__ int32_t cx[RS_TW * RS_MAXK], cy[RS_TH * RS_MAXK];
    __shared__ int32_t bx[RS_TW * 2], by[RS_TH * 2];

    const int tid = threadIdx.x;
    const int txi = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
    const int tyi = rest % tiles_y, img = rest / tiles_y;
    const int ox0 = txi * RS_TW, oy0 = tyi * RS_TH;

    int v = d.filter_id ? d.filter_id[img] : 0;
    v = v < 0 ? 0 : (v > d.nf - 1 ? d.nf - 1 : v);
    const int ksx = d.ksize_x, ksy = d.ksize_y, kstx = ksx | 1, ksty = ksy | 1;
    stage_axis(d.bounds_x + (size_t)v * d.out_w * 2, d.coeffs_x + (size_t)v * d.out_w * ksx, ox0, RS_TW, d.out_w,
               d.in_w, ksx, kstx, bx, cx);
    stage_axis(d.bounds_y + (size_t)v * d.out_h * 2, d.coeffs_y + (size_t)v * d.out_h * ksy, oy0, RS_TH, d.out_h,
               d.in_h, ksy, ksty, by, cy);
    __syncthreads();

    // the source rows this tile needs: [y0, y0 + rows)
    int y0 = d.in_h, y1 = 0;
#pragma unroll
    for (int i = 0; i < RS_TH; ++i) {
        const int f = by[i * 2], c = by[i * 2 + 1];
        if (c > 0) {
            y0 = f < y0 ? f : y0;
            y1 = f + c > y1 ? f + c : y1;
        }
    }
    int rows = y1 - y0;
    rows = rows < 0 ? 0 : (rows > RS_MAXROWS ? RS_MAXROWS : rows);

    const size_t in_plane = (size_t)d.in_h * d.in_w, out_plane = (size_t)d.out_h * d.out_w;
    const uint8_t* src = d.src + (size_t)img * 3 * in_plane;

    // horizontal pass: (channel, source row, 4 adjacent outputs) per thread and step
    for (int i = tid; i < 3 * rows * RS_QW; i += 256) {
        const int xq = i % RS_QW, cr = i / RS_QW, c = cr / rows, r = cr - c * rows;
        const uint8_t* row = src + (size_t)c * in_plane + (size_t)(y0 + r) * d.in_w;
        // one pixel after the other, each with its own tap loop.  (Advancing the 4 pixels together, a
        // tap each per step under a per-pixel predicate, measured slower at 16 x 3 x 512^2: 79 against
        // 54 us for bicubic x4)
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = xq * 4 + j, first = bx[ox * 2], count = bx[ox * 2 + 1];
            const int32_t* k = cx + ox * kstx;
            int acc = 1 << 21;
            for (int t = 0; t < count; ++t) acc += (int)row[first + t] * k[t];
            packed |= clip8(acc) << (8 * j);
        }
        mid[(c * RS_MAXROWS + r) * RS_ROWDW + xq] = packed;
    }
    __syncthreads();

    // vertical pass + epilogue: (channel, output row, 4 adjacent outputs) per thread and step
    const bool vec_out = (d.out_w & 3) == 0;
    for (int i = tid; i < 3 * RS_TH * RS_QW; i += 256) {
        const int xq = i % RS_QW, oyl = (i / RS_QW) % RS_TH, c = i / (RS_QW * RS_TH);
        const int oy = oy0 + oyl, ox = ox0 + xq * 4;
        if (oy >= d.out_h || ox >= d.out_w) continue;
        int first = by[oyl * 2] - y0, count = by[oyl * 2 + 1];
        count = first + count > rows ? rows - first : count;
        const int32_t* k = cy + oyl * ksty;
        const uint32_t* col = mid + (c * RS_MAXROWS + first) * RS_ROWDW + xq;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
        for (int t = 0; t < count; ++t) {
            const uint32_t p = col[t * RS_ROWDW];
            const int w = k[t];
            a0 += (int)(p & 255u) * w;
            a1 += (int)((p >> 8) & 255u) * w;
            a2 += (int)((p >> 16) & 255u) * w;
            a3 += (int)(p >> 24) * w;
        }
        const uint32_t q[4] = {clip8(a0), clip8(a1), clip8(a2), clip8(a3)};
        const size_t o = ((size_t)img * 3 + c) * out_plane + (size_t)oy * d.out_w + ox;
        const float mean = pick3(d.mean, c), stdv = pick3(d.std, c);
        if (vec_out) {
            if (d.dst_u8)
                *reinterpret_cast<uint32_t*>(d.dst_u8 + o) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            if (d.lr_f32) {
                f32x4 f;
#pragma unroll
                for (int j = 0; j < 4; ++j) f[j] = ((float)q[j] / 255.f - mean) / stdv;
                *reinterpret_cast<f32x4*>(d.lr_f32 + o) = f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (ox + j < d.out_w) {
                    if (d.dst_u8) d.dst_u8[o + j] = (uint8_t)q[j];
                    if (d.lr_f32) d.lr_f32[o + j] = ((float)q[j] / 255.f - mean) / stdv;
                }
            }
        }
    }

    // the HR tensor of the source region this tile owns (integer ratio; checked by the caller)
    if (d.hr_f32) {
        const int sy = d.in_h / d.out_h, sx = d.in_w / d.out_w;
        const int ry0 = oy0 * sy, rx0 = ox0 * sx;
        const int rh = (d.in_h - ry0 < RS_TH * sy ? d.in_h - ry0 : RS_TH * sy);
        const int rw = (d.in_w - rx0 < RS_TW * sx ? d.in_w - rx0 : RS_TW * sx);
        float* hr = d.hr_f32 + (size_t)img * 3 * in_plane;
        if ((d.in_w & 3) == 0) {
            const int qw = rw >> 2;  // rx0 and rw are multiples of 4 with in_w
            for (int i = tid; i < 3 * rh * qw; i += 256) {
                const int xq = i % qw, cr = i / qw, c = cr / rh, r = cr - c * rh;
                const size_t o = (size_t)c * in_plane + (size_t)(ry0 + r) * d.in_w + rx0 + xq * 4;
                const uint32_t p = *reinterpret_cast<const uint32_t*>(src + o);
                const float mean = pick3(d.mean, c), stdv = pick3(d.std, c);
                f32x4 f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = (float)((p >> (8 * j)) & 255u) / 255.f;
                    f[j] = d.hr_norm ? (x - mean) / stdv : x * 2.f - 1.f;
                }
                *reinterpret_cast<f32x4*>(hr + o) = f;
            }
        } else {
            for (int i = tid; i < 3 * rh * rw; i += 256) {
                const int xx = i % rw, cr = i / rw, c = cr / rh, r = cr - c * rh;
                const size_t o = (size_t)c * in_plane + (size_t)(ry0 + r) * d.in_w + rx0 + xx;
                const float x = (float)src[o] / 255.f;
                hr[o] = d.hr_norm ? (x - pick3(d.mean, c)) / pick3(d.std, c) : x * 2.f - 1.f;
            }
        }
    }
}

int resample_u8_dispatch(const isr_resample_desc* d, hipStream_t s) {
    const int tiles_x = (d->out_w + RS_TW - 1) / RS_TW, tiles_y = (d->out_h + RS_TH - 1) / RS_TH;
    const long long blocks = (long long)d->n * tiles_x * tiles_y;
    if (blocks >= (1ll << 31)) return DISPATCH_UNSUPPORTED;
    hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, *d, tiles_x, tiles_y);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
