// The dihedral transforms (include/isr.h): isr_dihedral, isr_ensemble_expand_u8 and isr_ensemble_reduce.
// All three only move data (the reduce adds eight floats per element), so all that matters is that
// every global read and every global write runs along its own innermost axis.  An op is decoded into
// (t, fy, fx): y[i][j] = x[fy ? h - 1 - a : a][fx ? w - 1 - b : b] with (a, b) = t ? (j, i) : (i, j).
// A block owns one square tile of the OUTPUT; the matching source tile (flipped origin, never
// transposed) goes to LDS row by row, and the output rows are read back out of it, along LDS columns
// when t is set.  Flips only reverse an index inside the tile.
//
// uint8: 64 x 64 tile, LDS rows of 17 dwords (68 B).  A lane moves 4 bytes on both sides (one dword
// where the address is 4-byte aligned and the quad inside the image, bytes otherwise).
//   fill and straight read: a 32-lane half holds quads 0..15 of rows r and r + 16; 16 * 17 = 272 = 16
//     (mod 32), so the two rows take banks b..b + 15 and b + 16..b + 31: conflict-free.
//   transposed read: lane (ri = l & 3, q = l >> 2) makes output row 4 g + ri, quad q, from LDS rows
//     4 q + e, e = 0..3 (one ds_read_b32 each, the byte picked by a shift), column = the output row.  A
//     half holds q = 0..7 or 8..15 and four ri that share one dword (a broadcast): rows 4 q apart
//     are 68 q = 4 q (mod 32) dwords apart, 8 distinct banks: conflict-free.  A wave stores 4 rows of
//     64 contiguous bytes.
// fp32: 32 x 32 tile, rows of 33 dwords; a half reads or writes one row (stride 1) or one column
//   (stride 33 = 1 mod 32): conflict-free either way.
// The reduce gives a thread 4 adjacent outputs of one row (8 quads x 32 rows = 256 threads): the four
// even members come straight from global memory (16-byte loads where aligned), the four odd
// members' source tiles go to LDS first (4 x 32 x 33 floats = 16.5 KB); element e of quad q reads row
// 4 q + e, column = its output row: a half holds 8 quads x 4 rows, banks 4 q + row: conflict-free.
#include "isr_common.h"
#include "dispatch.h"

namespace isr {

namespace {

constexpr int D8_T = 64, D8_P = 17;   // uint8 tile side, LDS pitch in dwords
constexpr int D32_T = 32, D32_P = 33; // fp32 tile side, LDS pitch in dwords

struct Op {
    bool t, fy, fx;
};

__device__ __forceinline__ Op decode(int k) {
    const int r = k & 3, f = (k >> 2) & 1;
    return {(r & 1) != 0, r >= 2, ((r == 1 || r == 2) ? 1 : 0) != f};
}

// the inverse of op k in 0..7
__host__ __device__ __forceinline__ int inverse(int k) { return k < 4 ? (4 - k) & 3 : k; }

// (row, quad) of a 64 x 16-quad tile for thread t in pass it of 4: see the bank layout above
__device__ __forceinline__ void d8_rowquad(int t, int it, int& r, int& q) {
    const int g = t >> 4;
    q = t & 15;
    r = (g & 1) * 16 + (g >> 1) + (it & 1) * 8 + (it >> 1) * 32;
}

__device__ __forceinline__ void store_quad_u8(uint8_t* row, int x, int w, uint32_t v) {
    uint8_t* p = row + x;
    if (x + 3 < w && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<uint32_t*>(p) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x + e < w) p[e] = (uint8_t)(v >> (8 * e));
    }
}

// One 64 x 64 output tile (origin oy0, ox0) of op `k` applied to the h x w plane src; dst is the
// ho x wo result plane.  lds: D8_T * D8_P dwords.
__device__ __forceinline__ void tile_u8(uint32_t* lds, const uint8_t* src, uint8_t* dst, int h, int w, int k,
                                        int oy0, int ox0) {
    const Op op = decode(k);
    const int ho = op.t ? w : h, wo = op.t ? h : w;
    const int a0 = op.t ? ox0 : oy0, b0 = op.t ? oy0 : ox0;
    const int iy0 = op.fy ? h - a0 - D8_T : a0, ix0 = op.fx ? w - b0 - D8_T : b0;
    const int t = threadIdx.x;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        int r, q;
        d8_rowquad(t, it, r, q);
        const int y = iy0 + r, x = ix0 + 4 * q;
        uint32_t v = 0;
        if (y >= 0 && y < h && x > -4 && x < w) {
            const uint8_t* p = src + ((ptrdiff_t)y * w + x);
            if (x >= 0 && x + 3 < w && ((uintptr_t)p & 3) == 0) {
                v = *reinterpret_cast<const uint32_t*>(p);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x + e >= 0 && x + e < w) v |= (uint32_t)p[e] << (8 * e);
            }
        }
        lds[r * D8_P + q] = v;
    }
    __syncthreads();
    if (!op.t) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            int li, q;
            d8_rowquad(t, it, li, q);
            const int oy = oy0 + li, ox = ox0 + 4 * q;
            if (oy >= ho || ox >= wo) continue;
            const int r = op.fy ? D8_T - 1 - li : li;
            const uint32_t v = op.fx ? __builtin_bswap32(lds[r * D8_P + 15 - q]) : lds[r * D8_P + q];
            store_quad_u8(dst + (size_t)oy * wo, ox, wo, v);
        }
    } else {
        const int ri = t & 3, q = (t >> 2) & 15, wv = t >> 6;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int li = (wv * 4 + it) * 4 + ri;
            const int oy = oy0 + li, ox = ox0 + 4 * q;
            if (oy >= ho || ox >= wo) continue;
            const int c = op.fx ? D8_T - 1 - li : li;
            uint32_t v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = op.fy ? D8_T - 1 - (4 * q + e) : 4 * q + e;
                v |= ((lds[r * D8_P + (c >> 2)] >> (8 * (c & 3))) & 255u) << (8 * e);
            }
            store_quad_u8(dst + (size_t)oy * wo, ox, wo, v);
        }
    }
}

// Fills one 32 x 33 LDS tile with the source tile of output tile (oy0, ox0) under `op`; src is h x w.
// Outside the image: zeros (never read back: they belong to outputs outside the result).
__device__ __forceinline__ void fill_f32(uint32_t* lds, const uint32_t* src, int h, int w, Op op, int oy0, int ox0) {
    const int a0 = op.t ? ox0 : oy0, b0 = op.t ? oy0 : ox0;
    const int iy0 = op.fy ? h - a0 - D32_T : a0, ix0 = op.fx ? w - b0 - D32_T : b0;
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = g + 8 * it, y = iy0 + r, x = ix0 + c;
        lds[r * D32_P + c] = (y >= 0 && y < h && x >= 0 && x < w) ? src[(size_t)y * w + x] : 0u;
    }
}

// element (li, lj) of the output tile, from a tile fill_f32 made
__device__ __forceinline__ uint32_t read_f32(const uint32_t* lds, Op op, int li, int lj) {
    const int a = op.t ? lj : li, b = op.t ? li : lj;
    return lds[(op.fy ? D32_T - 1 - a : a) * D32_P + (op.fx ? D32_T - 1 - b : b)];
}

__device__ __forceinline__ void tile_f32(uint32_t* lds, const uint32_t* src, uint32_t* dst, int h, int w, int k,
                                         int oy0, int ox0) {
    const Op op = decode(k);
    const int ho = op.t ? w : h, wo = op.t ? h : w;
    fill_f32(lds, src, h, w, op, oy0, ox0);
    __syncthreads();
    const int lj = threadIdx.x & 31, g = threadIdx.x >> 5;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int li = g + 8 * it, oy = oy0 + li, ox = ox0 + lj;
        if (oy < ho && ox < wo) dst[(size_t)oy * wo + ox] = read_f32(lds, op, li, lj);
    }
}

// 4 adjacent floats row[x0 .. x0 + 3] (rev: row[x0 + 3 .. x0]), zeros outside [0, w)
__device__ __forceinline__ f32x4 load_quad_f32(const float* row, int x0, int w, bool rev) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const float* p = row + x0;
    if (x0 >= 0 && x0 + 3 < w && ((uintptr_t)p & 15) == 0) {
        v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x0 + e >= 0 && x0 + e < w) v[e] = p[e];
    }
    if (rev) v = f32x4{v[3], v[2], v[1], v[0]};
    return v;
}

}  // namespace

// block -> (plane = image * c + channel, tile); square tiles of the output
template <int ELEM>
__global__ __launch_bounds__(256) void dihedral_kernel(isr_dihedral_desc d, int tiles_x, int tiles_y) {
    __shared__ uint32_t lds[ELEM == 1 ? D8_T * D8_P : D32_T * D32_P];
    constexpr int T = ELEM == 1 ? D8_T : D32_T;
    const int txi = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
    const int tyi = rest % tiles_y, pl = rest / tiles_y;
    const int k = d.ops ? (d.ops[pl / d.c] & 7) : d.op;
    const size_t plane = (size_t)d.h * d.w;
    if constexpr (ELEM == 1)
        tile_u8(lds, (const uint8_t*)d.x + pl * plane, (uint8_t*)d.y + pl * plane, d.h, d.w, k, tyi * T, txi * T);
    else
        tile_f32(lds, (const uint32_t*)d.x + pl * plane, (uint32_t*)d.y + pl * plane, d.h, d.w, k, tyi * T, txi * T);
}

// block -> (member k, plane, tile); the tile count of a plane is the same for both shapes
__global__ __launch_bounds__(256) void ensemble_expand_u8_kernel(isr_ensemble_expand_desc d, int tiles_h, int tiles_w) {
    __shared__ uint32_t lds[D8_T * D8_P];
    const int tiles = tiles_h * tiles_w, planes = d.n * 3;
    const int tile = blockIdx.x % tiles, rest = blockIdx.x / tiles;
    const int pl = rest % planes, k = rest / planes;
    const int tiles_x = (k & 1) ? tiles_h : tiles_w;  // an odd member is w x h
    const size_t plane = (size_t)d.h * d.w;
    uint8_t* dst = ((k & 1) ? d.odd : d.even) + ((size_t)(k >> 1) * planes + pl) * plane;
    tile_u8(lds, d.x + pl * plane, dst, d.h, d.w, k, tile / tiles_x * D8_T, tile % tiles_x * D8_T);
}

// block -> (plane, 32 x 32 tile of the h x w output)
__global__ __launch_bounds__(256) void ensemble_reduce_kernel(isr_ensemble_reduce_desc d, int tiles_x, int tiles_y) {
    __shared__ uint32_t lds[4][D32_T * D32_P];
    const int txi = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
    const int tyi = rest % tiles_y, pl = rest / tiles_y;
    const int h = d.h, w = d.w, oy0 = tyi * D32_T, ox0 = txi * D32_T;
    const size_t plane = (size_t)h * w, member = (size_t)d.n * 3 * plane;
    // member k = 2 j + 1 is a w x h plane; op inverse(k) takes it back to h x w
#pragma unroll
    for (int j = 0; j < 4; ++j)
        fill_f32(lds[j], (const uint32_t*)d.odd + j * member + pl * plane, w, h, decode(inverse(2 * j + 1)), oy0, ox0);
    __syncthreads();
    const int q = threadIdx.x & 7, li = threadIdx.x >> 3;
    const int oy = oy0 + li, ox = ox0 + 4 * q;
    if (oy >= h || ox >= w) return;
    f32x4 s;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const Op op = decode(inverse(k));
        f32x4 m;
        if (k & 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = __uint_as_float(read_f32(lds[k >> 1], op, li, 4 * q + e));
        } else {
            const float* row = d.even + (k >> 1) * member + pl * plane + (size_t)(op.fy ? h - 1 - oy : oy) * w;
            m = load_quad_f32(row, op.fx ? w - 4 - ox : ox, w, op.fx);
        }
        if (k == 0) s = m;
        else s = s + m;
    }
    const f32x4 m = s * 0.125f;
    const size_t o = pl * plane + (size_t)oy * w + ox;
    if (d.y_u8) {
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float qv = rintf((m[e] + 1.f) / 2.f * 255.f);  // the tail's expression (conv9x9.hip)
            v |= (uint32_t)(uint8_t)fminf(fmaxf(qv, 0.f), 255.f) << (8 * e);
        }
        store_quad_u8((uint8_t*)d.y + o - ox, ox, w, v);
    } else {
        float* p = (float*)d.y + o;
        if (ox + 3 < w && ((uintptr_t)p & 15) == 0) {
            *reinterpret_cast<f32x4*>(p) = m;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ox + e < w) p[e] = m[e];
        }
    }
}

static long long tile_blocks(long long planes, int h, int w, int t, int& tiles_y, int& tiles_x) {
    tiles_y = (h + t - 1) / t;
    tiles_x = (w + t - 1) / t;
    return planes * tiles_y * tiles_x;
}

// -2: more workgroups than a grid holds
int dihedral_dispatch(const isr_dihedral_desc* d, hipStream_t s) {
    const bool t = !d->ops && (d->op & 1);  // per-image ops: square, the tile grid is the same
    int tiles_y, tiles_x;
    const long long blocks = tile_blocks((long long)d->n * d->c, t ? d->w : d->h, t ? d->h : d->w,
                                         d->elem == 1 ? D8_T : D32_T, tiles_y, tiles_x);
    if (blocks >= (1ll << 31)) return DISPATCH_UNSUPPORTED;
    if (d->elem == 1)
        hipLaunchKernelGGL(dihedral_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, *d, tiles_x, tiles_y);
    else
        hipLaunchKernelGGL(dihedral_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, *d, tiles_x, tiles_y);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int ensemble_expand_u8_dispatch(const isr_ensemble_expand_desc* d, hipStream_t s) {
    int tiles_h, tiles_w;
    const long long blocks = tile_blocks(8ll * d->n * 3, d->h, d->w, D8_T, tiles_h, tiles_w);
    if (blocks >= (1ll << 31)) return DISPATCH_UNSUPPORTED;
    hipLaunchKernelGGL(ensemble_expand_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, *d, tiles_h, tiles_w);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int ensemble_reduce_dispatch(const isr_ensemble_reduce_desc* d, hipStream_t s) {
    int tiles_y, tiles_x;
    const long long blocks = tile_blocks((long long)d->n * 3, d->h, d->w, D32_T, tiles_y, tiles_x);
    if (blocks >= (1ll << 31)) return DISPATCH_UNSUPPORTED;
    hipLaunchKernelGGL(ensemble_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, *d, tiles_x, tiles_y);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int dihedral_inverse(int op) { return inverse(op); }

}  // namespace isr
