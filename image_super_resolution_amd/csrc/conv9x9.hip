// 9x9 'same' convolutions at the two ends of the generator, on MFMA.
//
// head: ResNet.conv0 / EResNet.conv0 = ConvWithoutBN(3, 64, 9) + LeakyReLU
//       (utils/models.py:596, :625), with Normalize (utils/datasets.py:65-71)
//       fused for uint8 input.  K = 9 rows x 12 column taps (9 real) x 4
//       channels (3 real): a k-step of 16 is 4 consecutive column taps of one
//       row x 4 channels = 2 adjacent pixels x 8 bytes of the channels-padded
//       LDS halo, so A fragments are plain 16-byte LDS reads (no im2col).
// tail: ResNet.conv2 / EResNet.conv2 = ConvWithoutBN(64, 3, 9) + Tanh
//       (utils/models.py:607, :636), with TanhToArrayImage (:448-451) fused
//       for uint8 output.  N = 3 is too skinny for MFMA, so the kernel moves
//       the 9 kernel ROWS into N: stage 1 is a 1x9 conv producing
//       T[y'][x][(ky,co)] (27 of 32 columns used) for the TH+8 input rows of
//       the tile; stage 2 sums out[y][x][co] = sum_ky T[y+ky-4][x][(ky,co)] in
//       LDS and applies bias + tanh (+ uint8 quantisation).
#include "isr_common.h"
#include "dispatch.h"

namespace isr {

// ============================== head ======================================
namespace head {
constexpr int R = 4, WM = 4, NF = 2, TH = R * WM, TW = 32, CT = NF * 32;
constexpr int HR = TH + 8, HC = 44; // halo cols: 32 + 8, padded so tap groups 9..11 stay in range
constexpr int HALO_BYTES = HR * HC * 8;
constexpr int EPS = CT + 4;
constexpr int EP_BYTES = WM * 32 * EPS * 4;  // one output row per wave at a time
constexpr int LDS = EP_BYTES > HALO_BYTES ? EP_BYTES : HALO_BYTES;
}  // namespace head

// packed head weights: [ky 9][ks 3][n 64][k 16] bf16,
// k = 8h + e → column tap t = 4ks + 2h + (e>>2), channel c = e & 3 (zero if t>=9 or c>=3).
template <bool H>
__global__ __launch_bounds__(256) void head9x9_kernel(isr_head_desc d) {
    using namespace head;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int img = blockIdx.z;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int wave = wave_id();
    const int lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;

    // ---- halo: rows y0-4 .. y0+TH+3, cols x0-4 .. x0+39, 4 ch bf16 ----
    const size_t plane = (size_t)d.h * d.w;
    for (int p = threadIdx.x; p < HR * HC; p += 256) {
        const int row = p / HC, col = p - row * HC;
        const int yy = y0 - 4 + row, xx = x0 - 4 + col;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (yy >= 0 && yy < d.h && xx >= 0 && xx < d.w && col < 40) {
            const size_t o = (size_t)img * 3 * plane + (size_t)yy * d.w + xx;
            if (d.x_u8) {
                const uint8_t* xp = (const uint8_t*)d.x;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = ((float)xp[o + c * plane] / 255.f - d.mean[c]) * d.inv_std[c];
            } else {
                const float* xp = (const float*)d.x;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = xp[o + c * plane];
            }
        }
        if constexpr (H) {
            f16x4 t;
#pragma unroll
            for (int c = 0; c < 4; ++c) t[c] = (_Float16)v[c];
            *reinterpret_cast<f16x4*>(smem + p * 8) = t;
        } else {
            bf16x4 t;
#pragma unroll
            for (int c = 0; c < 4; ++c) t[c] = (__bf16)v[c];
            *reinterpret_cast<bf16x4*>(smem + p * 8) = t;
        }
    }
    __syncthreads();

    f32x16 acc[R][NF];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[r][f][g] = 0.f;

    const char* wp = (const char*)d.wpack;
#pragma unroll 1
    for (int ks = 0; ks < 3; ++ks) {
        bf16x8 b[9][NF];
#pragma unroll
        for (int ky = 0; ky < 9; ++ky)
#pragma unroll
            for (int f = 0; f < NF; ++f)
                b[ky][f] = *reinterpret_cast<const bf16x8*>(wp + (((ky * 3 + ks) * CT + f * 32 + l31) * 16 + hh * 8) * 2);
#pragma unroll
        for (int i = 0; i < R + 8; ++i) {
            const char* ap = smem + ((wave * R + i) * HC + l31 + 4 * ks + 2 * hh) * 8;
            bf16x4 lo = *reinterpret_cast<const bf16x4*>(ap);
            bf16x4 hi = *reinterpret_cast<const bf16x4*>(ap + 8);
            bf16x8 a;
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] = lo[e]; a[4 + e] = hi[e]; }
#pragma unroll
            for (int ky = 0; ky < 9; ++ky) {
                const int r = i - ky;
                if (r >= 0 && r < R) {
#pragma unroll
                    for (int f = 0; f < NF; ++f) acc[r][f] = mfma32t<H>(a, b[ky][f], acc[r][f]);
                }
            }
        }
    }
    __syncthreads();

    // epilogue one output row per wave at a time through a wave-private 32 x EPS float
    // image (35 KB for the block instead of 139 KB: more than one block per CU)
    float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EPS);
    Epi e;
    e.bias = d.bias; e.slope = d.slope; e.s1 = 1.f; e.s2 = 1.f;
    e.y = d.y; e.y2 = d.y2; e.r1.data = nullptr; e.r2.data = nullptr; e.h = d.h; e.w = d.w;
    e.m = d.m; e.mslope = d.mslope;
    constexpr int CG = CT / 8;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        __builtin_amdgcn_s_waitcnt(0xC07F);  // previous row's image reads are complete
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int px = (g & 3) + 8 * (g >> 2) + 4 * hh;
                ep[px * EPS + f * 32 + l31] = acc[r][f][g];
            }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < CT / 16; ++it) {
            const int jj = lane + 64 * it;
            const int cg = jj % CG, px = jj / CG;
            float v[8];
            const float* src = ep + px * EPS + cg * 8;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = src[k];
            epi_plain8<H>(e, v, img, y0 + wave * R + r, x0 + px, cg * 8);
        }
    }
}

template <class OT>
__global__ void pack_head_kernel(const float* __restrict__ w, OT* __restrict__ out, int cout, int cin) {
    const int total = 9 * 3 * cout * 16;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        int rem = idx;
        const int k = rem % 16; rem /= 16;
        const int n = rem % cout; rem /= cout;
        const int ks = rem % 3; rem /= 3;
        const int ky = rem;
        const int hh = k >> 3, e = k & 7;
        const int t = 4 * ks + 2 * hh + (e >> 2), c = e & 3;
        float v = 0.f;
        if (t < 9 && c < cin) v = w[(((size_t)n * cin + c) * 9 + ky) * 9 + t];
        out[idx] = (OT)v;
    }
}

// ============================== tail ======================================
// Two kernels ship: the 8-wave row-streaming walk (variant 5, production) and the 8-row per-tile
// kernel (variant 3, the fallback of images whose output passes 2 GiB).  Both give the same bits:
// the same MFMA order per T element and the same ky-sum order.  The forms that lost their A/B (the
// 16-row per-tile kernel, the persistent, 4-wave and lane-streaming walks) were removed; their
// measurements are in DESIGN.md section 5.
// packed tail weights: [kx 9][chunk 2][ks 2][n 32][hpos 2][8] bf16,
// n = ky*3 + co (27 used), element = W[co][chunk*32 + ks*16 + h*8 + e][ky][kx], h = hpos ^ ((n>>3)&1).
namespace tail {
constexpr int W_BYTES = 9 * 2 * 2 * 32 * 32;  // [kx][chunk][ks][n][hpos][8] bf16 = 36864
}  // namespace tail

// ---- 8-row tail (variant 3): a per-tile kernel with 8 output rows per block and one
// 32-channel halo chunk resident at a time (chunk 1 refills chunk 0's slot after a
// barrier), so LDS is 76 KB and two blocks share a CU: one block's halo fetch runs
// beside the other's MFMAs.
namespace tail8 {
constexpr int TH = 8, TW = 32, WM = 4;
constexpr int TR = TH + 8;                    // 16 input rows
constexpr int RT = TR / WM;                   // 4 input rows per wave
constexpr int HC = TW + 8;                    // 40 halo cols
constexpr int HIPL = TR * HC / 32;            // 20 glds per 16-channel plane
constexpr int HALO_INSTR = 2 * HIPL;          // 40 per 32-channel chunk
constexpr int HALO_BYTES = HALO_INSTR * 1024; // 40960
constexpr int W_BYTES = tail::W_BYTES;        // 36864
constexpr int W_INSTR = W_BYTES / 1024;       // 36
constexpr int TS = 33;
constexpr int T_BYTES = TR * 32 * TS * 4;     // 67584
constexpr int P1 = HALO_BYTES + W_BYTES;      // 77824
constexpr int LDS = P1 > T_BYTES ? P1 : T_BYTES;
static_assert(HALO_INSTR % WM == 0 && W_INSTR % WM == 0, "even glds split");
static_assert(TR * HC % 32 == 0, "");
static_assert(2 * LDS <= 163840, "two blocks per CU");
}  // namespace tail8

template <bool H = false>
__global__ __launch_bounds__(256, 2) void tail9x9_k8_kernel(isr_tail_desc d) {
    using namespace tail8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int img = blockIdx.z;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int wave = wave_id();
    const int lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;

    const char* xbase = view_at(d.x, img, y0 - 4, x0 - 4, 0);
    const size_t pstride = plane_bytes(d.x);
    const int xrow = d.x.wp * 32;
    char* halo = smem;
    char* wl = smem + HALO_BYTES;

    f32x16 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[t][g] = 0.f;

    auto load_halo = [&](int chunk) {
        for (int j = wave; j < HALO_INSTR; j += WM) {
            const int kp = j / HIPL;
            const int u = (j - kp * HIPL) * 64 + lane;
            const int q = u >> 1;
            const int row = q / HC, col = q - row * HC;
            const int c = (u & 1) ^ ((q >> 3) & 1);
            glds16(xbase + (size_t)(chunk * 2 + kp) * pstride + row * xrow + col * 32 + c * 16, halo + j * 1024);
        }
    };
    for (int j = wave; j < W_INSTR; j += WM)
        glds16((const char*)d.wpack + j * 1024 + lane * 16, wl + j * 1024);
    load_halo(0);

#pragma unroll
    for (int chunk = 0; chunk < 2; ++chunk) {
        wait_vm0();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int kx = 0; kx < 9; ++kx) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int n = l31;
                const bf16x8 b = lds_read16(wl + ((((kx * 2 + chunk) * 2 + ks) * 32 + n) * 2 + (hh ^ ((n >> 3) & 1))) * 16);
                const char* hp = halo + ks * HIPL * 1024;
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const int q = (wave * RT + t) * HC + kx + l31;
                    acc[t] = mfma32t<H>(lds_read16(hp + halo_unit2(q, hh) * 16), b, acc[t]);
                }
            }
        }
        if (chunk == 0) {
            __syncthreads();  // every wave is done with chunk 0's halo before it is overwritten
            load_halo(1);
        }
    }
    __syncthreads();

    float* T = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int px = (g & 3) + 8 * (g >> 2) + 4 * hh;
            T[((wave * RT + t) * 32 + px) * TS + l31] = acc[t][g];
        }
    __syncthreads();

    const size_t plane = (size_t)d.h * d.w;
    for (int item = threadIdx.x; item < TH * TW; item += 256) {
        const int yr = item >> 5, px = item & 31;
        const int yy = y0 + yr, xx = x0 + px;
        float s[3];
#pragma unroll
        for (int co = 0; co < 3; ++co) s[co] = d.bias ? d.bias[co] : 0.f;
#pragma unroll
        for (int ky = 0; ky < 9; ++ky) {
            const float* tp = T + ((yr + ky) * 32 + px) * TS + ky * 3;
#pragma unroll
            for (int co = 0; co < 3; ++co) s[co] += tp[co];
        }
        if (yy < d.h && xx < d.w) {
            const size_t o = (size_t)img * 3 * plane + (size_t)yy * d.w + xx;
#pragma unroll
            for (int co = 0; co < 3; ++co) {
                const float t = tanhf(s[co]);
                if (d.y_u8) {
                    const float q = rintf((t + 1.f) / 2.f * 255.f);
                    ((uint8_t*)d.y)[o + co * plane] = (uint8_t)fminf(fmaxf(q, 0.f), 255.f);
                } else {
                    ((float*)d.y)[o + co * plane] = t;
                }
            }
        }
    }
}

__device__ __forceinline__ f32x4 lds_read16f4_async(const char* p) {
    f32x4 r;
    const uint32_t a = (uint32_t)(uintptr_t)ISR_LDS_PTR(p);
    asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(a) : "memory");
    return r;
}
template <int N>
__device__ __forceinline__ void lds_wait_t4(f32x4 (&t)[5]) {
    asm volatile("s_waitcnt lgkmcnt(%5)"
                 : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4])
                 : "i"(N));
}
template <int N>
__device__ __forceinline__ void lds_wait1(bf16x8& a) {
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "i"(N));
}
__device__ __forceinline__ void vm_wait(int n) {  // s_waitcnt vmcnt(n), n = 0 or 2 (runtime-uniform)
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// ---- row-streaming tail, 8 waves (variant 5): no recomputed rows.  A block owns a 32-column
// strip of one image over `sh` output rows and walks DOWN it: each wave turns one input row into
// its T row (the 1x9 row conv, N = (ky, co)) with 36 MFMAs, every T row is computed once (the
// per-tile kernel recomputes the 8 halo rows of every tile: 2x the MFMA work), and output row y is
// finished once T rows y-4 .. y+4 exist.  The T terms go to a 16-row ring keyed by the output row
// they feed (O[r0][px][pos(co, ky)] = T(r0+ky)[px][ky*3+co]).  The 36 weight fragments stay in
// VGPRs (one LDS read per MFMA instead of two: with weights in LDS the waves' fragment reads
// saturated the LDS port before the MFMAs did).  Two waves per SIMD: the non-MFMA costs of a wave
// (LDS-DMA issue, the finish's VALU, LDS waits) overlap its partner's MFMAs.  Eight T rows per
// iteration (one per wave), input rows double-buffered (group i+1's DMA issued in the gaps of
// iteration i), the O ring written at the end of the iteration; after barrier #2 the next
// iteration reads its O terms into registers before its top barrier, so O row r0 lives two
// iterations: 16 rows.  The finish of an older output row (ky sums, tanh, 2 stores) is interleaved
// into the MFMA sequence of the current T row.  Bit-identical to variant 3.
// LDS reads of the loop are asm (lds_read16_async / lds_read16f4_async) with counted lgkmcnt
// waits: hipcc's own waits here were lgkmcnt(0) every few MFMAs.  Counted vmcnt: per wave,
// 5 LDS-DMA per row group and exactly 2 stores per finished row.
namespace tail8w {
constexpr int TW = 32, WM = 8, GR = 8;       // strip width, waves, rows per group (one per wave)
constexpr int HC = TW + 8;
constexpr int ROWB = 4 * HC * 32;             // 5120
constexpr int ROW_INSTR = ROWB / 1024;        // 5
constexpr int NG = 2;
constexpr int NT = 16;
constexpr int TS = 36;                        // O row: [px][co 0: 0..8, co 1: 9..17, co 2: 20..28] + pad (conflict-free 16-B px reads)
constexpr int TROW = TW * TS * 4;             // 4608
constexpr int OFF_IN = 0;
constexpr int OFF_T = OFF_IN + NG * GR * ROWB;      // 81920
constexpr int LDS = OFF_T + NT * TROW + 64;        // 155712 (+64: lanes 32..63 of px 31 read 4 floats past a row)
constexpr int PD = 4;                          // A-fragment prefetch distance (MFMA steps)
constexpr int ST = 2;                          // stores per finished row per wave
static_assert(LDS <= 163840, "LDS");
}  // namespace tail8w

template <bool H = false>
__global__ __launch_bounds__(512, 1) void tail9x9_stream8_kernel(isr_tail_desc d, int sh) {
    using namespace tail8w;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nstrip = d.wa / TW, nseg = d.ha / sh;
    int b = xcd_remap(blockIdx.x, gridDim.x);
    const int strip = b % nstrip;
    b /= nstrip;
    const int seg = b % nseg;
    const int img = b / nseg;
    const int x0 = strip * TW, ys = seg * sh;
    const int wave = wave_id();
    const int lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;
    const int nit = sh / GR + 1;  // T rows ys-4 .. ys+sh+3, eight per iteration
    float* T = reinterpret_cast<float*>(smem + OFF_T);
    const size_t pstride = plane_bytes(d.x);
    const char* xcol = view_at(d.x, img, 0, x0 - 4, 0);
    const int xrow = d.x.wp * 32;

    uint32_t doff[ROW_INSTR];
#pragma unroll
    for (int j = 0; j < ROW_INSTR; ++j) {
        const int u = j * 64 + lane;
        const int p = u / (2 * HC), r = u - p * 2 * HC;
        const int q = r >> 1, c = (r & 1) ^ ((q >> 3) & 1);
        doff[j] = (uint32_t)(p << 16 | (q * 32 + c * 16));  // plane (pstride may exceed 4 GB) | in-plane
    }
    auto dma = [&](int g, int j) {
        const int y = ys - 4 + GR * g + wave;  // within the buffer's zero border (pad 4)
        glds16(xcol + (ptrdiff_t)y * xrow + (size_t)(doff[j] >> 16) * pstride + (doff[j] & 0xffff),
               smem + OFF_IN + ((g % NG) * GR + wave) * ROWB + j * 1024);
    };
    bf16x8 wr[36];
#pragma unroll
    for (int st = 0; st < 36; ++st) {
        const int chunk = st / 18, kx = (st / 2) % 9, ks = st & 1, n = l31;
        wr[st] = *reinterpret_cast<const bf16x8*>((const char*)d.wpack +
                                                  ((((kx * 2 + chunk) * 2 + ks) * 32 + n) * 2 + (hh ^ ((n >> 3) & 1))) * 16);
    }
#pragma unroll
    for (int j = 0; j < ROW_INSTR; ++j) dma(0, j);

    const size_t plane = (size_t)d.h * d.w;
    const int esz = d.y_u8 ? 1 : 4;
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
        (char*)d.y + (size_t)img * 3 * plane * esz, (short)0, (int)(3 * plane * esz), 0x00020000);
    const int cA = hh ? 2 : 0;
    const float biasA = d.bias ? d.bias[cA] : 0.f, biasB = d.bias ? d.bias[1] : 0.f;
    const int wky = l31 < 27 ? l31 / 3 : 9;
    const int wco = l31 - 3 * (l31 / 3);
    const int wpos = l31 < 27 ? (wco == 0 ? wky : wco == 1 ? 9 + wky : 20 + wky) : 29 + (l31 - 27);
    uint32_t aoff[9];
#pragma unroll
    for (int kx = 0; kx < 9; ++kx) aoff[kx] = halo_unit2(kx + l31, hh) * 16;

    f32x4 t4[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) t4[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto tv = [&](int n) { return t4[n >> 2][n & 3]; };

    for (int i = 0; i <= nit; ++i) {
        const bool fin = i >= 2;
        // this iteration's O terms (output row ys + 8(i-2) + wave): the O ring is complete up to
        // it since barrier #2 of the previous iteration.  Issued here, at the top, so no asm
        // load is in flight across the loop's back-edge (the compiler may copy such registers)
        const int r0 = GR * (i - 2) + wave;
        if (fin) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                t4[k] = lds_read16f4_async((const char*)(T + (r0 & (NT - 1)) * (TW * TS) + l31 * TS + 20 * hh + 4 * k));
        }
        // own row of group i landed; younger VMEM: the stores of iteration i-1
        vm_wait(ST * (i - 1 >= 2));
        lds_wait_t4<0>(t4);
        // top barrier: LDS-DMA data (vmcnt, then a barrier, then ds_read), and every wave holds
        // its O terms, so their ring slots may be rewritten by this iteration's T writes
        __builtin_amdgcn_s_barrier();
        const bool dma_on = i + 1 < nit;
        const int yy = ys + r0, xx = x0 + l31;
        const bool valid = yy < d.h && xx < d.w;
        float sA = biasA, sB = biasB;
        auto store = [&](float sv, int co, bool ok) {
            const float t = tanhf(sv);
            const int off = ok ? (int)((co * plane + (size_t)yy * d.w + xx) * esz) : 0x7ffffff0;
            if (d.y_u8) {
                const float q = rintf((t + 1.f) / 2.f * 255.f);
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)fminf(fmaxf(q, 0.f), 255.f), yrs, off, 0, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, t), yrs, off, 0, 0);
            }
        };

        if (i < nit) {
            const char* row = smem + OFF_IN + ((i % NG) * GR + wave) * ROWB;
            f32x16 acc;
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[g] = 0.f;
            bf16x8 fa[PD];
            auto rd = [&](int st_, int slot) {
                const int chunk = st_ / 18, kx = (st_ / 2) % 9, ks = st_ & 1;
                fa[slot] = lds_read16_async(row + (chunk * 2 + ks) * (2 * HC) * 16 + aoff[kx]);
            };
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s2 = 0; s2 < PD; ++s2) rd(s2, s2);
#pragma unroll
            for (int s2 = 0; s2 < 36; ++s2) {
                const int younger_rd = (35 - s2) < (PD - 1) ? (35 - s2) : (PD - 1);
                switch (younger_rd) {
                    case 3: lds_wait1<3>(fa[s2 % PD]); break;
                    case 2: lds_wait1<2>(fa[s2 % PD]); break;
                    case 1: lds_wait1<1>(fa[s2 % PD]); break;
                    default: lds_wait1<0>(fa[s2 % PD]); break;
                }
                __builtin_amdgcn_sched_barrier(0);
                acc = mfma32t<H>(fa[s2 % PD], wr[s2], acc);
                if (s2 + PD < 36) rd(s2 + PD, s2 % PD);
                if (s2 >= 1 && s2 <= ROW_INSTR && dma_on) dma(i + 1, s2 - 1);
                if (fin) {
                    if (s2 >= 1 && s2 <= 9) {  // same order as the per-tile kernels: bias, ky 0..8
                        sA += tv(s2 - 1);
                        sB += tv(9 + s2 - 1);
                    }
                    if (s2 == 12) store(sA, cA, valid);
                    if (s2 == 24) store(sB, 1, valid && hh == 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // T row 8i + wave into the O ring: T(r, px, n = ky*3+co) -> O[r - ky][px][pos(co, ky)]
            float* wrow = T + ((GR * i + wave - wky) & (NT - 1)) * (TW * TS) + 4 * hh * TS + wpos;
#pragma unroll
            for (int g = 0; g < 16; ++g) wrow[((g & 3) + 8 * (g >> 2)) * TS] = acc[g];
        } else if (fin) {
#pragma unroll
            for (int ky = 0; ky < 9; ++ky) {
                sA += tv(ky);
                sB += tv(9 + ky);
            }
            store(sA, cA, valid);
            store(sB, 1, valid && hh == 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // barrier #2: every T row of iteration i is in the O ring
    }
}

template <class OT>
__global__ void pack_tail_kernel(const float* __restrict__ w, OT* __restrict__ out, int cout, int cin) {
    const int total = tail::W_BYTES / 2;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        int rem = idx;
        const int e = rem % 8; rem /= 8;
        const int hpos = rem % 2; rem /= 2;
        const int n = rem % 32; rem /= 32;
        const int ks = rem % 2; rem /= 2;
        const int chunk = rem % 2; rem /= 2;
        const int kx = rem;
        const int hh = hpos ^ ((n >> 3) & 1);
        const int ky = n / 3, co = n % 3;
        const int ci = chunk * 32 + ks * 16 + hh * 8 + e;
        float v = 0.f;
        if (n < 27 && co < cout) v = w[(((size_t)co * cin + ci) * 9 + ky) * 9 + kx];
        out[idx] = (OT)v;
    }
}

// ============================== launchers ================================
int head9x9_fwd_dispatch(const isr_head_desc* d, hipStream_t s) {
    dim3 grid(d->wa / head::TW, d->ha / head::TH, d->n);
    auto go = [&](auto kern) {
        lds_limit((const void*)kern, head::LDS);
        hipLaunchKernelGGL(kern, grid, dim3(256), head::LDS, s, *d);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    };
    return d->f16 ? go(head9x9_kernel<true>) : go(head9x9_kernel<false>);
}

// The production choice for a descriptor on a device of `cus` compute units: the walk's segment
// height (8 .. 512), or 0 for the per-tile fallback of images whose output passes 2 GiB (the walk
// stores through 32-bit offsets).  -2: ha is no multiple of 8.
// segment height: the longest walk (<= 512 rows) that still gives every CU a strip — fewer,
// longer walks recompute fewer halo T rows and leave no partial last wave of blocks:
// 16x512^2 fp32 179 us at 128 rows, 164 at 256, 157 at 512 (profiles/r02_tail_sh.jsonl)
int tail_segment_rows(const isr_tail_desc* d, int cus) {
    if ((size_t)3 * d->h * d->w * (d->y_u8 ? 1 : 4) >= ((size_t)1 << 31)) return 0;
    int sh = 512;
    while (sh > 8 && (d->ha % sh || (long)d->n * (d->wa / tail8w::TW) * (d->ha / sh) < cus)) sh >>= 1;
    while (d->ha % sh) sh >>= 1;
    return sh < 8 ? -2 : sh;
}

// variant 0 = production = 5, the 8-wave row-streaming walk (170-177 us at 16 x 512^2, fp32 out,
// against 354-375 us for the 8-row per-tile kernel, variant 3); 3 is also the fallback of images
// whose output passes 2 GiB.  -2: any other id.
int tail9x9_fwd_variant(const isr_tail_desc* d, int variant, hipStream_t s) {
    if (variant == 0) variant = 5;
    if (variant != 3 && variant != 5) return DISPATCH_UNSUPPORTED;
    const int sh = variant == 5 ? tail_segment_rows(d, cu_count()) : 0;
    if (sh == 0) variant = 3;
    if (variant == 3) {
        auto go = [&](auto kern) {
            lds_limit((const void*)kern, tail8::LDS);
            hipLaunchKernelGGL(kern, dim3(d->wa / tail8::TW, d->ha / tail8::TH, d->n), dim3(256), tail8::LDS, s, *d);
            return hipGetLastError() == hipSuccess ? 0 : -1;
        };
        return d->f16 ? go(tail9x9_k8_kernel<true>) : go(tail9x9_k8_kernel<false>);
    }
    if (sh < 8) return DISPATCH_UNSUPPORTED;
    const int blocks = d->n * (d->wa / tail8w::TW) * (d->ha / sh);
    auto go = [&](auto kern) {
        lds_limit((const void*)kern, tail8w::LDS);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(512), tail8w::LDS, s, *d, sh);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    };
    return d->f16 ? go(tail9x9_stream8_kernel<true>) : go(tail9x9_stream8_kernel<false>);
}

// no shipping tail kernel writes stamps (only the removed 4-wave walk did)
int tail_stamps_set(void*) { return DISPATCH_UNSUPPORTED; }

int tail9x9_fwd_dispatch(const isr_tail_desc* d, hipStream_t s) { return tail9x9_fwd_variant(d, 0, s); }

size_t head9x9_packed_bytes(int cout) { return (size_t)9 * 3 * cout * 16 * 2; }
size_t tail9x9_packed_bytes() { return tail::W_BYTES; }

// h: fp16 weights (the isr_*_desc.f16 forms), else bf16; same layout and size
int head9x9_pack(const float* w, void* out, int cout, int cin, hipStream_t s, bool h) {
    if (h) hipLaunchKernelGGL(pack_head_kernel<_Float16>, dim3(64), dim3(256), 0, s, w, (_Float16*)out, cout, cin);
    else hipLaunchKernelGGL(pack_head_kernel<__bf16>, dim3(64), dim3(256), 0, s, w, (__bf16*)out, cout, cin);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int tail9x9_pack(const float* w, void* out, int cout, int cin, hipStream_t s, bool h) {
    if (h) hipLaunchKernelGGL(pack_tail_kernel<_Float16>, dim3(64), dim3(256), 0, s, w, (_Float16*)out, cout, cin);
    else hipLaunchKernelGGL(pack_tail_kernel<__bf16>, dim3(64), dim3(256), 0, s, w, (__bf16*)out, cout, cin);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
