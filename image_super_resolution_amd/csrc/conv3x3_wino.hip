// 3x3 stride-1 'same' convolution by 1-D Winograd F(2,3) along x on CDNA4 MFMA
// (v_mfma_f32_32x32x16_f16), channel-blocked fp16 activations, fp32 accumulation.
// An opt-in inference alternative to conv3x3.hip's direct form (isr_conv3x3_wino_fwd): 4 MFMA
// products per output pair and kernel row instead of 6.  Not bit-identical to the direct form.
//
// Per kernel row ky, input channel c and output pair j (outputs x = 2j, 2j+1; inputs
// d0..d3 = x[2j-1 .. 2j+2]; taps g0..g2 = W[co][c][ky][0..2]):
//   V0 = d0 - d2   V1 = d1 + d2   V2 = d2 - d1   V3 = d1 - d3   (packed fp16 adds: rounded once)
//   U0 = g0   U1 = (g0+g1+g2)/2   U2 = (g0-g1+g2)/2   U3 = g2   (fp32 → fp16 at pack time)
//   M_p = sum_{ky,c} U_p V_p                                    (fp32, one accumulator set per p)
//   y(2j) = M0 + M1 + M2       y(2j+1) = M1 - M2 - M3           (fp32, epilogue)
// then conv3x3.hip's epilogue: v = act(y + bias); v = v*s1 + r1; v = v*s2 + r2; store y, y2.
//
// Block tile: TH = R*WR output rows x 64 output columns (32 pairs) x CT = 32*WC output channels,
// WR x WC waves; wave (wr, wc) owns rows [wr*R, wr*R+R) and couts [wc*32, wc*32+32).  GEMM view
// per wave and row: M = 32 couts (A = U_p), N = 32 pairs (B = V_p), K = 16 input channels per
// chunk; four accumulator sets per output row (R = 2: the direct tile's 128 accumulator VGPRs).
// Per chunk the (TH+2) x 66 halo pixels of one 16-channel plane and the chunk's 12 x CT
// transformed weights are copied global → LDS (global_load_lds_dwordx4) into a 2-deep ring.
// The DMA's source address is free per 16 bytes, so the LDS halo image is de-interleaved:
// row image = [parity of the halo column][channel half][33 columns] x 16 B.  With E[k] = halo
// column 2k and O[k] = column 2k+1: d0 = E[j], d1 = O[j], d2 = E[j+1], d3 = O[j+1] — each one
// ds_read_b128 at a 16-byte lane stride.  The input transform runs in registers on the
// fragments a wave has just read; every V fragment feeds the up-to-R output rows that read
// its input row.
//
// Width guard: buffers are allocated to wa % 32 == 0 (row pitch wa + 2 pad), the tile is 64 wide.
// On an odd multiple of 32 the last tile of a row is a half tile: halo columns past x = wa are
// read from column x = wa instead (the border; they feed only outputs that are not stored) and
// no residual load or store is formed at x >= wa.
#include "isr_common.h"
#include "dispatch.h"

namespace isr {

template <int R_, int WR_, int WC_>
struct W3 {
    static constexpr int R = R_, WR = WR_, WC = WC_;
    static constexpr int WM = WR * WC;       // waves per block
    static constexpr int TH = R * WR;
    static constexpr int TW = 64;
    static constexpr int HR = TH + 2;        // halo rows
    static constexpr int KU = 33;            // columns per (parity, channel half) run of a halo row
    static constexpr int RU = 4 * KU;        // 16-byte units per halo row (66 px x 32 B)
    static constexpr int HU = HR * RU;       // units per halo plane
    static constexpr int HALO_INSTR = (HU + 63) / 64;  // glds instructions per chunk (64 x 16 B each)
    static constexpr int CT = 32 * WC;       // output channels per block
    static constexpr int W_INSTR = 12 * WC;  // [ky][p][CT couts] x 32 B, 1 KiB (32 couts) each
    static constexpr int INSTR = HALO_INSTR + W_INSTR;
    static constexpr int IPW = (INSTR + WM - 1) / WM;  // glds per wave per chunk
    static constexpr int STAGE = INSTR * 1024;
    static constexpr int LDS = 2 * STAGE;
    static constexpr int NT = 64 * WM;
    static constexpr int BPC = 163840 / LDS;  // blocks per CU by LDS
    static constexpr int OCC = BPC * WM / 4 >= 2 ? 2 : 1;  // waves per SIMD to budget registers for
    static_assert(LDS <= 163840, "LDS budget");
    static_assert(ISR_TILE_H % TH == 0, "row tiles must divide the computed extent");
};

template <class C>
__global__ __launch_bounds__(C::NT, C::OCC) void conv3x3_wino_kernel(isr_conv_desc d) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = C::R, WM = C::WM;

    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int nct = d.cout / C::CT;
    const int nbx = (d.wa + C::TW - 1) / C::TW, nby = d.ha / C::TH;
    const int ct = t % nct; t /= nct;
    const int bx = t % nbx; t /= nbx;
    const int by = t % nby;
    const int img = t / nby;
    const int x0 = bx * C::TW;
    const int y0 = by * C::TH;
    const int wave = wave_id();
    const int wr = wave % C::WR, wc = wave / C::WR;
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const int nchunks = d.cin / 16;

    // halo column c of the tile is pixel x0 - 1 + c; columns past x = wa (a half tile) read x = wa
    const int cmax = d.wa - x0 + 1;
    const char* xbase = view_at(d.x, img, y0 - 1, x0 - 1, 0);
    const size_t pstride = plane_bytes(d.x);
    const int xrow_bytes = d.x.wp * 32;
    const char* wbase = (const char*)d.wpack;
    const size_t wchunk_bytes = (size_t)12 * d.cout * 32;

    auto stage = [&](int chunk, int buf) {
        char* dst = smem + buf * C::STAGE;
        const char* xs = xbase + (size_t)chunk * pstride;
        const char* ws = wbase + (size_t)chunk * wchunk_bytes;
#pragma unroll
        for (int k = 0; k < C::IPW; ++k) {
            const int j = wave + WM * k;
            if (j < C::HALO_INSTR) {
                // unit u of the plane image → (row, parity, channel half, column run index)
                const int u = j * 64 + lane;
                uint32_t o = 0;
                if (u < C::HU) {
                    const int row = u / C::RU;
                    const int rem = u - row * C::RU;
                    const int ph = rem / C::KU;
                    const int kk = rem - ph * C::KU;
                    int col = 2 * kk + (ph >> 1);
                    col = col < cmax ? col : cmax;
                    o = (uint32_t)(row * xrow_bytes + col * 32 + (ph & 1) * 16);
                }
                glds16(xs + o, dst + j * 1024);
            } else if (j < C::INSTR) {
                const int u = (j - C::HALO_INSTR) * 64 + lane;
                const int seg = u / (C::CT * 2);  // ky * 4 + p
                const int rem = u - seg * (C::CT * 2);
                glds16(ws + (uint32_t)((seg * d.cout + ct * C::CT) * 32 + rem * 16), dst + j * 1024);
            }
        }
    };

    // D[cout][pair] accumulators (A = U_p, B = V_p): register g of lane l holds cout
    // (g&3) + 8*(g>>2) + 4*hh of pair l31.  M1 enters both outputs with weight +1, so the bias
    // is its initial value.
    f32x16 acc[R][4];
    {
        f32x16 b0;
#pragma unroll
        for (int g = 0; g < 16; ++g) b0[g] = d.bias ? d.bias[ct * C::CT + wc * 32 + (g & 3) + 8 * (g >> 2) + 4 * hh] : 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[r][p][g] = p == 1 ? b0[g] : 0.f;
    }

    stage(0, 0);
#pragma nounroll
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        // this wave's pieces of `chunk` landed; every wave is done reading the other buffer
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (chunk + 1 < nchunks) stage(chunk + 1, (chunk + 1) & 1);

        const char* hs = smem + (chunk & 1) * C::STAGE;
        const char* ws = hs + C::HALO_INSTR * 1024;
        bf16x8 u[3][4];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                u[ky][p] = lds_read16(ws + (((ky * 4 + p) * C::CT + wc * 32 + l31) * 2 + (hh ^ ((l31 >> 3) & 1))) * 16);
#pragma unroll
        for (int ia = 0; ia < R + 2; ++ia) {
            const char* rp = hs + ((wr * R + ia) * C::RU + hh * C::KU + l31) * 16;
            const f16x8 e0 = __builtin_bit_cast(f16x8, lds_read16(rp));
            const f16x8 o0 = __builtin_bit_cast(f16x8, lds_read16(rp + 2 * C::KU * 16));
            const f16x8 e1 = __builtin_bit_cast(f16x8, lds_read16(rp + 16));
            const f16x8 o1 = __builtin_bit_cast(f16x8, lds_read16(rp + 2 * C::KU * 16 + 16));
            bf16x8 v[4];
            v[0] = __builtin_bit_cast(bf16x8, e0 - e1);
            v[1] = __builtin_bit_cast(bf16x8, o0 + e1);
            v[2] = __builtin_bit_cast(bf16x8, e1 - o0);
            v[3] = __builtin_bit_cast(bf16x8, o0 - o1);
            // input row ia feeds output row r = ia - ky through kernel row ky
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int r = ia - ky;
                if (r >= 0 && r < R) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) acc[r][p] = mfma32t<true>(u[ky][p], v[p], acc[r][p]);
                }
            }
        }
    }

    // ---- epilogue: inverse transform, then the direct form's epilogue per output pixel.
    // Two v_permlane32_swap rounds give every lane 8 contiguous couts twice (16-byte stores).
    // A lane loads its residuals before it stores the same elements (y may alias r1 / r2).
    const int c0 = ct * C::CT + wc * 32;  // this wave's first cout
    const bool has_r1 = d.r1.data != nullptr && (d.r1_cn == 0 || c0 < d.r1_cn);
    const bool has_s1 = d.r1.data != nullptr;
    const bool has_r2 = d.r2.data != nullptr;
    const bool has_y2 = d.y2.data != nullptr;
    const bool scale2 = d.s2 != 1.f;
    const float slope = d.slope;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int yy = y0 + wr * R + r;
#pragma unroll
        for (int par = 0; par < 2; ++par) {
            const int xx = x0 + 2 * l31 + par;
            float v[16];
#pragma unroll
            for (int g = 0; g < 16; ++g)
                v[g] = par == 0 ? (acc[r][0][g] + acc[r][1][g]) + acc[r][2][g]
                                : (acc[r][1][g] - acc[r][2][g]) - acc[r][3][g];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                swap_halves(v[k], v[4 + k]);
                swap_halves(v[8 + k], v[12 + k]);
            }
            // v[8*blk + e] = cout c0 + 16*blk + 8*hh + e
            if (xx < d.wa) {
                const bool valid = yy < d.h && xx < d.w;
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    float* q = v + 8 * blk;
                    const int co = c0 + 16 * blk + 8 * hh;
                    bf16x8 q1 = {}, q2 = {};
                    if (has_r1) q1 = *reinterpret_cast<const bf16x8*>(view_at(d.r1, img, yy, xx, co));
                    if (has_r2) q2 = *reinterpret_cast<const bf16x8*>(view_at(d.r2, img, yy, xx, co));
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        q[e] = q[e] >= 0.f ? q[e] : q[e] * slope;
                        if (has_s1) q[e] = q[e] * d.s1 + (has_r1 ? elt<true>(q1, e) : 0.f);
                        if (has_r2) q[e] = q[e] * d.s2 + elt<true>(q2, e);
                        else if (scale2) q[e] *= d.s2;
                        if (!valid) q[e] = 0.f;
                    }
                    const bf16x8 o = pack8<true>(q);
                    *reinterpret_cast<bf16x8*>(view_at(d.y, img, yy, xx, co)) = o;
                    if (has_y2) *reinterpret_cast<bf16x8*>(view_at(d.y2, img, yy, xx, co)) = o;
                }
            }
        }
    }
}

// Tiles (8 waves, one block per CU, two waves per SIMD at 128 accumulator VGPRs each):
using W_G = W3<2, 8, 1>;  // cout % 64 != 0 (RDB growth convs): 16 rows x 64 columns x 32 couts, 100 KB ring
using W_W = W3<2, 4, 2>;  // cout % 64 == 0 (RDB final conv): 8 rows x 64 columns x 64 couts, 90 KB ring

template <class C>
static int launch_wino(const isr_conv_desc* d, hipStream_t s) {
    auto kern = conv3x3_wino_kernel<C>;
    lds_limit((const void*)kern, C::LDS);
    const int blocks = ((d->wa + C::TW - 1) / C::TW) * (d->ha / C::TH) * d->n * (d->cout / C::CT);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(C::NT), C::LDS, s, *d);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int conv3x3_wino_fwd_dispatch(const isr_conv_desc* d, hipStream_t s) {
    return d->cout % 64 ? launch_wino<W_G>(d, s) : launch_wino<W_W>(d, s);
}

// ---- weight packing: fp32 OIHW → fp16 [cin/16][ky 3][p 4][cout][hpos 2][8] ----------------
// element = U_p(W[n][c16*16 + h*8 + e][ky][0..2]), h = hpos ^ ((n >> 3) & 1) (the direct pack's
// swizzle: the 32 couts of an A fragment hit distinct bank slots).  U in fp32, rounded once.
__global__ void pack_wino_kernel(const float* __restrict__ w, _Float16* __restrict__ out, int cout, int cin) {
    const size_t total = (size_t)cout * cin * 12;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += stride) {
        size_t rem = idx;
        const int e = rem % 8; rem /= 8;
        const int hpos = rem % 2; rem /= 2;
        const int n = rem % cout; rem /= cout;
        const int seg = rem % 12; rem /= 12;
        const int c16 = (int)rem;
        const int ky = seg >> 2, p = seg & 3;
        const int h = hpos ^ ((n >> 3) & 1);
        const int ci = c16 * 16 + h * 8 + e;
        const float* g = w + ((size_t)n * cin + ci) * 9 + ky * 3;
        float u;
        if (p == 0) u = g[0];
        else if (p == 3) u = g[2];
        else if (p == 1) u = ((g[0] + g[1]) + g[2]) * 0.5f;
        else u = ((g[0] - g[1]) + g[2]) * 0.5f;
        out[idx] = (_Float16)u;
    }
}

size_t conv3x3_wino_packed_bytes(int cout, int cin) { return (size_t)cout * cin * 12 * 2; }

int conv3x3_wino_pack(const float* w, void* out, int cout, int cin, hipStream_t s) {
    const size_t total = conv3x3_wino_packed_bytes(cout, cin) / 2;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_wino_kernel, dim3(blocks), dim3(256), 0, s, w, (_Float16*)out, cout, cin);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace isr
