// 3x3 stride-1 'same' convolution as an implicit GEMM on CDNA4 MFMA
// (v_mfma_f32_32x32x16_bf16), channel-blocked bf16 activations, fp32 accumulation.
//
// Replaces the ATen convolution behind Conv / ConvWithoutBN / RDB / RRDB /
// Scaler of the reference (utils/models.py:75-111, 174-199, 245-271, 298-317,
// 572-589) together with their BN (folded), LeakyReLU, torch.cat, residual
// add/mul and PixelShuffle, which all become the epilogue of one launch.
//
// Block tile: TH = R*WM output rows x 32 output columns x CT = NF*32 output
// channels; wave w owns rows [w*R, w*R+R).  GEMM view per block:
//   M = 32 pixels of one row (one MFMA row-fragment per output row),
//   N = CT output channels (NF fragments of 32),
//   K = 9 taps x Cin, walked in chunks of KC (16 or 32) input channels.
// Activations are [N][C/16][H][W][16]: a K-chunk is KC/16 contiguous planes, so
// each halo row of a chunk is one contiguous 34 x 32-byte run (whole cache
// lines).  Per chunk the (TH+2) x 34 halo planes and the chunk's packed weights
// are copied global → LDS with global_load_lds_dwordx4 into an NST-deep ring;
// each wave walks (k-step, dx) and re-uses every A fragment (one input row) for
// the up-to-3 output rows (dy taps) that read it: R+2 A reads feed 3*R*NF MFMAs.
// The epilogue transposes one output row at a time through LDS so that every
// lane stores 16 contiguous bytes (8 channels) of one pixel.
// Grid: 1D, XCD-aware (xcd_remap) with the cout tile innermost, then x, y, image.
#include <string.h>

#include "isr_common.h"
#include "dispatch.h"

namespace isr {

// Timing stamps (tuning builds only, isr_tuning_conv_stamps): per block, wall-clock
// (s_memrealtime, 100 MHz) at entry / first chunk landed / main loop done / epilogue
// done, plus the raw HW_ID and XCC_ID registers.  Written by a vector store of lane 0
// of wave 0 into a buffer of its own (never read by the kernel).
#ifdef ISR_TUNING
__device__ unsigned long long* g_conv_stamps;
#endif
__device__ __forceinline__ void conv_stamp(int slot) {
#ifdef ISR_TUNING
    unsigned long long* p = g_conv_stamps;
    if (p != nullptr && threadIdx.x == 0) {
        unsigned long long t;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");  // not hoistable
        p[(size_t)blockIdx.x * 8 + slot + threadIdx.x] = t;
        if (slot == 0) {
            const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);   // HW_REG_HW_ID
            const unsigned xcc = __builtin_amdgcn_s_getreg((15 << 11) | (0 << 6) | 20); // HW_REG_XCC_ID
            p[(size_t)blockIdx.x * 8 + 6 + threadIdx.x] = hw;
            p[(size_t)blockIdx.x * 8 + 7 + threadIdx.x] = xcc;
        }
    }
#else
    (void)slot;
#endif
}

// Knobs of one tile configuration, with their defaults: a named configuration (K_* below) derives
// from this and shadows the knobs in which it differs; C3<K> adds everything that follows from them.
struct C3Knobs {
    // output rows per wave, waves per block, 32-cout fragments per block, input channels per
    // chunk (16 or 32), chunk ring depth
    static constexpr int R = 4, WM = 4, NF = 1, KC = 16, NST = 2;
    // storage type of activations and weights: false = bf16, true = fp16 (isr_conv_desc.f16, inference)
    static constexpr bool H = false;
    // 1: the RDB residual fold (r1 == the conv's own input channels, see fold_ok) is compiled in;
    // only the RDB final-conv instantiations carry it (it costs registers)
    static constexpr int FOLD = 0;
    // 0: each step's fragments read right before its MFMAs; 1: double-buffered fragment registers
    // across (k-step, dx) steps; 2: the next step's reads spread over the current step's MFMAs
    // (front-loading them instead: 0.43-0.92x, register pressure)
    static constexpr int PIPE = 0;
    // refill placement with PIPE 2: false = the next chunk's LDS-DMA issued right after the current
    // chunk's step-0 fragment reads, true = issued before them (round-1 order; as without PIPE 2)
    static constexpr bool REFILL_FIRST = false;
    // tap window: 0 = all 3x3 taps; 1 = taps {0,1}^2; 2 = taps {1,2}^2 (the 2x2 convs that a
    // stride-2 3x3 conv and its transpose become on the 2x2 phase decomposition, isr_conv_desc.taps)
    static constexpr int TWN = 0;
    static constexpr int CIN = 0; // 0 = runtime cin; else compile-time (own symbol)
    // Ablation bits, tuning builds only (outputs wrong): 1 = no MFMA (operands
    // kept live), 2 = stage only chunk 0 (no refill), 4 = no epilogue stores, 8 = the weights of
    // chunk 0 only (later chunks refill their halo but not their weights: the time a block would
    // take with its weights resident in LDS, round 6 probe for the Scaler / VGG short-K convs).
    static constexpr int ABL = 0;
};

template <class K>
struct C3 : K {
    static constexpr int TLO = K::TWN == 2 ? 1 : 0;
    static constexpr int TN = K::TWN ? 2 : 3;
    static constexpr int NA = K::R + TN - 1;  // input rows one wave reads per step
    static constexpr int TH = K::R * K::WM;
    static constexpr int TW = 32;
    static constexpr int HR = TH + 2;  // halo rows
    static constexpr int HC = TW + 2;  // halo cols
    static constexpr int CT = K::NF * 32; // output channels per block
    static constexpr int KS = K::KC / 16; // MFMA k-steps (= planes) per chunk
    static constexpr int HQ = HR * HC; // halo pixels per plane
    static constexpr int HIPL = (HQ + 31) / 32; // glds instructions per plane (32 px x 32 B each)
    static constexpr int HALO_INSTR = KS * HIPL;
    static constexpr int W_INSTR = 9 * KS * CT / 32; // [ks][tap][n][hpos] x 16 B
    static constexpr int INSTR = HALO_INSTR + W_INSTR;
    static constexpr int IPW = (INSTR + K::WM - 1) / K::WM; // glds per wave per chunk (uniform)
    static constexpr int STAGE = IPW * K::WM * 1024;
    static constexpr int RING = K::NST * STAGE;
    static constexpr int NT = 64 * K::WM;
    static constexpr int EPS = CT + 4;                 // floats per pixel in the epilogue image
    static constexpr int EP_BYTES = K::WM * 32 * EPS * 4; // one output row per wave at a time
    static constexpr int LDS = (RING > EP_BYTES) ? RING : EP_BYTES;
    static constexpr int BPC = 163840 / LDS; // blocks per CU by LDS
    static constexpr int OCC = BPC * K::WM / 4 >= 2 ? 2 : 1; // waves per SIMD to budget registers for
    static_assert(LDS <= 163840, "LDS budget");
    static_assert(K::KC == 16 || K::KC == 32, "chunk width");
    static_assert(!K::REFILL_FIRST || K::PIPE == 2, "REFILL_FIRST picks between the two orders of PIPE 2");
};

template <int V> struct IC { static constexpr int value = V; };

// A operand of the residual fold: (1/s1) I on couts [16 h16, 16 h16 + 16) of a 32-cout
// fragment (lane l supplies A[l & 31][8 (l >> 5) .. + 8]); trunk.hip builds the same.
template <bool H>
__device__ __forceinline__ uint32_t fold_idv(float s1) {  // storage-type bits of 1/s1, in an SGPR
    return __builtin_amdgcn_readfirstlane((uint32_t)bits16<H>(1.f / s1));
}
__device__ __forceinline__ bf16x8 fold_a(uint32_t idv, int h16) {
    int lane = threadIdx.x & 63;
    // opaque to the optimiser: built next to its one use instead of hoisted out of the chunk
    // loop (two hoisted operands = 8 VGPRs the 256-VGPR final-conv kernel does not have)
    asm volatile("" : "+v"(lane));
    const int j = (lane & 31) - 16 * h16 - 8 * (lane >> 5);
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    u32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = j == 2 * k ? idv : (j == 2 * k + 1 ? idv << 16 : 0u);
    return __builtin_bit_cast(bf16x8, r);
}

// The fold applies when r1 is exactly the conv's own input channels [0, cout) (one cout tile),
// the activation is the identity and 1/s1 is exact in bf16 (add_rate 0.2 → 5).
template <class C, bool XS2>
__device__ __forceinline__ bool fold_ok(const isr_conv_desc& d) {
    if constexpr (!C::FOLD || C::NF != 2 || C::KS != 1 || C::TN != 3 || C::PIPE != 2 || XS2) {
        return false;
    } else {
        if (!d.r1.data || d.r1.data != d.x.data || d.r1.coff != d.x.coff || d.r1_cn != 0) return false;
        if (d.cout != C::CT || d.slope != 1.f || d.y2.data || d.m.data || d.shuffle != 1) return false;
        const float inv = 1.f / d.s1;
        if constexpr (C::H) return (float)(_Float16)inv == inv;
        else return (float)(__bf16)inv == inv;
    }
}

// Epilogue.  Accumulators are D[cout][pixel]: lane l owns pixel l31 of the row
// and couts (g&3) + 8*(g>>2) + 4*hh of each 32-cout fragment; the bias is
// already in them (accumulator init).
//  * plain stores (MODE 0..7): two v_permlane32_swap rounds per fragment give
//    every lane 8 contiguous couts twice, so each store is 16 bytes and one
//    store instruction covers 32 pixels x 32 contiguous bytes; no LDS, no
//    barrier.  All residual loads of a row are issued before its stores (the
//    output may alias a residual: the in-place RRDB update).
//  * PixelShuffle(2) (MODE 8): transpose through LDS one row at a time, so a
//    lane stores 8 channels of one shuffled output pixel.
// MODE bits (compile-time: no per-element branches): 1 = r1, 2 = r2, 4 = y2, 8 = shuffle,
// 16 = LeakyReLU' mask (backward).  r1_cn / m_c0 are multiples of 32, so their
// channel tests are uniform per 32-cout fragment (scalar branches).
template <class C, int MODE>
__device__ __forceinline__ void epilogue(const isr_conv_desc& d, f32x16 (&acc)[C::R][C::NF], int img, int ct,
                                         int x0, int y0, int wave, int lane) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = C::R, NF = C::NF, CT = C::CT, EPS = C::EPS;
    const int l31 = lane & 31, hh = lane >> 5;
    const float slope = d.slope;
    if constexpr (MODE & 8) {
        constexpr int ITEMS = CT / 16; // items (8 channels of one shuffled pixel) per lane per row
        constexpr int CG = CT / 32;
        float* ep = reinterpret_cast<float*>(smem) + wave * (32 * EPS);
        const int cg = lane % CG;
        const int sj = (lane / CG) & 1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // registers 4j..4j+3 are 4 consecutive couts (the 4 sub-pixels of one shuffled
            // channel): one 16-byte write each (lane units 17·l31 + 2j + hh: conflict-free)
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 q = {acc[r][f][4 * j], acc[r][f][4 * j + 1], acc[r][f][4 * j + 2], acc[r][f][4 * j + 3]};
                    *reinterpret_cast<f32x4*>(ep + l31 * EPS + f * 32 + 8 * j + 4 * hh) = q;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            const int yy = y0 + wave * R + r;
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                // item → sub-row si (compile-time), output column xo, channel group cg
                const int si = it / CG;
                const int xo = (lane / CG + 64 * it / CG) & 63;
                const int xc = xo >> 1;
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    v[k] = ep[xc * EPS + 4 * (cg * 8 + k) + 2 * si + sj];
                    v[k] = v[k] >= 0.f ? v[k] : v[k] * slope;
                }
                if constexpr (MODE & 16) {  // LeakyReLU' of the (shuffled-grid) mask source, all channels
                    const bf16x8 mq =
                        load16(view_at(d.m, img, 2 * yy + si, 2 * x0 + xo, ct * (CT / 4) + cg * 8));
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (!(elt<C::H>(mq, k) > 0.f)) v[k] *= d.mslope;
                }
                if (!(yy < d.h && x0 + xc < d.w)) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = 0.f;
                }
                store8_t<C::H>(view_at(d.y, img, 2 * yy + si, 2 * x0 + xo, ct * (CT / 4) + cg * 8), v);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
    } else {
        const int xx = x0 + l31;
        // Residual / mask operands are loaded U (row, fragment) units at a time,
        // all loads of a pass before any of its stores, so the epilogue waits
        // for memory R*NF/U times instead of once per unit.  U is sized so the
        // operand registers stay at <= 32 VGPRs beside the 128 accumulators.
        // Loads of a unit precede its stores (in-place RRDB update: y may alias r1/r2).
        constexpr int P = ((MODE & 1) ? 1 : 0) + ((MODE & 2) ? 1 : 0) + ((MODE & 16) ? 1 : 0);
        constexpr int NU = R * NF;
        constexpr int U0 = P == 0 ? 1 : 4 / P;  // 4 operand units (8 VGPRs each) loaded per pass
        constexpr int U = U0 > NU ? NU : U0;
        static_assert(NU % U == 0, "units per pass");
        bf16x8 q1[U][2], q2[U][2], qm[U][2];
        auto load_unit = [&](int uu, int buf) {
            const int r = uu / NF, f = uu % NF;
            const int yy = y0 + wave * R + r;
            const int cf = ct * CT + f * 32;
            const bool use_r1 = (MODE & 1) && (d.r1_cn == 0 || cf < d.r1_cn);
            const bool use_m = (MODE & 16) && cf >= d.m_c0;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int co = cf + 16 * blk + 8 * hh;
                if constexpr (MODE & 1) {
                    if (use_r1) q1[buf][blk] = load16(view_at(d.r1, img, yy, xx, co));
                }
                if constexpr (MODE & 2) q2[buf][blk] = load16(view_at(d.r2, img, yy, xx, co));
                if constexpr (MODE & 16) {
                    if (use_m) qm[buf][blk] = load16(view_at(d.m, img, yy, xx, co));
                }
            }
        };
        const bool scale2 = d.s2 != 1.f;  // s2 also scales when there is no r2 (backward)
#pragma unroll
        for (int uu = 0; uu < NU; ++uu) {
            const int r = uu / NF, f = uu % NF, cb = uu % U;
            const int yy = y0 + wave * R + r;
            const bool valid = yy < d.h && xx < d.w;
            if constexpr (P > 0) {
                if (cb == 0) {
#pragma unroll
                    for (int i = 0; i < U; ++i) load_unit(uu + i, i);
                }
            }
            const int cf = ct * CT + f * 32;
            const bool use_r1 = (MODE & 1) && (d.r1_cn == 0 || cf < d.r1_cn);
            const bool use_m = (MODE & 16) && cf >= d.m_c0;
            float v[16];
#pragma unroll
            for (int g = 0; g < 16; ++g) v[g] = acc[r][f][g];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                swap_halves(v[k], v[4 + k]);
                swap_halves(v[8 + k], v[12 + k]);
            }
            // v[8*blk + e] = cout f*32 + 16*blk + 8*hh + e
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                float* u = v + 8 * blk;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    u[e] = u[e] >= 0.f ? u[e] : u[e] * slope;
                    if constexpr (MODE & 32) u[e] = u[e] * d.s1;
                    if constexpr (MODE & 1) u[e] = u[e] * d.s1 + (use_r1 ? elt<C::H>(q1[cb][blk], e) : 0.f);
                    if constexpr (MODE & 2) {
                        u[e] = u[e] * d.s2 + elt<C::H>(q2[cb][blk], e);
                    } else {
                        if (scale2) u[e] *= d.s2;
                    }
                    if constexpr (MODE & 16) {
                        if (use_m && !(elt<C::H>(qm[cb][blk], e) > 0.f)) u[e] *= d.mslope;
                    }
                    if (!valid) u[e] = 0.f;
                }
                const int co = cf + 16 * blk + 8 * hh;
                store8_t<C::H>(view_at(d.y, img, yy, xx, co), u);
                if constexpr (MODE & 4) store8_t<C::H>(view_at(d.y2, img, yy, xx, co), u);
            }
        }
    }
}

// Packed weights (isr_pack_conv3x3): [c16 = cin/16][tap 9][cout][hpos 2][8 bf16],
// element = W[n][c16*16 + h*8 + e][tap], h = hpos ^ ((n >> 3) & 1).
// XS2: the input is read as PixelShuffle(2)ᵀ (isr_conv_desc.x_sub2) — a template flag so the
// common path carries no per-chunk address division.
// One output tile (logical tile index t: cout tile innermost, then x, y, image) of the conv
// described by `d`, computed by the whole workgroup.
template <class C, bool XS2>
__device__ __forceinline__ void conv_tile(const isr_conv_desc& d, int t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = C::R, NF = C::NF, WM = C::WM;

    const int nct = d.cout / C::CT;
    const int nbx = d.wa / C::TW, nby = d.ha / C::TH;
    const int ct = t % nct; t /= nct;
    const int bx = t % nbx; t /= nbx;
    const int by = t % nby;
    const int img = t / nby;
    const int x0 = bx * C::TW;
    const int y0 = by * C::TH;
    const int wave = wave_id();
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const int nchunks = C::CIN ? C::CIN / C::KC : d.cin / C::KC;
    // RDB residual fold (trunk.hip): when r1 is the conv's own input channels [0, cout) and the
    // activation is the identity, x/s1 is added by extra MFMAs on the staged centre pixels
    // (A = (1/s1) I, exact in bf16) and the epilogue computes acc * s1 — no r1 re-read.  The
    // same MFMA order as trunk.hip's kernel, so every path stays bit-identical.
    const bool fold = fold_ok<C, XS2>(d);
    const uint32_t fidv = C::FOLD ? fold_idv<C::H>(d.s1) : 0u;
    conv_stamp(0);

    // ---- per-lane glds source offsets (chunk-invariant) -------------------
    // x_sub2 (backward of PixelShuffle): halo pixel (row, col) of sub-position s
    // lives at x pixel (2row + (s>>1), 2col + (s&1)) — pixel stride 2 plus a
    // per-chunk offset.
    const int ps = XS2 ? 2 : 1;
    const char* xbase = view_at(d.x, img, ps * (y0 - 1), ps * (x0 - 1), 0);
    const size_t pstride = plane_bytes(d.x);
    const char* wbase = (const char*)d.wpack;
    const int xrow_bytes = d.x.wp * 32;
    auto xchunk = [&](int chunk) -> size_t {
        if constexpr (!XS2) return (size_t)chunk * C::KS * pstride;
        const int cs4 = d.cin >> 2;
        const int c0 = chunk * C::KC;
        const int sp = c0 / cs4, cb = (c0 - sp * cs4) >> 4;
        return (size_t)cb * pstride + (size_t)(sp >> 1) * xrow_bytes + (sp & 1) * 32;
    };
    const size_t wchunk_bytes = (size_t)C::KS * 9 * d.cout * 32;
    // recomputed per stage instead of held in IPW registers (the wide kernel sits at the
    // 256-VGPR limit of two waves per SIMD)
    auto off_of = [&](int k) -> uint32_t {
        const int j = wave + WM * k;
        uint32_t o = 0;
        if (j < C::HALO_INSTR) {
            const int kp = j / C::HIPL;
            const int u = (j - kp * C::HIPL) * 64 + lane;
            const int q = u >> 1;
            if (q < C::HQ) {
                const int row = q / C::HC;
                const int col = q - row * C::HC;
                const int c = (u & 1) ^ ((q >> 3) & 1);
                o = (uint32_t)(kp * pstride + ps * (row * xrow_bytes + col * 32) + c * 16);
            }
        } else if (j < C::INSTR) {
            const int u = (j - C::HALO_INSTR) * 64 + lane;
            const int seg = u / (C::CT * 2); // (ks, tap)
            const int rem = u - seg * (C::CT * 2);
            o = (uint32_t)((seg * d.cout + ct * C::CT) * 32 + rem * 16);
        }
        return o;
    };

    auto stage = [&](int chunk, int buf) {
        char* dst = smem + buf * C::STAGE;
        const char* xs = xbase + xchunk(chunk);
        const char* ws = wbase + (size_t)chunk * wchunk_bytes;
#pragma unroll
        for (int k = 0; k < C::IPW; ++k) {
            const int j = wave + WM * k;
            const uint32_t o = off_of(k);
            if (j < C::HALO_INSTR) {
                glds16(xs + o, dst + j * 1024);
            } else if (!(C::ABL & 8) || chunk == 0) {
                glds16(ws + o, dst + j * 1024);
            }
        }
    };

    // D[cout][pixel] accumulators (A = weights, B = pixels): register g of lane l
    // holds cout f*32 + (g&3) + 8*(g>>2) + 4*hh of pixel l31; the bias is the init.
    f32x16 acc[R][NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        f32x16 b0;
#pragma unroll
        for (int g = 0; g < 16; ++g)
            b0[g] = d.bias ? d.bias[ct * C::CT + f * 32 + (g & 3) + 8 * (g >> 2) + 4 * hh] : 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][f] = b0;
    }

    auto prologue = [&]() {
#pragma unroll
        for (int s = 0; s < C::NST - 1; ++s)
            if (s < nchunks) stage(s, s);
    };
    prologue();
    conv_stamp(5);

    const int qw = wave * R * C::HC + l31; // halo pixel of (row w*R, col l31)
    // one K-chunk; FC = the chunk index (0..3) when the residual fold adds its MFMAs to this chunk,
    // -1 otherwise (the fold's chunks are peeled so that its accumulator choice is compile-time:
    // a run-time choice made hipcc copy a 16-VGPR accumulator and spill the 192->64 kernel)
    auto do_chunk = [&](const int chunk, auto fc_tag) {
        constexpr int FC = decltype(fc_tag)::value;
        (void)FC;
            // chunk `chunk` landed for this wave: younger chunks in flight = min(NST-2, nchunks-1-chunk)
            if constexpr (C::NST >= 3) {
                if (chunk + C::NST - 2 < nchunks) {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((C::NST - 2) * C::IPW) : "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (chunk == 0) conv_stamp(1);
            const bool refill = !(C::ABL & 2) && chunk + C::NST - 1 < nchunks;
            if constexpr (C::REFILL_FIRST || C::PIPE != 2) {
                if (refill) stage(chunk + C::NST - 1, (chunk + C::NST - 1) % C::NST);
            }

            const char* hs = smem + ((C::ABL & 2) ? 0 : (chunk % C::NST)) * C::STAGE;
            const char* ws = hs + C::HALO_INSTR * 1024;
            // Software pipeline over the chunk's (k-step, dx) steps: the fragments of
            // step st+1 are read into the other register set while step st's MFMAs
            // run, so LDS latency is covered by MFMA work of the same wave.
            constexpr int NS = C::KS * C::TN;
            constexpr int TN = C::TN, TLO = C::TLO, NA = C::NA;
            bf16x8 fb[2][TN][NF], fa[2][NA];
            auto load_step = [&](int st, int set) {
                const int ks = st / TN, dx = TLO + st % TN;
                const char* hp = hs + ks * C::HIPL * 1024;
    #pragma unroll
                for (int dyi = 0; dyi < TN; ++dyi)
    #pragma unroll
                    for (int f = 0; f < NF; ++f) {
                        const int n = f * 32 + l31;
                        const int u = ((ks * 9 + (TLO + dyi) * 3 + dx) * C::CT + n) * 2 + (hh ^ ((n >> 3) & 1));
                        fb[set][dyi][f] = lds_read16(ws + u * 16);
                    }
    #pragma unroll
                for (int ia = 0; ia < NA; ++ia) {
                    const int q = qw + (TLO + ia) * C::HC + dx;
                    fa[set][ia] = lds_read16(hp + halo_unit2(q, hh) * 16);
                }
            };
            // one fragment of step st: idx < TN*NF → weights (dyi, f), else activation row ia
            auto read_one = [&](int st, int idx, int set) {
                const int ks = st / TN, dx = TLO + st % TN;
                if (idx < TN * NF) {
                    const int dyi = idx / NF, f = idx % NF;
                    const int n = f * 32 + l31;
                    const int u = ((ks * 9 + (TLO + dyi) * 3 + dx) * C::CT + n) * 2 + (hh ^ ((n >> 3) & 1));
                    fb[set][dyi][f] = lds_read16(ws + u * 16);
                } else {
                    const int ia = idx - TN * NF;
                    int qb = qw;
                    // fold kernels: the row's swizzled address is recomputed at each read (an opaque
                    // copy of qw) — hoisted, the peeled fold chunks kept ~18 of them live and spilled
                    if constexpr (C::FOLD) asm volatile("" : "+v"(qb));
                    const int q = qb + (TLO + ia) * C::HC + dx;
                    fa[set][ia] = lds_read16(hs + ks * C::HIPL * 1024 + halo_unit2(q, hh) * 16);
                }
            };
            if constexpr (C::PIPE) load_step(0, 0);
            if constexpr (C::PIPE == 2) {
                // the refill's LDS-DMA issue (10-16 instructions, scalar address math) runs while
                // step 0's fragment reads are in flight, instead of ahead of them
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (!C::REFILL_FIRST) {
                    if (refill) stage(chunk + C::NST - 1, (chunk + C::NST - 1) % C::NST);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const int cur = C::PIPE ? (st & 1) : 0;
                if constexpr (C::PIPE == 2) {
                    // interleaved: this step's MFMAs with the next step's fragment reads (one
                    // read after each MFMA), so at most one step's reads are in flight (<= 15,
                    // the lgkmcnt range: beyond it hipcc can only wait lgkmcnt(0))
                    constexpr int NRD = TN * NF + NA;  // reads per step
                    constexpr int NM = R * TN * NF;    // MFMAs per step
                    int m = 0;

    #pragma unroll
                    for (int ia = 0; ia < NA; ++ia) {
    #pragma unroll
                        for (int dyi = 0; dyi < TN; ++dyi) {
                            const int r = ia - dyi;
                            if (r >= 0 && r < R) {
    #pragma unroll
                                for (int f = 0; f < NF; ++f) {
                                    acc[r][f] = mfma32t<C::H>(fb[cur][dyi][f], fa[cur][ia], acc[r][f]);
                                    if (st + 1 < NS)
                                        for (int k = m * NRD / NM; k < (m + 1) * NRD / NM; ++k) read_one(st + 1, k, cur ^ 1);
                                    __builtin_amdgcn_sched_barrier(0);  // pin the (MFMA, reads) order
                                    ++m;
                                }
                            }
                        }
                        if constexpr (FC >= 0 && C::FOLD && C::NF == 2 && C::KS == 1 && C::TN == 3) {
                            // residual fold: + x/s1 on the centre pixels of output row ia - 1 (dx = 1,
                            // dy = 1), right after input row ia's MFMAs (trunk.hip's order); the chunk
                            // (0..3) is a compile-time constant here, so the target accumulator is too
                            if (st == 1 && ia >= 1 && ia <= R) {
                                const bf16x8 a = fold_a(fidv, FC & 1);
                                acc[ia - 1][FC >> 1] = mfma32t<C::H>(a, fa[cur][ia], acc[ia - 1][FC >> 1]);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                    continue;
                } else if constexpr (C::PIPE) {
                    if (st + 1 < NS) load_step(st + 1, cur ^ 1);
                    // keep the prefetch ahead of this step's MFMAs (hipcc otherwise sinks
                    // each ds_read next to its first use and waits lgkmcnt(0) there)
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    load_step(st, 0);
                }
                // input row TLO+ia feeds output row r through kernel row dy = TLO+dyi: r = ia - dyi
    #pragma unroll
                for (int ia = 0; ia < NA; ++ia) {
    #pragma unroll
                    for (int dyi = 0; dyi < TN; ++dyi) {
                        const int r = ia - dyi;
                        if (r >= 0 && r < R) {
    #pragma unroll
                            for (int f = 0; f < NF; ++f) {
                                if constexpr (C::ABL & 1) {
                                    asm volatile("" ::"v"(fa[cur][ia]), "v"(fb[cur][dyi][f]));
                                } else {
                                    acc[r][f] = mfma32t<C::H>(fb[cur][dyi][f], fa[cur][ia], acc[r][f]);
                                }
                            }
                        }
                    }
                }
            }
    };
    int chunk0 = 0;
    if constexpr (C::FOLD && C::NF == 2 && C::KS == 1 && C::TN == 3) {
        if (fold && nchunks >= 4) {
            do_chunk(0, IC<0>{});
            do_chunk(1, IC<1>{});
            do_chunk(2, IC<2>{});
            do_chunk(3, IC<3>{});
            chunk0 = 4;
        }
    }
    // not unrolled: with a compile-time cin (the 192->64 kernels) hipcc unrolled all 12 chunk bodies
    // and spilled 476 B/lane (108 vs 72 us per call)
#pragma nounroll
    for (int chunk = chunk0; chunk < nchunks; ++chunk) do_chunk(chunk, IC<-1>{});
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier(); // all waves done reading the ring before it becomes the epilogue image
    conv_stamp(2);

    if constexpr (C::ABL & 4) {
        if (d.n < 0) { // never true: keeps the accumulators (and so the MFMAs) live
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int g = 0; g < 16; ++g) s += acc[r][f][g];
            ((float*)d.y.data)[threadIdx.x] = s;
        }
        return;
    }
    // ---- epilogue (mode picked once, wave-uniform, so no per-element branches)
    const int mode = d.shuffle == 2 ? (d.m.data ? 24 : 8)
                     : fold ? (32 | (d.r2.data ? 2 : 0))
                            : ((d.r1.data ? 1 : 0) | (d.r2.data ? 2 : 0) | (d.y2.data ? 4 : 0) | (d.m.data ? 16 : 0));
    switch (mode) {
        case 32: epilogue<C, 32>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 34: epilogue<C, 34>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 0: epilogue<C, 0>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 1: epilogue<C, 1>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 2: epilogue<C, 2>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 3: epilogue<C, 3>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 4: epilogue<C, 4>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 5: epilogue<C, 5>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 6: epilogue<C, 6>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 7: epilogue<C, 7>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 8: epilogue<C, 8>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 24: epilogue<C, 24>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 16: epilogue<C, 16>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 17: epilogue<C, 17>(d, acc, img, ct, x0, y0, wave, lane); break;
        case 18: epilogue<C, 18>(d, acc, img, ct, x0, y0, wave, lane); break;
        default: epilogue<C, 19>(d, acc, img, ct, x0, y0, wave, lane); break;  // 19; y2 + mask is rejected by isr_conv3x3_fwd
    }
#ifdef ISR_TUNING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    conv_stamp(3);
#endif
}

template <class C, bool XS2>
__global__ __launch_bounds__(C::NT, C::OCC) void conv3x3_fwd_kernel(isr_conv_desc d) {
    conv_tile<C, XS2>(d, xcd_remap(blockIdx.x, gridDim.x));
}

template <class C, bool XS2>
static int launch3x3_k(const isr_conv_desc* d, hipStream_t s) {
    auto kern = conv3x3_fwd_kernel<C, XS2>;
    lds_limit((const void*)kern, C::LDS);
    const int blocks = (d->wa / C::TW) * (d->ha / C::TH) * d->n * (d->cout / C::CT);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(C::NT), C::LDS, s, *d);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// FULL: the production tiles also carry the PixelShuffleᵀ-input form; the A/B variants
// take the plain form only (x_sub2 → unsupported).
template <class C, bool FULL = false>
static int launch3x3(const isr_conv_desc* d, hipStream_t s) {
    if (d->cout % C::CT || d->cin % C::KC || d->ha % C::TH) return DISPATCH_UNSUPPORTED;
    if (C::CIN && d->cin != C::CIN) return DISPATCH_UNSUPPORTED;
    if constexpr (FULL) {
        if (d->x_sub2) return launch3x3_k<C, true>(d, s);
    } else {
        if (d->x_sub2) return DISPATCH_UNSUPPORTED;
    }
    return launch3x3_k<C, false>(d, s);
}

// Variant table: variant 0 is the production choice per shape; the others are
// kept for on-device A/B tuning (isr_conv3x3_fwd_variant, tools/tune_conv.py).
// (tools/tune_conv.py on MI355X, N=16 128²: the 16x32-tile, 2-blocks/CU configs are
// fastest on every shape of the generator; the 32x32 8-wave tiles win only at long K)
// A K_* record spells the knobs in which it differs from C3Knobs (or from the record it derives
// from); V_* = C3<K_*> are the production tiles.
// V_G0 / V_F0: the next step's fragment reads interleaved one per MFMA (PIPE 2): 2-7 % over the
// batched prefetch, whose 18-24 reads in flight exceed lgkmcnt's range (so hipcc waited lgkmcnt(0))
// cout == 32 (RDB growth convs): 16x32, 4 waves, KC16 double buffer, 58 KB → 2 blocks / CU
struct K_G0 : C3Knobs { static constexpr int PIPE = 2; };
// cout % 64 == 0: 16x32, 4 waves, KC16 double buffer, 76 KB → 2 blocks / CU
struct K_W0 : C3Knobs { static constexpr int NF = 2, PIPE = 2; };
struct K_F0 : K_W0 { static constexpr int CIN = 192; };  // RDB final conv 192→64: V_W0 with compile-time cin
struct K_F0F : K_F0 { static constexpr int FOLD = 1; };  // V_F0 with the residual fold (r1 == x)
// fp16 storage (isr_conv_desc.f16: the inference path) — the same four production tiles
struct K_G0H : K_G0 { static constexpr bool H = true; };
struct K_W0H : K_W0 { static constexpr bool H = true; };
struct K_F0H : K_F0 { static constexpr bool H = true; };
struct K_F0FH : K_F0F { static constexpr bool H = true; };
// tap windows {0,1}^2 / {1,2}^2 (isr_conv_desc.taps 1 / 2): the V_W0 tile without the fragment pipeline
struct K_T01 : C3Knobs { static constexpr int NF = 2, TWN = 1; };
struct K_T12 : C3Knobs { static constexpr int NF = 2, TWN = 2; };
using V_G0 = C3<K_G0>; using V_W0 = C3<K_W0>; using V_F0 = C3<K_F0>; using V_F0F = C3<K_F0F>;
using V_G0H = C3<K_G0H>; using V_W0H = C3<K_W0H>; using V_F0H = C3<K_F0H>; using V_F0FH = C3<K_F0FH>;
#ifdef ISR_TUNING  // the A/B variants of conv3x3_fwd_variant (K_G1 / K_G2 prefetch, PIPE 1; K_W1 / K_W2 not)
struct K_G1 : C3Knobs { static constexpr int WM = 8, NST = 3, PIPE = 1; };  // 32x32 px tile, 8 waves, 3-deep KC16 ring
struct K_G2 : C3Knobs { static constexpr int R = 2, KC = 32, PIPE = 1; };   // 8x32, KC32, 2 blocks / CU
struct K_G3 : C3Knobs { static constexpr int R = 2, PIPE = 2; };            // 8x32 tile, double buffer, interleaved
struct K_W1 : C3Knobs { static constexpr int WM = 8, NF = 2; };             // 32x32 px tile, 8 waves, KC16 double buffer
struct K_W2 : C3Knobs { static constexpr int R = 2, NF = 2, KC = 32; };     // 8x32, KC32
struct K_W3 : C3Knobs { static constexpr int R = 2, NF = 2, PIPE = 2; };    // 8x32 tile, interleaved
struct K_G0R : K_G0 { static constexpr bool REFILL_FIRST = true; };  // variant 8: refill before step-0 reads (r1)
struct K_W0R : K_W0 { static constexpr bool REFILL_FIRST = true; };
struct K_F0R : K_F0 { static constexpr bool REFILL_FIRST = true; };
struct K_G0X8 : K_G0 { static constexpr int WM = 8; };  // variant 9: 32x32 tile, 8 waves, PIPE 2 (92 KB, 1 block/CU)
struct K_W0X8 : K_W0 { static constexpr int WM = 8; };  // (111 KB)
struct K_F0X8 : K_F0 { static constexpr int WM = 8; };
struct K_W0NW : K_W0 { static constexpr int ABL = 8; };  // timing probes (outputs wrong): V_W0 / K_W0X8
struct K_W0X8NW : K_W0X8 { static constexpr int ABL = 8; };  // without the weight refills
// ablations ABL_ of the V_G0 / V_W0 tiles (timing only, outputs wrong), with PIPE 1 / 0
template <int ABL_> struct K_GAbl : C3Knobs { static constexpr int PIPE = 1, ABL = ABL_; };
template <int ABL_> struct K_WAbl : C3Knobs { static constexpr int NF = 2, ABL = ABL_; };
#endif

// Host mirror of fold_ok: r1 is the conv's own input channels [0, cout), identity activation,
// 1/s1 exact in bf16 (its low 16 fp32 bits zero).
static bool fold_host(const isr_conv_desc* d) {
    if (!d->r1.data || d->r1.data != d->x.data || d->r1.coff != d->x.coff || d->r1_cn != 0) return false;
    if (d->cout != 64 || d->slope != 1.f || d->y2.data || d->m.data || d->shuffle != 1 || d->x_sub2 || d->taps)
        return false;
    const float inv = 1.f / d->s1;
    uint32_t bits;
    memcpy(&bits, &inv, 4);
    if (d->f16) {  // exact in fp16: 10 mantissa bits, a normal fp16 exponent
        const int ex = (int)((bits >> 23) & 0xff) - 127;
        return (bits & 0x1fffu) == 0 && ex >= -14 && ex <= 15;
    }
    return (bits & 0xffffu) == 0;
}

int conv3x3_fwd_variant(const isr_conv_desc* d, int variant, hipStream_t s) {
    if (d->f16) {  // fp16 storage: the production tiles only (the inference forward)
        if (variant != 0 || d->x_sub2 || d->taps || d->m.data) return DISPATCH_UNSUPPORTED;
        if (d->cout % 64) return launch3x3<V_G0H>(d, s);
        return d->cin == 192 ? (fold_host(d) ? launch3x3<V_F0FH>(d, s) : launch3x3<V_F0H>(d, s)) : launch3x3<V_W0H>(d, s);
    }
    if (d->cout % 64) {  // 32-cout tiles: growth convs (cout 32) and dgrad of them (96, 160)
        switch (variant) {
            case 0: return launch3x3<V_G0, true>(d, s);
#ifdef ISR_TUNING
            // A/B tile configurations (none faster than V_G0 on the generator's shapes)
            case 1: return launch3x3<C3<K_G1>>(d, s);
            case 2: return launch3x3<C3<K_G2>>(d, s);
            case 3: return launch3x3<C3<K_G3>>(d, s);
            case 8: return launch3x3<C3<K_G0R>>(d, s);
            case 9: return launch3x3<C3<K_G0X8>>(d, s);
            // ablations (timing only, outputs wrong): tuning builds only
            case 4: return launch3x3<C3<K_GAbl<1>>>(d, s);
            case 5: return launch3x3<C3<K_GAbl<2>>>(d, s);
            case 6: return launch3x3<C3<K_GAbl<4>>>(d, s);
            case 7: return launch3x3<C3<K_GAbl<3>>>(d, s);
#endif
        }
        return DISPATCH_UNSUPPORTED;
    }
    switch (variant) {
        case 0: return d->cin == 192 ? (fold_host(d) ? launch3x3<V_F0F>(d, s) : launch3x3<V_F0, true>(d, s))
                                     : launch3x3<V_W0, true>(d, s);
#ifdef ISR_TUNING
        case 1: return launch3x3<C3<K_W1>>(d, s);
        case 2: return launch3x3<C3<K_W2>>(d, s);
        case 3: return launch3x3<C3<K_W3>>(d, s);
        case 8: return d->cin == 192 ? launch3x3<C3<K_F0R>>(d, s) : launch3x3<C3<K_W0R>>(d, s);
        case 9: return d->cin == 192 ? launch3x3<C3<K_F0X8>>(d, s) : launch3x3<C3<K_W0X8>>(d, s);
        // timing probes (outputs wrong): V_W0 / variant 9 without the weight refills (ABL 8)
        case 10: return launch3x3<C3<K_W0NW>>(d, s);
        case 11: return launch3x3<C3<K_W0X8NW>>(d, s);
        // ablations (timing only, outputs wrong): tuning builds only
        case 4: return launch3x3<C3<K_WAbl<1>>>(d, s);
        case 5: return launch3x3<C3<K_WAbl<2>>>(d, s);
        case 6: return launch3x3<C3<K_WAbl<4>>>(d, s);
        case 7: return launch3x3<C3<K_WAbl<3>>>(d, s);
#endif
    }
    return DISPATCH_UNSUPPORTED;
}

#ifdef ISR_TUNING
int conv_stamps_set(void* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_conv_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -1; }
#else
int conv_stamps_set(void*) { return DISPATCH_UNSUPPORTED; }
#endif

int conv3x3_fwd_dispatch(const isr_conv_desc* d, hipStream_t s) {
    if (d->f16) return conv3x3_fwd_variant(d, 0, s);
    if (d->taps == 1) return d->cout % 64 ? DISPATCH_UNSUPPORTED : launch3x3<C3<K_T01>, true>(d, s);
    if (d->taps == 2) return d->cout % 64 ? DISPATCH_UNSUPPORTED : launch3x3<C3<K_T12>, true>(d, s);
    return conv3x3_fwd_variant(d, 0, s);
}

// ---- weight packing: fp32 OIHW → bf16 [c16][tap][cout][hpos][8] -----------
// Forward: the packed conv has (cout, cin) = the layer's, element W[n][ci][tap].
// dgrad (transposed): the packed conv maps the layer's output gradient (cin' =
// layer cout) to its input gradient (cout' = layer cin): element
// scale * W[co(ci')][n][8 - tap] (180° rotation), where with sub2 the input
// channel ci' = s*(layer cout/4) + c stands for layer channel co = 4c + s
// (PixelShuffle order, see isr_conv_desc.x_sub2).
template <class OT = __bf16>
__device__ __forceinline__ void pack3x3_range(const float* __restrict__ w, OT* __restrict__ out, int pcout,
                                              int pcin, int transposed, int sub2, float scale, size_t first,
                                              size_t stride, int src_n0 = 0, int src_cin = 0) {
    // dgrad window: packed output channel n = layer input channel src_n0 + n of a layer with
    // src_cin input channels (row stride of w); 0 → the whole layer (src_cin = pcout)
    const int wrow = src_cin > 0 ? src_cin : pcout;
    const size_t total = (size_t)pcout * pcin * 9;
    for (size_t idx = first; idx < total; idx += stride) {
        size_t rem = idx;
        const int e = rem % 8; rem /= 8;
        const int hpos = rem % 2; rem /= 2;
        const int n = rem % pcout; rem /= pcout;
        const int tap = rem % 9; rem /= 9;
        const int c16 = (int)rem;
        const int h = hpos ^ ((n >> 3) & 1);
        const int ci = c16 * 16 + h * 8 + e;
        float v;
        if (!transposed) {
            v = w[((size_t)n * pcin + ci) * 9 + tap];
        } else {
            const int cs4 = pcin >> 2;
            const int co = sub2 ? (ci % cs4) * 4 + ci / cs4 : ci;  // layer output channel
            v = w[((size_t)co * wrow + src_n0 + n) * 9 + (8 - tap)];  // layer W[co][n0 + n][8 - tap]
        }
        out[idx] = (OT)(v * scale);
    }
}

template <class OT>
__global__ void pack3x3_kernel(const float* __restrict__ w, OT* __restrict__ out, int pcout, int pcin,
                               int transposed, int sub2, float scale) {
    pack3x3_range<OT>(w, out, pcout, pcin, transposed, sub2, scale, blockIdx.x * (size_t)blockDim.x + threadIdx.x,
                      (size_t)gridDim.x * blockDim.x);
}

// Many packs in one launch (the training plan repacks every conv each step):
// blockIdx.y = item, blockIdx.x strides over that item's elements.
__global__ void pack3x3_batch_kernel(const isr_pack_item* __restrict__ items) {
    const isr_pack_item it = items[blockIdx.y];
    const int pcout = it.dgrad ? it.cin : it.cout, pcin = it.dgrad ? it.cout : it.cin;
    pack3x3_range(it.w, (__bf16*)it.out, pcout, pcin, it.dgrad, it.sub2, it.dgrad ? it.scale : 1.f,
                  blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x,
                  it.dgrad ? it.src_n0 : 0, it.dgrad ? it.src_cin : 0);
}

int conv3x3_pack_batch(const isr_pack_item* items, int n, hipStream_t s) {
    hipLaunchKernelGGL(pack3x3_batch_kernel, dim3(96, n), dim3(256), 0, s, items);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

size_t conv3x3_packed_bytes(int cout, int cin) { return (size_t)cout * cin * 9 * 2; }

static int pack_launch(const float* w, void* out, int pcout, int pcin, int transposed, int sub2, float scale,
                       hipStream_t s) {
    const size_t total = conv3x3_packed_bytes(pcout, pcin) / 2;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack3x3_kernel<__bf16>, dim3(blocks), dim3(256), 0, s, w, (__bf16*)out, pcout, pcin, transposed,
                       sub2, scale);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int conv3x3_pack(const float* w, void* out, int cout, int cin, hipStream_t s) {
    return pack_launch(w, out, cout, cin, 0, 0, 1.f, s);
}

// the forward pack in fp16 (isr_conv_desc.f16): same layout and size
int conv3x3_pack_f16(const float* w, void* out, int cout, int cin, hipStream_t s) {
    const size_t total = conv3x3_packed_bytes(cout, cin) / 2;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack3x3_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, w, (_Float16*)out, cout, cin, 0, 0,
                       1.f);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// layer weights [cout][cin][3][3] → packed dgrad conv (cout' = cin, cin' = cout)
int conv3x3_pack_dgrad(const float* w, void* out, int cout, int cin, float scale, int sub2, hipStream_t s) {
    return pack_launch(w, out, cin, cout, 1, sub2, scale, s);
}

}  // namespace isr
