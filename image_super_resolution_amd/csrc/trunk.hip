// The RRDB trunk (utils/models.py:298-317 RRDB.forward over :245-271 RDB.forward, the
// `nn.Sequential(*RRDB)` of ResNet/EResNet :598 / :627) as ONE persistent launch: every RDB
// conv (4 growth convs 64+32k -> 32 + LeakyReLU; the final 192 -> 64 conv with the RDB and
// RRDB residuals) of every block, with tile-level dependencies instead of kernel boundaries.
//
// Running every (layer, tile) as an independent conv tile (the first persistent chain, removed:
// DESIGN.md section 5) paid descriptor round trips, a pipeline fill, the dependency wait, the
// pipeline drain and the store drain per tile and per layer, ~45 % of every RDB.  Here a
// workgroup runs ONE continuous stream of K-chunks over its (layer, tile) items:
//  * the 2-slot LDS ring never drains at a tile or layer boundary: the first chunk of the next
//    (layer, tile) is staged by LDS-DMA while the current tile's last chunk computes;
//  * a tile starts on the K-chunks its previous layer did NOT write (an RDB conv reads the
//    block input and the older growth outputs, which the previous layer's stencil wait already
//    covered) and waits for its 3x3 tile neighbourhood only before staging the first chunk the
//    previous layer wrote (`first_new`); that poll is issued one chunk ahead of the refill;
//  * no per-tile descriptor chain: a 64-byte layer record (compiled on the device from the
//    caller's isr_conv_desc table by trunk_prep_kernel) is read through the scalar cache, the
//    bias is staged into LDS with the first chunk;
//  * the RDB residual r1 = x[0:64] (the conv's own input) is added by four extra MFMAs per chunk
//    on the already-staged centre pixels (A = (1/s1) I, exact in bf16 for add_rate 0.2) instead
//    of re-reading 64 KB per tile in the epilogue: out = (acc + x/s1) * s1.  conv3x3.hip applies
//    the same fold at the same point of the same MFMA order, so the per-conv launches stay
//    bit-identical to this kernel.
// Hand-off (cdna_hip_programming.md Guideline 16, R1): write-through (sc1) output stores,
// drained by every wave before a workgroup barrier and a relaxed agent-scope progress store;
// consumers poll the 9 neighbour words (sc1 loads, per wave) and read activations with sc1
// LDS-DMA.  Progress words are serial numbers gen * 1024 + layers done (no zeroing per call).
#include "trunk_common.h"
#include "dispatch.h"

namespace isr {

size_t trunk_state_words(int n, int ha, int wa) {
    const size_t tiles = (size_t)n * (ha / tk::TH) * (wa / tk::TW);
    return trunk_rec_off((int)tiles) + 1024 * 16;
}

// ---- prep: validate the layer table and compile it into records; bump the generation ----
// err bits: 1 grid, 2 view geometry, 4 kind/cout, 8 cin/bias, 16 unsupported epilogue form,
// 32 residual form, 64 a 16-channel plane of 2 GiB or more (one buffer resource spans one plane),
// 128 too many layers.
// Growth pairs (run_tile's PH forms): layers L and L + 1 are marked 1 and 2 in rec.deps bits 12-15
// when both are kind 0 with the growth epilogue form, read the same planes of the same buffer,
// L + 1 reads 32 channels more, and those 32 are exactly what L writes (first_new(L + 1) ==
// cin(L) / 16); greedily from the left, where the order rule of trunk_pairs.h allows pairs for a
// `grid`-workgroup launch and `pair_mode` (TRUNK_PAIRS_*) asks for them.  Geometry word r0 = the
// number of paired layers.
__global__ __launch_bounds__(1024) void trunk_prep_kernel(const isr_conv_desc* layers, const int32_t* kinds, int nl,
                                                          int n, int ha, int wa, unsigned* state, int th,
                                                          int h16, int grid, int pair_mode) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned char pairable[1024];  // layer L can pair with L + 1
    __shared__ unsigned npaired;
    unsigned* err = reinterpret_cast<unsigned*>(smem);
    const int L = threadIdx.x;
    const int nbx = wa / tk::TW, nby = ha / th, ntiles = n * nbx * nby;
    const size_t ro = trunk_rec_off(ntiles);
    const bool pairs_ok = pair_mode != TRUNK_PAIRS_OFF && pairs_allowed(ntiles, nbx, nby, n, grid);
    if (L == 0) {
        *err = 0;
        npaired = 0;
    }
    pairable[L] = 0;
    __syncthreads();
    const isr_conv_desc& g0 = layers[0];
    if (L < nl) {
        const isr_conv_desc& d = layers[L];
        unsigned e = 0;
        auto same_geo = [&](const isr_view& v) {
            return v.hp == g0.x.hp && v.wp == g0.x.wp && v.cs == g0.x.cs && v.pad == g0.x.pad && v.coff % 16 == 0 &&
                   v.pad >= 1;
        };
        const int kind = kinds[L];
        // kind 2 (the training backward's RDB gather convs): a 32-cout layer whose epilogue is the
        // LeakyReLU' mask of a forward activation instead of a LeakyReLU: v = acc * (m > 0 ? 1 :
        // mslope), m = channels [m.coff, +32) of a buffer of the same geometry (no r1 / r2)
        const bool masked = kind == 2;
        if (d.n != n || d.ha != ha || d.wa != wa || d.h != g0.h || d.w != g0.w) e |= 1;
        if (!same_geo(d.x) || !same_geo(d.y) || (d.r2.data && !same_geo(d.r2)) || (masked && !same_geo(d.m))) e |= 2;
        if (kind == 0 || kind == 2 ? d.cout != 32 : (kind == 1 ? d.cout != 64 : true)) e |= 4;
        if (d.cin % 16 || d.cin < 64 || d.cin / 16 > 120 || !d.bias || ((uintptr_t)d.bias & 15)) e |= 8;
        if (d.f16 != h16 || d.shuffle != 1 || d.x_sub2 || d.taps || d.y2.data || (d.m.data != nullptr) != masked ||
            (masked && (d.m_c0 != 0 || d.slope != 1.f || d.r1.data || d.r2.data || d.s1 != 1.f || d.s2 != 1.f)))
            e |= 16;
        int fold = 0;
        uint16_t idv = 0;
        if (d.r1.data) {
            // A = (1/s1) I must be exact in the storage type (the chain's f16 flag)
            const float inv = 1.f / d.s1;
            float back;
            if (h16) {
                const _Float16 hi = (_Float16)inv;
                idv = __builtin_bit_cast(uint16_t, hi);
                back = (float)hi;
            } else {
                const __bf16 bi = (__bf16)inv;
                idv = __builtin_bit_cast(uint16_t, bi);
                back = (float)bi;
            }
            const bool alias = d.r1.data == d.x.data && d.r1.coff == d.x.coff && d.r1_cn == 0;
            if (!alias || kind != 1 || d.slope != 1.f || back != inv) e |= 32;
            fold = 1;
        } else if (d.r2.data) {
            e |= 32;
        }
        int first_new = tk::NEED_NONE;
        if (L > 0) {
            const isr_conv_desc& p = layers[L - 1];
            const int lo = p.y.coff, hi = p.y.coff + p.cout;
            first_new = d.cin / 16;  // reads nothing the previous layer wrote: wait before storing
            if (p.y.data == d.x.data) {
                for (int c = 0; c < d.cin / 16; ++c) {
                    const int c0 = d.x.coff + 16 * c;
                    if (c0 < hi && lo < c0 + 16) {
                        first_new = c;
                        break;
                    }
                }
            }
        }
        TrunkRec rec;
        rec.x = (uint64_t)(uintptr_t)d.x.data;
        rec.y = (uint64_t)(uintptr_t)d.y.data;
        rec.w = (uint64_t)(uintptr_t)d.wpack;
        rec.b = (uint64_t)(uintptr_t)d.bias;
        rec.r2 = (uint64_t)(uintptr_t)(masked ? d.m.data : d.r2.data);  // kind 2: the mask buffer
        rec.planes = (uint32_t)(d.x.coff / 16) | (uint32_t)(d.y.coff / 16) << 16;
        rec.shape = (uint32_t)((masked ? d.m.coff : d.r2.coff) / 16) | (uint32_t)(d.cin / 16) << 16 |
                    (uint32_t)(kind & 255) << 24;
        // the tile epilogue's form: what the general body tests per value, decided once here
        // (comparisons with a NaN slope or scale are false: such a layer stays general)
        int form = EPI_GENERAL;
        if (kind == 0 && !d.r1.data && !d.r2.data && d.s2 == 1.f && d.slope > 0.f && d.slope < 1.f)
            form = EPI_GROWTH;
        else if (kind == 1 && fold && d.slope == 1.f)
            form = d.r2.data ? EPI_FINAL_R2 : (d.s2 == 1.f ? EPI_FINAL : EPI_FINAL_S2);
        rec.deps = (uint32_t)first_new | (uint32_t)fold << 8 | (uint32_t)form << 9 | (uint32_t)idv << 16;
        rec.slope = masked ? d.mslope : d.slope;
        rec.s1 = d.s1;
        rec.s2 = d.s2;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&rec);
        uint32_t* dst = state + ro + (size_t)L * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[i] = src[i];
        if (e) atomicOr(err, e);
        if (pairs_ok && !e && form == EPI_GROWTH && L + 1 < nl && kinds[L + 1] == 0) {
            const isr_conv_desc& q = layers[L + 1];
            const bool q_growth = !q.r1.data && !q.r2.data && q.s2 == 1.f && q.slope > 0.f && q.slope < 1.f;
            const bool shared = q.x.data == d.x.data && q.x.coff == d.x.coff && q.cin == d.cin + 32;
            const bool feeds = d.y.data == d.x.data && d.y.coff == d.x.coff + d.cin;
            const bool wanted = pair_mode >= TRUNK_PAIRS_ALL || d.cin / 16 >= 8;
            pairable[L] = q_growth && shared && feeds && wanted && q.cout == 32 && q.f16 == h16;
        }
    }
    __syncthreads();
    if (L < nl) {
        // greedy from the left: inside a run of pairable layers every second one starts a pair
        auto first_of_pair = [&](int i) {
            if (i < 0 || !pairable[i]) return false;
            int s = i;
            while (s > 0 && pairable[s - 1]) --s;
            return ((i - s) & 1) == 0;
        };
        const unsigned pb = first_of_pair(L) ? 1u : (first_of_pair(L - 1) ? 2u : 0u);
        if (pb) {
            state[ro + (size_t)L * 16 + 12] |= pb << 12;  // rec.deps (word 12), written by this thread above
            atomicAdd(&npaired, 1u);
        }
    }
    __syncthreads();
    if (L == 0) {
        const size_t plane = (size_t)g0.x.hp * g0.x.wp * 32;  // every buffer resource spans one plane
        const unsigned e = *err | (plane >= 0x7fffffffull ? 64u : 0u) | (nl > 1024 ? 128u : 0u);
        uint32_t* geo = state + ro - 16;
        const int32_t gv[16] = {n, g0.h, g0.w, ha, wa, g0.x.hp, g0.x.wp, g0.x.cs / 16, g0.x.pad, nbx, nby, ntiles,
                                (int32_t)e, (int32_t)npaired, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; ++i) geo[i] = (uint32_t)gv[i];
        state[0] = state[0] + 1u;  // this launch's generation (a vector store by one lane)
    }
}

int trunk_prep_launch(const isr_chain_desc* cd, int th, int grid, int pair_mode, hipStream_t s) {
    hipLaunchKernelGGL(trunk_prep_kernel, dim3(1), dim3(1024), 16, s, cd->layers, cd->kinds, cd->nl, cd->n, cd->ha,
                       cd->wa, cd->state, th, cd->f16 ? 1 : 0, grid, pair_mode);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- main kernel -------------------------------------------------------------------------
#ifdef ISR_TUNING
// per (layer 75..89, tile) 8 stamps: [0] tile entry, [1] chunk 0 landed, [2] main loop done,
// [3] stores issued, [4] first dependency poll issued, [5] dependency met (s_memrealtime, 100 MHz)
__device__ unsigned long long* g_trunk_stamps;
#endif
__device__ __forceinline__ void trunk_stamp(int L, int t, int ntiles, int slot) {
#ifdef ISR_TUNING
    unsigned long long* p = g_trunk_stamps;
    if (p != nullptr && threadIdx.x == 0 && L >= 75 && L < 90) {
        unsigned long long v;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");
        p[((size_t)(L - 75) * ntiles + t) * 8 + slot] = v;
    }
#else
    (void)L, (void)t, (void)ntiles, (void)slot;
#endif
}

// Tuning builds: ablation knobs (timing only, outputs wrong): bit 1 = no halo LDS-DMA after the
// first item, 4 = no epilogue stores, 8 = no weight LDS-DMA, 16 = no dependency waits;
// [1] = workgroups per CU (host side, 0 = occupancy).  (An MFMA ablation branch inside the step
// loop would cut the MFMA/read schedule into blocks.)
#ifdef ISR_TUNING
__device__ int g_trunk_knobs[4];
static int g_trunk_per_cu = 0;
__device__ __forceinline__ int trunk_abl_load() { return __builtin_amdgcn_readfirstlane(g_trunk_knobs[0]); }
#else
__device__ __forceinline__ int trunk_abl_load() { return 0; }
#endif

// Tuning builds: per-item cycle stamps (s_memtime) for layers 77 (growth2, 8 chunks) and 79 (final,
// 12 chunks) of tile 0 of each workgroup's first tile: lane 0 of waves 0 and WM/2, 8 slots per item:
// [0] item top, [1] own DMA landed, [2] barrier passed, [3] refill issued, [4] MFMAs issued.
#ifdef ISR_TUNING
__device__ unsigned long long* g_item_stamps;
#endif
__device__ __forceinline__ void item_stamp(int L, int first_tile, int ch, int slot, int wm) {
#ifdef ISR_TUNING
    unsigned long long* p = g_item_stamps;
    const int w = wave_id();
    if (p != nullptr && first_tile && (threadIdx.x & 63) == 0 && (w == 0 || w == wm / 2) && (L == 77 || L == 79)) {
        const unsigned long long v = __builtin_amdgcn_s_memtime();
        p[((((size_t)blockIdx.x * 2 + (L == 79)) * 16 + ch) * 2 + (w != 0)) * 8 + slot] = v;
    }
#else
    (void)L, (void)first_tile, (void)ch, (void)slot, (void)wm;
#endif
}

struct TrunkArgs {
    unsigned* state;
    int rec_off;   // words
    int nl;
    int acquire;
    int keep;      // TRUNK_KEEP_* bits (trunk_keep.h)
};


// 4-byte-per-lane LDS-DMA (the bias: 64 floats = 256 B per wave instruction)
__device__ __forceinline__ void glds4(const void* gsrc, void* lds) {
    __builtin_amdgcn_global_load_lds(gsrc, ISR_LDS_PTR(lds), 4, 0, 0);
}

// The kernel's build: two 4-wave workgroups per CU (4 output rows per wave: the 16-row tile), a
// 2-slot LDS ring (one K-chunk in flight), two fragment sets (the next dx step's fragments are read
// during this step's MFMAs).  The forms that lost their A/B against it (deeper rings, 8-wave
// workgroups, 32-row tiles, one fragment set, the XCD-aware tile deal, non-temporal cache policies)
// were removed: DESIGN.md section 5.
struct TK {
    static constexpr int WM = 4, R = 4, NST = 2;
    static constexpr int HALO_AUX = 16, STORE_AUX = 16;  // sc1 on the halo LDS-DMA and the output stores
    static constexpr int NT = 64 * WM;
    static constexpr int TH = tk::TH;                     // tile rows (x 32 columns)
    static constexpr int HQ = (TH + 2) * tk::HC;          // halo pixels of a chunk
    static constexpr int HP = (HQ + 31) / 32;             // halo pieces (1 KB) per chunk
    static_assert(R * WM == TH, "the waves cover the tile rows");
    static constexpr int HPW = (HP + WM - 1) / WM;        // halo pieces per wave (at most)
    static constexpr int WPW = (tk::WPF + WM - 1) / WM;  // weight pieces per wave (at most)
    static constexpr int SLOT = (HP + tk::WPF) * 1024;
    static constexpr int BIAS_OFF = NST * SLOT;          // 4 bias slots of 256 B
    static constexpr int LDS = BIAS_OFF + 4 * 256;
    static constexpr int BPC = 2;                         // workgroups per CU
    static_assert(BPC * LDS <= 163840, "LDS budget");
    static constexpr int WPS = BPC * WM / 4;              // waves per SIMD
};

// Where the chunks of one (layer, tile) item come from (LDS-DMA through buffer resources:
// 32-bit offsets, no per-piece 64-bit address arithmetic).
struct Src {
    const char* x;   // base of the 16-channel plane chunk 0 reads (image img, plane xp)
    uint32_t h0;     // in-plane byte offset of the halo origin: pixel (y0-1, x0-1)
    const char* w;   // packed weights of chunk 0
    const float* b;  // bias
    int wpc;         // weight pieces per chunk (9 / 18)
    uint32_t xbytes, wbytes;  // extents of one activation plane and of the packed weights
    // phase 1 of a growth pair (else nullptr): the second layer's record, for its 32-cout pack (two
    // chunks longer than `w`) and its bias.  The chunk's 18 LDS pieces are the 64-cout image [tap][f]:
    // piece 2 j = tap j of `w`, piece 2 j + 1 = tap j of the second pack, both at chunk * 9 + j of
    // their own packs
    const_rec* pb;
};

struct TrunkCtx {
    unsigned* state;
    unsigned gen;
    int acquire;
    int hp, wp, cs16, pad, h, w, nbx, nby, ntiles;
    uint32_t pstride;            // bytes per 16-channel plane (< 2 GiB: prep err bit 64); every buffer
                                 // resource spans ONE plane (a per-(image, plane) base), so the
                                 // buffers themselves may be any size (the 4K still, video batches)
    uint32_t hoff[TK::HPW];       // per-lane halo piece offsets (chunk-invariant)
    int keep;                    // growth pairs keep their tile in LDS across the phase-2 hand-off
    uint32_t kbase;              // kept tiles: LDS offset of this lane's epilogue registers of its
                                 // wave's row 0 inside a slot's halo image (trunk_keep.h)
    uint32_t ring_src, ring_lds; // kept tiles: this lane's ring unit (threads 0..199), its in-plane
                                 // source offset and its LDS offset inside a slot's halo image
    int abl;                     // tuning ablation bits (0 in production builds)
};

__device__ __forceinline__ Src src_of(const TrunkCtx& c, const_rec& rec, int t) {
    const int bx = t % c.nbx, tmp = t / c.nbx, by = tmp % c.nby, img = tmp / c.nby;
    Src s;
    s.x = (const char*)(uintptr_t)rec.x + (size_t)((uint32_t)img * c.cs16 + rec_xp(rec)) * c.pstride;
    s.h0 = (uint32_t)(((by * TK::TH - 1 + c.pad) * c.wp + (bx * tk::TW - 1 + c.pad)) * 32);
    s.w = (const char*)(uintptr_t)rec.w;
    s.b = (const float*)(uintptr_t)rec.b;
    s.wpc = rec_kind(rec) == 1 ? tk::WPF : tk::WPG;  // 64 / 32 couts (kinds 0 and 2: 32)
    s.xbytes = c.pstride;
    s.wbytes = (uint32_t)(rec_nch(rec) * s.wpc * 1024);
    s.pb = nullptr;
    if (rec_pair(rec) == 1) {
        s.pb = &rec + 1;
        s.wpc = tk::WPF;  // LDS pieces per chunk; wbytes stays the extent of the 32-cout pack
    }
    return s;
}

// One chunk's LDS-DMA into ring slot `slot`: each wave its share of the 20 halo and 9 / 18
// weight pieces; wave 0 also the bias (first chunk of a tile).  Halo pieces are sc1 (L1
// bypass: other workgroups of this launch wrote them).  Returns the vector-memory instructions
// this wave issued (wave-uniform), for the counted waits.
__device__ __forceinline__ uint32_t stage_pieces(const uint32_t* hoff, uint32_t pstride, int abl, const Src& s,
                                                 int chunk, int slot, bool with_bias, int bslot, bool halo = true) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = wave_id(), lane = threadIdx.x & 63;
    char* dst = smem + slot * TK::SLOT;
    uint32_t n = 0;
    const auto rx = rsrc_n(s.x + (size_t)chunk * pstride, s.xbytes);  // chunk c = plane xp + c
    const uint32_t so = s.h0;
    if (!(abl & 1) && halo) {  // (kept tiles: weights and bias only, the halo image is written in LDS)
#pragma unroll
        for (int k = 0; k < TK::HPW; ++k) {
            const int j = wave + TK::WM * k;
            if (j < TK::HP) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, ISR_LDS_PTR(dst + j * 1024), 16, hoff[k], so, 0, TK::HALO_AUX);
                ++n;
            }
        }
    }
    // a pair's piece j = wave + WM k has the wave's parity (WM is even): one pack per wave
    static_assert(TK::WM % 2 == 0, "pair staging: a wave's pieces all come from one pack");
    const bool pair = s.pb != nullptr, second = pair && (wave & 1);
    const char* wsrc = s.w;
    uint32_t wext = s.wbytes;
    if (second) {
        wsrc = (const char*)(uintptr_t)s.pb->w;
        wext += 2 * tk::WPG * 1024;  // the second layer reads two chunks more
    }
    const auto rw = rsrc_n(wsrc, wext);
    const uint32_t wo = (uint32_t)(chunk * (pair ? tk::WPG : s.wpc) * 1024);
    char* wd = dst + TK::HP * 1024;
#pragma unroll
    for (int k = 0; k < TK::WPW; ++k) {
        const int j = wave + TK::WM * k;
        if (j < s.wpc && !(abl & 8)) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, ISR_LDS_PTR(wd + j * 1024), 16, lane * 16,
                                                     wo + (pair ? j >> 1 : j) * 1024, 0, 0);
            ++n;
        }
    }
    if (with_bias && wave == 0) {
        char* bd = smem + TK::BIAS_OFF + bslot * 256;
        if (pair) {  // couts [0, 32) = the first layer's bias, [32, 64) = the second's
            if (lane < 32) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_n(s.b, 128u), ISR_LDS_PTR(bd), 4, lane * 4, 0, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_n((const float*)(uintptr_t)s.pb->b, 128u), ISR_LDS_PTR(bd + 128), 4, lane * 4, 0, 0, 0);
            }
            ++n;
        } else if (lane < (s.wpc == tk::WPG ? 32 : 64)) {  // cout floats only
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_n(s.b, s.wpc == tk::WPG ? 128u : 256u), ISR_LDS_PTR(bd), 4,
                                                     lane * 4, 0, 0, 0);
        }
        ++n;
    }
    return n;
}

__device__ __forceinline__ uint32_t stage_chunk(const TrunkCtx& c, const Src& s, int chunk, int slot, bool with_bias,
                                                int bslot, bool halo = true) {
#ifdef ISR_TUNING
    // tuning-build check of the ring protocol: the chunk lies inside the layer (chunk < nch: its
    // weights inside the packed table) and the slot inside the ring.  A violation gives the launch
    // up (the host raises) and issues nothing, instead of a DMA to a wrong place.
    if (chunk < 0 || (uint32_t)(chunk * (s.pb ? tk::WPG : s.wpc) * 1024) >= s.wbytes || slot < 0 || slot >= TK::NST ||
        bslot < 0 || bslot > 3) {
        if (threadIdx.x == 0) {
            __hip_atomic_store(c.state + 1, c.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(c.state + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return 0;
    }
#endif
    return stage_pieces(c.hoff, c.pstride, c.abl, s, chunk, slot, with_bias, bslot, halo);
}

// Kept tiles: the 9 weight pieces of chunk `chunk` of the 32-cout pack of `rec` (the second layer of
// a growth pair) into the weight area of ring slot `slot`, where a 32-cout chunk body reads them; the
// slot's halo image is not touched.  Returns the instructions this wave issued, as stage_pieces.
__device__ __forceinline__ uint32_t stage_keep_weights(const TrunkCtx& c, const_rec& rec, int chunk, int slot) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const uint32_t wbytes = (uint32_t)(rec_nch(rec) * tk::WPG * 1024), wo = (uint32_t)(chunk * tk::WPG * 1024);
#ifdef ISR_TUNING
    // tuning-build check, as in stage_chunk: the chunk's weights lie inside the packed table
    if (chunk < 0 || wo >= wbytes || slot < 0 || slot >= TK::NST) {
        if (threadIdx.x == 0) {
            __hip_atomic_store(c.state + 1, c.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(c.state + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return 0;
    }
#endif
    char* wd = smem + slot * TK::SLOT + TK::HP * 1024;
    const auto rw = rsrc_n((const char*)(uintptr_t)rec.w, wbytes);
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < (tk::WPG + TK::WM - 1) / TK::WM; ++k) {
        const int j = wave + TK::WM * k;
        if (j < tk::WPG && !(c.abl & 8)) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, ISR_LDS_PTR(wd + j * 1024), 16, lane * 16, wo + j * 1024, 0, 0);
            ++n;
        }
    }
    return n;
}

// The tile that follows the current one in this workgroup's stream.
struct Next {
    bool exists;
    int L, t;
    Src src;
    int first_new;   // its first chunk its previous layer wrote (NEED_NONE on layer 0)
    int nch;
    bool self_dep;   // its neighbourhood contains the tile being computed now
};

// Per wave, carried from item to item (all wave-uniform).  Items are the K-chunks of the
// stream in order; `issued` counts this wave's vector-memory instructions, and m[0..] holds
// `issued` right after the DMA of the current item and of the items staged after it, so the
// top of an item waits for exactly its own DMA (wait_vm(issued - m[0])) and leaves the later
// items, stores and loads in flight.
struct Stream {
    int item;             // global index of the item being computed
    int staged;           // global index of the last item whose DMA was issued
    int tseq;             // tiles started (bias slot = tseq & 3)
    uint32_t issued;
    uint32_t m0, m1, m2, m3;  // FIFO: m0 = current item (named scalars: an array would be indexed
                              // at run time and live in scratch, whose ops count in vmcnt)
    int pend_t;           // tile whose progress word waits for its stores (-1: none)
    unsigned pend_v;
    uint32_t pend_mark;   // `issued` right after those stores
    bool dep_next;        // the next tile's neighbourhood has been verified
    bool kept_next;       // kept tiles: the previous item left this item's chunks 0 and 1 in LDS but for
                          // their ring (a final conv followed by a growth pair on the same tile)
};

__device__ __forceinline__ void push_mark(Stream& st) {
    const int pos = st.staged - st.item;  // position of the item just staged
    const uint32_t v = st.issued;
    st.m0 = pos == 0 ? v : st.m0;
    st.m1 = pos == 1 ? v : st.m1;
    st.m2 = pos == 2 ? v : st.m2;
    st.m3 = pos >= 3 ? v : st.m3;
}

__device__ __forceinline__ void pop_mark(Stream& st) {
    st.m0 = st.m1;
    st.m1 = st.m2;
    st.m2 = st.m3;
}

// Publish the pending tile's progress word now (every wave drains all its vector memory, then a
// workgroup barrier): required before any blocking wait, so that no workgroup ever spins on a
// word this workgroup holds back.  Wave-uniform call sites only (it contains a barrier).
__device__ __forceinline__ void force_publish(const TrunkCtx& c, Stream& st) {
    if (st.pend_t < 0) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    raw_barrier();
    if (threadIdx.x == 0)
        __hip_atomic_store(c.state + 4 + st.pend_t, st.pend_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    st.pend_t = -1;
}

// The tile after (L, t) in workgroup b's stream of a G-workgroup grid: the next tile of the same
// layer, else the workgroup's first tile of the next layer; false at the end of the stream.  A growth
// pair is one item of `step` = 2 layers: the same pair at t + G, else layer L + 2.
__device__ __forceinline__ bool next_item(int L, int step, int t, int b, int G, int ntiles, int nl, int& nL, int& nt) {
    nL = L;
    nt = t;
    if (t + G < ntiles) {
        nt = t + G;
        return true;
    }
    if (L + step < nl) {
        nL = L + step;
        nt = b;
        return true;
    }
    return false;
}

// Does tile t2's 3x3 neighbourhood contain tile t?
__device__ __forceinline__ bool tiles_adjacent(const TrunkCtx& c, int t, int t2) {
    const int bx = t % c.nbx, tq = t / c.nbx, by = tq % c.nby, im = tq / c.nby;
    const int bx2 = t2 % c.nbx, nq = t2 / c.nbx, by2 = nq % c.nby, im2 = nq / c.nby;
    return im == im2 && abs(bx - bx2) <= 1 && abs(by - by2) <= 1;
}

// The forward layers' tiles run the chunk stream specialised by role; the masked kind-2 layers (the
// backward chain's gather convs) keep the general chunk, CR_GENERAL.
enum : int {
    CR_GENERAL,  // every test at run time
    CR_FIRST,    // chunk 0: bias, counted vmcnt wait, staged at its own top when the previous tile could not
    CR_SECOND,   // chunk 1: the previous tile's publish can still be pending; run-time neighbourhood test
    CR_STEADY,   // refill = this tile's next chunk, no test at all
    CR_DEP,      // a steady chunk whose refill may be the first to stage what the previous layer wrote
    CR_LOOP,     // CR_DEP or, for the tile's last chunk, CR_LAST: chosen at run time
    CR_LAST      // refill = chunk 0 of the next item (layer kind, self-dependency, bias slot at run time)
};

// One (layer, tile).  With the chunk roles (forward layers) a steady chunk carries no
// run-time generality:
//  * its wait is the immediate vmcnt(0): its DMA was issued inside the previous chunk and the wave
//    has issued no vector-memory instruction since (only a tile's chunk 0 has the previous tile's
//    epilogue stores / r2 loads behind its DMA, and keeps a counted wait);
//  * on the 32-cout layers the ring slot is a template argument (the steady run is unrolled by two,
//    one chunk peeled when it starts on slot 1 or its count is odd), so every LDS offset is a
//    constant (the 64-cout layers: see FULL below);
//  * the refill is this tile's next chunk, issued straight-line: the weight-piece count comes from
//    NF, the halo plane base advances by one add-with-carry per chunk (no 64-bit multiply), the
//    mark of the staged item is just `issued`;
//  * the pending publish is tested at chunks 0 and 1 only (chunk 1's DMA is younger than the
//    previous tile's stores, so its top publishes whatever chunk 0's could not; every forced path
//    publishes);
//  * the neighbourhood wait runs at most once per tile, at the chunk whose refill first stages what
//    the previous layer wrote: the steady run is split there.
// The last chunk stages the next item's chunk 0, and only there is that item's source computed.
// Both forms keep the same stream state and hand-off protocol, so their tiles follow each other in
// one stream, and the same MFMA, fold and epilogue order: the outputs are bit-identical.  The prep
// kernel guarantees nch >= 4.
//
// Growth pairs (PH; the prep kernel marks them): layers L and L + 1 of an RDB read the same chunks
// 0..nch(L)-1, and L + 1 then two more, the output of L.  One pair item per tile stages the shared
// chunks once:
//  * PH 1 (NF = 2, L = the first layer): the shared chunks with the 64-cout chunk bodies, fragment 0
//    = layer L, fragment 1 = layer L + 1 (weight pieces interleaved from the two 32-cout packs, the
//    two biases in one bias slot, no fold); its last chunk stages no halo; the growth epilogue on
//    fragment 0 alone, pending publish L + 1; fragment 1's accumulators leave in `pacc`;
//  * PH 2 (NF = 1, L = the second layer): its last two chunks on `pacc`.  The first starts at its
//    own top (drain the stores, publish, wait for the neighbourhood's layer L - 1); the second
//    stages the next item's chunk 0 as any last chunk does.  Growth epilogue, publish L + 1.
//  * What phase 2 reads is, but for a ring of 100 halo pixels, what this workgroup has just computed
//    (trunk_keep.h).  Kept tiles (c.keep, the switch ISR_TRUNK_KEEP, default on): phase 1's last
//    chunk also stages the weights of phase 2's first chunk into the other slot; phase 1's epilogue
//    starts with a barrier, stages the weights of phase 2's second chunk into the last chunk's slot
//    and writes each packed output register to LDS beside its global store (plane 0 = the interior
//    of phase 2's first chunk, plane 1 = of its second); phase 2, after the neighbourhood wait,
//    loads only the ring of both chunks (2 loads, 2 LDS writes per thread), waits once, and runs
//    the two chunks back to back.  The bits in LDS are those the read-back delivered.  With the
//    switch off phase 1's last chunk stages nothing and phase 2's first chunk is staged whole at
//    its own top (20 halo pieces, 9 weight pieces), its second inside the first's refill.
//    The same holds where a final conv is followed by a growth pair on the same tile (a workgroup
//    that owns one tile, at every RDB boundary): the pair's chunks 0 and 1 are planes 0 and 1 of the
//    final conv's fragment 0 and are kept in the same way (`keep_nx` below, `st.kept_next`); its
//    chunks 2 and 3 are staged from HBM as ever.
// Each accumulator receives the MFMAs of its per-layer tile in the same order (chunk ascending, then
// dx, dy, row, the same for NF 1 and 2), so the bits are those of the unpaired stream.
template <int NF, bool MASKED = false, bool H = false, int PH = 0>
__device__ __forceinline__ void run_tile(const TrunkCtx& c, Stream& st, const_rec* recs, int L, int t,
                                         int nxL, int nxt, bool nx_exists, f32x16* pacc = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = TK::R, NST = TK::NST, CT = 32 * NF, TN = 3, NA = R + 2;
    constexpr bool ROLES = !MASKED;
    static_assert(PH == 0 || (!MASKED && NF == (PH == 1 ? 2 : 1)), "pair phases: 64-cout bodies, then 32-cout");
    // The 64-cout layers (128 accumulator + 96 fragment VGPRs) keep one chunk body per fold position
    // plus one loop body (CR_LOOP: run-time slot, run-time boundary / last test): with alternative
    // chunk bodies in the arms of a branch, or the steady run split into several loops, hipcc moves
    // the accumulators between register ranges at the joins and spills 700-1,000 VGPRs to scratch
    // (DESIGN.md section 5).  The 32-cout layers take the full form: compile-time slots, split run.
    constexpr bool FULL = ROLES && NF == 1;
    constexpr int WPC = NF == 2 ? tk::WPF : tk::WPG;  // weight pieces per chunk of a forward layer
    constexpr int WSTEP = PH == 1 ? tk::WPG : WPC;    // pieces per chunk in one weight pack
    const_rec& rec = recs[L];
    const int wave = wave_id(), lane = threadIdx.x & 63, l31 = lane & 31, hh = lane >> 5;
    const int bx = t % c.nbx, tmp = t / c.nbx, by = tmp % c.nby, img = tmp / c.nby;
    const int x0 = bx * tk::TW, y0 = by * TK::TH;
    const int nch = rec_nch(rec);
    const int first_new = rec_first_new(rec);  // NEED_NONE on layer 0
    const unsigned need = c.gen * 1024u + (unsigned)L;  // the neighbourhood is done with layer L-1
    const bool fold = NF == 2 && PH == 0 && rec_fold(rec);
    const bool has_r2 = NF == 2 && PH == 0 && rec.r2 != 0;
    constexpr bool masked = NF == 1 && MASKED;  // kind 2 (gather conv): LeakyReLU' mask from rec.r2
    const Src me = src_of(c, rec, t);
    // general form: the next item's source up front (the roles compute it in the last chunk)
    Next nx;
    if constexpr (!ROLES) {
        const_rec& nrec = recs[nxL];
        nx.exists = nx_exists;
        nx.L = nxL;
        nx.t = nxt;
        nx.src = src_of(c, nrec, nxt);
        nx.first_new = rec_first_new(nrec);
        nx.nch = rec_nch(nrec);
        nx.self_dep = tiles_adjacent(c, t, nxt);
    }
    // roles: the plane of the next chunk to stage (advanced by pstride per chunk) and that chunk's
    // offset in the weight table
    const int ch0 = PH == 2 ? nch - 2 : 0;  // the tile's first chunk
    // the pack this wave stages from (pair phase 1: odd waves stage the second layer's pieces)
    const char* w_own = me.w;
    uint32_t wext_own = me.wbytes;
    if constexpr (PH == 1) {
        if (wave & 1) {
            w_own = (const char*)(uintptr_t)recs[L + 1].w;
            wext_own += 2 * tk::WPG * 1024;
        }
    }
    const char* xn = me.x + (size_t)ch0 * c.pstride;
    uint32_t wo = (uint32_t)(ch0 * WSTEP * 1024);
    bool dep_ok = PH != 2 && (first_new == tk::NEED_NONE || st.dep_next);
    st.dep_next = false;
    const int bslot = st.tseq & 3;
    const int first_item = st.item;  // this tile's chunk 0
    const bool kept = PH != 0 && c.keep != 0;  // growth pairs: the tile stays in LDS across the hand-off
    // Same-tile layer boundary (c.keep & 2): this is a final conv, and the next item is a growth pair
    // on the same tile whose chunks 0..3 are this layer's output planes (ntiles <= workgroups: once
    // per RDB).  That item would be staged at its own top; its chunks 0 and 1 = fragment 0's two planes
    // are kept as phase 2's are: weights (and bias) of chunk 0 in the last chunk, of chunk 1 in the
    // epilogue, the interiors from the epilogue's registers.  Chunks 2 and 3 stage as ever.
    bool keep_nx = false;
    if constexpr (ROLES && NF == 2 && PH == 0) {
        const int fm = rec_form(rec);
        // first_new == 0 says only that the pair's chunk 0 overlaps this layer's 64 output channels (and
        // that it reads the buffer this layer writes): its first plane must BE output plane 0, or the
        // pair's chunks 0 and 1 are other planes than fragment 0's (a pair reading from y.coff + 16, + 32
        // or + 48 is a valid table: it is staged from HBM)
        keep_nx = (c.keep & 2) && nx_exists && nxt == t && nxL == L + 1 && (fm == EPI_FINAL || fm == EPI_FINAL_R2) &&
                  rec_first_new(recs[nxL]) == 0 && rec_pair(recs[nxL]) == 1 && rec_xp(recs[nxL]) == rec_yp(rec);
    }
    bool both_staged = false;  // this tile's first chunk found its second staged with it (kept tiles)
    trunk_stamp(L, t, c.ntiles, 0);

    // per-lane LDS read addresses (slot 0): weights A[n][k] (n = cout), halo rows of this wave
    const uint32_t a_w = (uint32_t)(TK::HP * 1024 + (2 * l31 + (hh ^ ((l31 >> 3) & 1))) * 16);
    uint32_t a_h[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
        a_h[dx] = (uint32_t)((wave * R * tk::HC + l31 + dx) * 32 + 16 * (hh ^ (((l31 + dx) >> 3) & 1)));

    // neighbourhood wait (blocking), preceded by the pending publish
    auto wait_deps = [&](int tt, unsigned nd) {
        force_publish(c, st);
        trunk_stamp(L, t, c.ntiles, 4);
        if (!(c.abl & 16)) dep_wait(c.state, nb_of(tt, c.nbx, c.nby), nd, c.gen);
        if (c.acquire) acquire_fence();
        trunk_stamp(L, t, c.ntiles, 5);
    };

    // roles: this tile's next chunk into ring slot S — the wave's share of the halo and weight
    // pieces, every piece count a constant except the ragged last round's
    auto stage_own = [&](const int sl) {
        char* dst = smem + sl * TK::SLOT;
        uint32_t n = 0;
        const auto rx = rsrc_n(xn, c.pstride);
        if (!(c.abl & 1)) {
#pragma unroll
            for (int k = 0; k < TK::HPW; ++k) {
                const int j = wave + TK::WM * k;
                if (TK::WM * k + TK::WM <= TK::HP || j < TK::HP) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, ISR_LDS_PTR(dst + j * 1024), 16, c.hoff[k], me.h0, 0,
                                                             TK::HALO_AUX);
                    ++n;
                }
            }
        }
        if (!(c.abl & 8)) {
            // pair phase 1: LDS piece j = tap j / 2 of the first (j even) or second (j odd) layer's
            // pack; j has the wave's parity, so a wave reads one pack
            const auto rw = rsrc_n(w_own, wext_own);
#pragma unroll
            for (int k = 0; k < (WPC + TK::WM - 1) / TK::WM; ++k) {
                const int j = wave + TK::WM * k;
                if (TK::WM * k + TK::WM <= WPC || j < WPC) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, ISR_LDS_PTR(dst + (TK::HP + j) * 1024), 16, lane * 16,
                                                             wo + (PH == 1 ? j >> 1 : j) * 1024, 0, 0);
                    ++n;
                }
            }
        }
        xn += c.pstride;
        wo += WSTEP * 1024;
        return n;
    };

    f32x16 acc[R][NF];
    if constexpr (PH == 2) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][0] = pacc[r];  // phase 1 left them: bias and the shared chunks
    }

    // one K-chunk; FC = the chunk index (0..3) when the residual fold adds its MFMAs to it, else -1
    // (peeled so that the fold's target accumulator is compile-time: a run-time choice made hipcc
    // MFMA into a temporary and copy 16 VGPRs back)
    const uint32_t idv = rec_idv(rec);
    // S = the ring slot (roles; -1: st.item % NST at run time), ROLE = the chunk's role
    auto do_chunk = [&](const int ch, auto fc_tag, auto s_tag, auto role_tag) {
        constexpr int FC = decltype(fc_tag)::value, S = decltype(s_tag)::value, ROLE = decltype(role_tag)::value;
        static_assert((ROLE == CR_GENERAL) == MASKED, "the masked layers run the general chunk");
            const int slot = S >= 0 ? S : st.item % NST;
            const bool stamp_tile = t == (int)blockIdx.x;
            item_stamp(L, stamp_tile, ch, 0, TK::WM);
            // ---- top of item: this item's DMA has landed for every wave ----
            bool ring_ok = true;  // (tuning builds: the immediate wait's premise holds)
            if constexpr (ROLE == CR_FIRST) {
                if (st.staged < st.item) {
                    // not staged (the previous tile's outputs lie in this tile's neighbourhood): drain,
                    // publish, wait, stage
                    // (pair phase 2 always comes here: phase 1 just wrote this chunk and staged no halo)
                    force_publish(c, st);
                    if ((PH == 2 || first_new == 0) && !dep_ok) {
                        wait_deps(t, need);
                        dep_ok = true;
                    }
                    bool ring_only = PH == 2 && kept;
                    if constexpr (PH == 1) {
                        ring_only = st.kept_next;
                        st.kept_next = false;
                    }
                    if (ring_only) {
                        both_staged = true;
                        // kept tile: the interior of both chunks and their weights are in LDS (phase
                        // 1's epilogue); only the ring, which other workgroups wrote, is fetched: one
                        // 16-byte sc1 load per chunk by threads 0..199, then the same bits to LDS.
                        // Both chunks are staged by this: the first chunk issues no refill
                        typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
                        asm volatile("" ::: "memory");  // the loads stay behind the neighbourhood wait
                        if (threadIdx.x < keep::RING_UNITS && !(c.abl & 1)) {
                            const char* xa = me.x + (size_t)ch * c.pstride;
                            const u32x4 ra = __builtin_amdgcn_raw_buffer_load_b128(rsrc_n(xa, c.pstride), c.ring_src, me.h0, TK::HALO_AUX);
                            const u32x4 rb = __builtin_amdgcn_raw_buffer_load_b128(rsrc_n(xa + c.pstride, c.pstride), c.ring_src, me.h0, TK::HALO_AUX);
                            *reinterpret_cast<u32x4*>(smem + slot * TK::SLOT + c.ring_lds) = ra;
                            *reinterpret_cast<u32x4*>(smem + (slot ^ 1) * TK::SLOT + c.ring_lds) = rb;
                        }
                        // The loads are compiler-visible: hipcc places their vmcnt wait before the two
                        // LDS stores, so the counted wait below finds nothing of this chunk in flight;
                        // the top barrier's lgkmcnt(0) (raw_barrier) is what completes the LDS stores
                        // before any wave reads the ring.
                        st.issued += 2;
                        st.staged = st.item + 1;
                        st.m0 = st.m1 = st.issued;
                    } else {
                        st.issued += stage_chunk(c, me, ch, slot, PH != 2, bslot);
                        st.staged = st.item;
                        st.m0 = st.issued;
                    }
                }
                xn += c.pstride;  // the first chunk is staged: the next chunk to stage is the second
                wo += WSTEP * 1024;
                wait_vm_coarse(st.issued - st.m0);
            } else if constexpr (ROLE != CR_GENERAL) {
#ifdef ISR_TUNING
                // tuning-build check of the immediate wait: nothing was issued since this chunk's DMA.
                // A violation gives the launch up (the host raises) and the chunk issues no refill.
                if (st.issued != st.m0) {
                    ring_ok = false;
                    if (threadIdx.x == 0) {
                        __hip_atomic_store(c.state + 1, c.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_add(c.state + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
#endif
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
            if (st.staged < st.item) {
                // not staged (the next tile needed this tile's own outputs): drain, publish, wait, stage
                force_publish(c, st);
                if (ch >= first_new && !dep_ok) {
                    wait_deps(t, need);
                    dep_ok = true;
                }
                st.issued += stage_chunk(c, me, ch, slot, ch == 0, bslot);
                st.staged = st.item;
                push_mark(st);
            }
            wait_vm(st.issued - st.m0);
            }
            item_stamp(L, stamp_tile, ch, 1, TK::WM);
            raw_barrier();
            item_stamp(L, stamp_tile, ch, 2, TK::WM);
            if constexpr (ROLE == CR_GENERAL || ROLE == CR_FIRST || ROLE == CR_SECOND) {
            if (st.pend_t >= 0 && (int)(st.m0 - st.pend_mark) >= 0) {  // its stores are older than this DMA
                if (threadIdx.x == 0)
                    __hip_atomic_store(c.state + 4 + st.pend_t, st.pend_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                st.pend_t = -1;
            }
            }
            if (PH == 2 && ROLE == CR_FIRST) trunk_stamp(L, t, c.ntiles, 1);  // the hand-off is over
            if (PH != 2 && (ROLE == CR_FIRST || (ROLE == CR_GENERAL && ch == 0))) {
                trunk_stamp(L, t, c.ntiles, 1);
                // bias → accumulators (register g of lane l: cout (g&3) + 8(g>>2) + 4hh of fragment f)
                const float* bs = reinterpret_cast<const float*>(smem + TK::BIAS_OFF + bslot * 256);
    #pragma unroll
                for (int f = 0; f < NF; ++f) {
                    f32x16 b0;
    #pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(bs + f * 32 + 8 * j + 4 * hh);
    #pragma unroll
                        for (int e = 0; e < 4; ++e) b0[4 * j + e] = q[e];
                    }
    #pragma unroll
                    for (int r = 0; r < R; ++r) acc[r][f] = b0;
                }
            }
            const char* sb = smem + slot * TK::SLOT;
            // two fragment sets: the next step's fragments are read during this step's MFMAs
            bf16x8 fb[2][TN][NF], fa[2][NA];
            auto read_one = [&](int dx, int idx, int set) {
                if (idx < TN * NF) {
                    const int dyi = idx / NF, f = idx % NF;
                    fb[set][dyi][f] = lds_read16(sb + a_w + ((dyi * 3 + dx) * CT * 2 + f * 64) * 16);
                } else {
                    const int ia = idx - TN * NF;
                    fa[set][ia] = lds_read16(sb + a_h[dx] + ia * tk::HC * 32);
                }
            };
            auto read_fb = [&](int dx, int dyi, int set) {
    #pragma unroll
                for (int f = 0; f < NF; ++f) read_one(dx, dyi * NF + f, set);
            };
            // step 0's fragments in order of first use (kernel-row-major MFMA order below)
            auto read_step0 = [&]() {
                read_fb(0, 0, 0);
    #pragma unroll
                for (int ia = 0; ia < R; ++ia) read_one(0, TN * NF + ia, 0);
                read_fb(0, 1, 0);
                read_one(0, TN * NF + R, 0);
                read_fb(0, 2, 0);
                read_one(0, TN * NF + R + 1, 0);
                __builtin_amdgcn_sched_barrier(0);
            };
            read_step0();

            // ---- refill: stage the stream one item ahead (this tile's next chunk, else the next
            // tile's chunk 0), in one block after step 0's reads ----
            const bool last = ROLE == CR_LAST || (ROLE == CR_LOOP && ch == nch - 1);
            if constexpr ((ROLE == CR_LAST || ROLE == CR_LOOP) && PH != 1) {
                // the next item's chunk 0 (with its bias), unless it needs this tile's own outputs
                // (pair phase 1: the next item is its own phase 2, which does)
                if (last && nx_exists && ring_ok) {
                    const_rec& nrec = recs[nxL];
                    bool go = true;
                    if (nxL > 0 && rec_first_new(nrec) == 0) {
                        if (tiles_adjacent(c, t, nxt)) {
                            go = false;  // staged at its own top
                        } else {
                            wait_deps(nxt, c.gen * 1024u + (unsigned)nxL);
                            st.dep_next = true;
                        }
                    }
                    if (go) {
                        st.issued += stage_chunk(c, src_of(c, nrec, nxt), 0, slot ^ 1, true, (bslot + 1) & 3);
                        ++st.staged;
                        st.m1 = st.issued;
                    } else if (keep_nx) {
                        // kept across the layer boundary: the next item's chunk-0 weights and its bias
                        // into the other slot; not counted as staged (the item still starts at its own top)
                        st.issued += stage_chunk(c, src_of(c, nrec, nxt), 0, slot ^ 1, true, (bslot + 1) & 3, false);
                    }
                }
            }
            if constexpr (PH == 1 && ROLE == CR_LOOP) {
                // kept tile: the weights of phase 2's first chunk (chunk nch of the second layer's
                // pack) into the other slot's weight area, idle since this chunk's top barrier; the
                // halo image of that slot is filled by the epilogue
                if (last && kept && ring_ok) st.issued += stage_keep_weights(c, recs[L + 1], nch, slot ^ 1);
            }
            if constexpr (ROLE != CR_GENERAL && ROLE != CR_LAST) {
                if constexpr (ROLE != CR_STEADY) {
                    if (!last && ch + 1 >= first_new && !dep_ok) {
                        wait_deps(t, need);
                        dep_ok = true;
                    }
                }
                if (ROLE == CR_FIRST && both_staged) {  // (kept tile: both chunks are in LDS)
                    xn += c.pstride;
                    wo += WSTEP * 1024;
                } else if (!last && ring_ok) {
                    st.issued += stage_own(slot ^ 1);
                    ++st.staged;
                    st.m1 = st.issued;
                }
            }
            if constexpr (ROLE == CR_GENERAL)
            while (st.staged < st.item + NST - 1) {
                const int off = st.staged + 1 - first_item;  // chunk offset from this tile's chunk 0
                const int nslot = (st.staged + 1) % NST;
                if (off < nch) {
                    if (off >= first_new && !dep_ok) {
                        wait_deps(t, need);
                        dep_ok = true;
                    }
                    st.issued += stage_chunk(c, me, off, nslot, false, 0);
                } else {
                    const int nc = off - nch;
                    if (!nx.exists || nc >= nx.nch) break;
                    if (nx.L > 0 && nc >= nx.first_new && !st.dep_next) {
                        if (nx.self_dep) break;  // needs this tile's outputs: staged at its own top
                        wait_deps(nx.t, c.gen * 1024u + (unsigned)nx.L);
                        st.dep_next = true;
                    }
                    st.issued += stage_chunk(c, nx.src, nc, nslot, nc == 0, (bslot + 1) & 3);
                }
                ++st.staged;
                push_mark(st);
            }
            __builtin_amdgcn_sched_barrier(0);
            item_stamp(L, stamp_tile, ch, 3, TK::WM);
            // the wave at priority 1 around the chunk's MFMA stream (s_setprio), so the co-resident
            // workgroup's refill / epilogue issue yields to it
            __builtin_amdgcn_s_setprio(1);

            // ---- MFMAs: 3 steps (dx), each in kernel-row-major order (dy, then output row r):
            // every accumulator still sees dy 0, 1, 2 in that order (conv3x3.hip's input-row-major
            // loop gives each accumulator the same sequence, so the bits agree).  The next step's
            // fragment of kernel row dy is read right after that row's last MFMA here, and its
            // input row ia right after the current one's last use. ----
    #pragma unroll
            for (int stp = 0; stp < 3; ++stp) {
                const int cur = stp & 1;
    #pragma unroll
                for (int dyi = 0; dyi < TN; ++dyi) {
    #pragma unroll
                    for (int r = 0; r < R; ++r) {
    #pragma unroll
                        for (int f = 0; f < NF; ++f) acc[r][f] = mfma32t<H>(fb[cur][dyi][f], fa[cur][r + dyi], acc[r][f]);
                        if constexpr (NF == 2 && FC >= 0) {
                            // residual fold: + x/s1 on the centre pixels of row r (dx = 1, dy = 1),
                            // between the row's dy = 1 and dy = 2 contributions (chunk FC, compile-time)
                            if (dyi == 1 && stp == 1) {
                                const bf16x8 a = fold_a_bits(idv, FC & 1);
                                acc[r][FC >> 1] = mfma32t<H>(a, fa[cur][r + 1], acc[r][FC >> 1]);
                            }
                        }
                        // input row ia = r + dyi is last used here when dyi == min(2, ia)
                        if (stp + 1 < 3 && (dyi == 2 || r == 0)) read_one(stp + 1, TN * NF + r + dyi, cur ^ 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (stp + 1 < 3) {
                        read_fb(stp + 1, dyi, cur ^ 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            __builtin_amdgcn_s_setprio(0);
            item_stamp(L, stamp_tile, ch, 4, TK::WM);
            pop_mark(st);  // the FIFO head moves to the next item (marks are positions from st.item)
            ++st.item;
    };
    if constexpr (ROLES) {
        // a chunk in the slot the stream has reached (a tile starts on either slot: counts may be odd)
        int ch = ch0;
        auto in_slot = [&](auto fc_tag, auto role_tag) {
            if constexpr (!FULL) do_chunk(ch, fc_tag, TIC<-1>{}, role_tag);
            else if (st.item & 1) do_chunk(ch, fc_tag, TIC<1>{}, role_tag);
            else do_chunk(ch, fc_tag, TIC<0>{}, role_tag);
            ++ch;
        };
        if constexpr (PH == 2) {  // straight-line: the two chunks phase 1 wrote
            in_slot(TIC<-1>{}, TIC<CR_FIRST>{});
            in_slot(TIC<-1>{}, TIC<CR_LAST>{});
        }
        if constexpr (NF == 2 && PH == 0) {
            if (fold) {  // the residual fold's chunks 0-3, peeled
                in_slot(TIC<0>{}, TIC<CR_FIRST>{});
                in_slot(TIC<1>{}, TIC<CR_SECOND>{});
                in_slot(TIC<2>{}, TIC<CR_DEP>{});
                in_slot(TIC<3>{}, TIC<CR_LOOP>{});  // the last chunk of a 64-channel input
            }
        }
        if constexpr (PH != 2)
        if (ch == 0) {
            in_slot(TIC<-1>{}, TIC<CR_FIRST>{});
            in_slot(TIC<-1>{}, TIC<CR_SECOND>{});
        }
        if constexpr (PH != 2)
        if (ch < nch) {
            // steady chunks [ch, nch - 1), split at the chunk `wb` whose refill stages chunk first_new
            const int wb = first_new - 1;
            int stop = wb >= ch && wb < nch - 1 ? wb : nch - 1;
            if constexpr (!FULL) {
                for (; ch < nch; ++ch) do_chunk(ch, TIC<-1>{}, TIC<-1>{}, TIC<CR_LOOP>{});
            } else {
                for (;;) {
                    if (ch < stop && (st.item & 1)) {  // peel: the run starts on slot 1
                        do_chunk(ch, TIC<-1>{}, TIC<1>{}, TIC<CR_STEADY>{});
                        ++ch;
                    }
                    for (; ch + 1 < stop; ch += 2) {
                        do_chunk(ch, TIC<-1>{}, TIC<0>{}, TIC<CR_STEADY>{});
                        do_chunk(ch + 1, TIC<-1>{}, TIC<1>{}, TIC<CR_STEADY>{});
                    }
                    if (ch < stop) {  // peel: an odd count
                        do_chunk(ch, TIC<-1>{}, TIC<0>{}, TIC<CR_STEADY>{});
                        ++ch;
                    }
                    if (ch >= nch - 1) break;
                    in_slot(TIC<-1>{}, TIC<CR_DEP>{});
                    stop = nch - 1;
                }
                in_slot(TIC<-1>{}, TIC<CR_LAST>{});
            }
        }
    } else {
        for (int ch = 0; ch < nch; ++ch) do_chunk(ch, TIC<-1>{}, TIC<-1>{}, TIC<CR_GENERAL>{});
    }
    trunk_stamp(L, t, c.ntiles, 2);

    // the neighbourhood must be done with layer L-1 before this tile's outputs land (a layer
    // that reads nothing its predecessor wrote never waited above)
    if (!dep_ok && first_new != tk::NEED_NONE) wait_deps(t, need);

    // ---- epilogue: straight from the accumulators, write-through (sc1) stores ----
    // EF = the layer's epilogue form (trunk_common.h EPI_*, classified by the prep kernel), FT = the
    // tile lies wholly inside the image.  EPI_GENERAL decides slope, fold, r2, mask, s2 and `valid`
    // per value at run time; the other forms carry only their own arithmetic, convert with the packed
    // instruction, and zero a ragged tile's outside pixels on the packed dwords (0.f packs to 0).
    // Every form gives the general body's bits: the LeakyReLU stays the general body's compare and
    // select (a >= 0 ? a : a * slope; hipcc canonicalises the inputs of a float max with one more
    // v_max each, so max(a, a * slope) costs the same 2.5 instructions per value and would still have
    // to be argued for -0 and NaN); the fold layers have slope == 1; u * s2 + r2 is one fused
    // multiply-add in the general body (hipcc contracts it) and an explicit one here.
    // KP (pair phase 1 with kept tiles): the tile's two output planes are the halo interiors of phase
    // 2's two chunks.  One barrier (every wave has finished the last chunk's fragment reads), the
    // weights of phase 2's second chunk into the last chunk's slot, and beside each global store the
    // same packed register to LDS: plane 0 into the other slot's halo image (phase 2's first chunk),
    // plane 1 into the last chunk's.  The row is an immediate offset: no VALU per value.
    auto epilogue = [&](auto form_tag, auto full_tag, auto keep_tag) {
        constexpr int EF = decltype(form_tag)::value;
        constexpr bool GEN = EF == EPI_GENERAL, FT = decltype(full_tag)::value != 0;
        constexpr bool KP = decltype(keep_tag)::value != 0;
        static_assert(!KP || (PH == 1 && EF == EPI_GROWTH) || (PH == 0 && NF == 2 && (EF == EPI_FINAL || EF == EPI_FINAL_R2)),
                      "kept tiles: pair phase 1, or a final conv before a pair on the same tile");
        uint32_t kb[2] = {0, 0};
        if constexpr (KP) {
            const int cur = (st.item - 1) % NST;  // the last chunk's slot
            raw_barrier();
            if constexpr (PH == 1) {
                st.issued += stage_keep_weights(c, recs[L + 1], nch + 1, cur);
            } else {  // the next item's chunk 1: the 64-cout weight image of the pair, no bias
                st.issued += stage_chunk(c, src_of(c, recs[nxL], nxt), 1, cur, false, 0, false);
                st.kept_next = true;
            }
            kb[0] = c.kbase + (uint32_t)((cur ^ 1) * TK::SLOT);
            kb[1] = c.kbase + (uint32_t)(cur * TK::SLOT);
        }
        static_assert(GEN || (EF == EPI_GROWTH ? (NF == 1 || PH == 1) && !MASKED : NF == 2 && PH == 0),
                      "form and layer kind");
        const bool use_r2 = GEN ? (has_r2 || masked) : EF == EPI_FINAL_R2;
        // the body's marker in the assembly (tools/trunk_isa_mix.py) and the LeakyReLU's 0.0f as a
        // value of this body alone: compared with the literal, the 64 compares of a growth tile were
        // hoisted above the branch between the full and the ragged body, and their lane masks held
        // in 128 SGPRs, most of them spilled
        float zero = 0.f;
        if constexpr (EF == EPI_GROWTH) asm volatile("; trunk epilogue form %1 full %2" : "+s"(zero) : "n"(EF), "n"((int)FT));
        else if constexpr (!GEN) asm volatile("; trunk epilogue form %0 full %1" ::"n"(EF), "n"((int)FT));
        typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
        const int xx = x0 + l31;
        const float slope = rec.slope, s1 = rec.s1, s2 = rec.s2;
        const bool scale2 = s2 != 1.f;
        // one buffer resource per output plane (cout channels = NF * 2 planes of 16): couts
        // [32 f + 16 blk, + 16) live in plane yp + 2 f + blk of image img
        const char* ybase = (const char*)(uintptr_t)rec.y + (size_t)((uint32_t)img * c.cs16 + rec_yp(rec)) * c.pstride;
        // RRDB residual (every third RDB's final conv): row r + 1's values are loaded while row r
        // is finished, so at most two rows (32 VGPRs) are live — loading them all before the last
        // chunk's MFMAs (64 VGPRs beside the 128 accumulators and the fragments) spilled.
        // Compiler-visible loads: hipcc places the wait before their first use itself.
        bf16x8 q2[R][NF][2];
        const char* r2base = (const char*)(uintptr_t)rec.r2 + (size_t)((uint32_t)img * c.cs16 + rec_r2p(rec)) * c.pstride;
        auto load_r2 = [&](int r) {
            const uint32_t pix = (uint32_t)((y0 + wave * R + r + c.pad) * c.wp + xx + c.pad);
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    const auto rr = rsrc_n(r2base + (size_t)(2 * f + blk) * c.pstride, c.pstride);
                    q2[r][f][blk] = __builtin_bit_cast(
                        bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rr, pix * 32 + 16 * hh, 0, 16));
                }
            st.issued += NF * 2;
        };
        if (use_r2) load_r2(0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (use_r2 && r + 1 < R) load_r2(r + 1);
            const int yy = y0 + wave * R + r;
            const bool valid = yy < c.h && xx < c.w;
            const uint32_t pix = (uint32_t)((yy + c.pad) * c.wp + xx + c.pad);
#pragma unroll
            for (int f = 0; f < (PH == 1 ? 1 : NF); ++f) {  // pair phase 1: fragment 0 is the layer
                float v[16];
                if constexpr (GEN) {
#pragma unroll
                    for (int g = 0; g < 16; ++g) v[g] = acc[r][f][g];
                } else {
                    // what does not depend on the pixel (activation, s1, s2) on the accumulator
                    // pairs before the lane swap: packed multiplies into fresh registers, which the
                    // swap then changes in place (swapping first cost a copy per accumulator)
                    typedef __attribute__((ext_vector_type(2))) float f32x2;
                    const f32x16& a = acc[r][f];
#pragma unroll
                    for (int g = 0; g < 16; g += 2) {
                        f32x2 p = {a[g], a[g + 1]};
                        if constexpr (EF == EPI_GROWTH) {
                            p = p * slope;
                        } else {
                            p = p * s1;
                            if constexpr (EF == EPI_FINAL_S2) p = p * s2;
                        }
                        v[g] = p[0];
                        v[g + 1] = p[1];
                    }
                    if constexpr (EF == EPI_GROWTH) {
#pragma unroll
                        for (int g = 0; g < 16; ++g) v[g] = a[g] >= zero ? a[g] : v[g];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    swap_halves(v[k], v[4 + k]);
                    swap_halves(v[8 + k], v[12 + k]);
                }
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    float* u = v + 8 * blk;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if constexpr (!GEN) {
                            if constexpr (EF == EPI_FINAL_R2) u[e] = __builtin_fmaf(u[e], s2, elt<H>(q2[r][f][blk], e));
                        } else {
                        if (masked)
                            u[e] = elt<H>(q2[r][f][blk], e) > 0.f ? u[e] : u[e] * slope;
                        else
                            u[e] = u[e] >= 0.f ? u[e] : u[e] * slope;
                        if (fold) u[e] = u[e] * s1;
                        if (has_r2) {
                            u[e] = u[e] * s2 + elt<H>(q2[r][f][blk], e);
                        } else {
                            if (scale2) u[e] *= s2;
                        }
                        if (!valid) u[e] = 0.f;
                        }
                    }
                    const auto yr = rsrc_n(ybase + (size_t)(2 * f + blk) * c.pstride, c.pstride);
                    const uint32_t off = pix * 32 + 16 * hh;
                    bf16x8 tq;
                    if constexpr (GEN) {
                        tq = pack8<H>(u);
                    } else {
                        tq = pack8_pairs<H>(u);
                        if constexpr (!FT) {
                            u32x4 z = __builtin_bit_cast(u32x4, tq);
#pragma unroll
                            for (int d = 0; d < 4; ++d) z[d] = valid ? z[d] : 0u;
                            tq = __builtin_bit_cast(bf16x8, z);
                        }
                    }
                    if (!(c.abl & 4)) {
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, tq), yr, off, 0, TK::STORE_AUX);
                        ++st.issued;
                    }
                    if constexpr (KP) {
                        if (f == 0)  // (a final conv: fragment 1 = planes 2 and 3 are staged from HBM)
                            *reinterpret_cast<u32x4*>(smem + kb[blk] + r * keep::ROW_STEP) = __builtin_bit_cast(u32x4, tq);
                    }
                }
            }
        }
    };
    // one wave-uniform branch per tile into the body of the layer's form (the masked layers: general)
    auto epilogue_of = [&](auto form_tag, auto keep_tag) {
        if (y0 + TK::TH <= c.h && x0 + tk::TW <= c.w) epilogue(form_tag, TIC<1>{}, keep_tag);
        else epilogue(form_tag, TIC<0>{}, keep_tag);
    };
    const int form = ROLES ? rec_form(rec) : (int)EPI_GENERAL;
    if constexpr (PH == 1) {
        // the prep kernel pairs layers of the growth form only; one wave-uniform branch on the switch
        if (kept) epilogue_of(TIC<EPI_GROWTH>{}, TIC<1>{});
        else epilogue_of(TIC<EPI_GROWTH>{}, TIC<0>{});
    } else if constexpr (PH == 2) {
        epilogue_of(TIC<EPI_GROWTH>{}, TIC<0>{});
    } else if constexpr (ROLES && NF == 1) {
        if (form == EPI_GROWTH) epilogue_of(TIC<EPI_GROWTH>{}, TIC<0>{});
        else epilogue(TIC<EPI_GENERAL>{}, TIC<0>{}, TIC<0>{});
    } else if constexpr (ROLES) {
        if (keep_nx && form == EPI_FINAL) epilogue_of(TIC<EPI_FINAL>{}, TIC<1>{});
        else if (keep_nx) epilogue_of(TIC<EPI_FINAL_R2>{}, TIC<1>{});
        else if (form == EPI_FINAL) epilogue_of(TIC<EPI_FINAL>{}, TIC<0>{});
        else if (form == EPI_FINAL_R2) epilogue_of(TIC<EPI_FINAL_R2>{}, TIC<0>{});
        else if (form == EPI_FINAL_S2) epilogue_of(TIC<EPI_FINAL_S2>{}, TIC<0>{});
        else epilogue(TIC<EPI_GENERAL>{}, TIC<0>{}, TIC<0>{});
    } else {
        epilogue(TIC<EPI_GENERAL>{}, TIC<0>{}, TIC<0>{});
    }
    trunk_stamp(L, t, c.ntiles, 3);
    st.pend_t = t;
    st.pend_v = c.gen * 1024u + (unsigned)(L + 1);
    st.pend_mark = st.issued;
    if constexpr (PH == 1) {
        // one bias slot per pair item: phase 2 ends the tile
#pragma unroll
        for (int r = 0; r < R; ++r) pacc[r] = acc[r][1];
    } else {
        ++st.tseq;
    }
}

template <bool H>
__global__ __launch_bounds__(TK::NT, TK::WPS) void trunk_kernel(TrunkArgs a) {
    TrunkCtx c;
    c.state = a.state;
    c.acquire = a.acquire;
    c.gen = __hip_atomic_load(a.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const_geo& g = *(const_geo*)(uintptr_t)(a.state + a.rec_off - 16);
    const_rec* recs = (const_rec*)(uintptr_t)(a.state + a.rec_off);
    if (g.err != 0) {  // the prep kernel refused the layer table: give up loudly
        if (threadIdx.x == 0) {
            __hip_atomic_store(a.state + 1, c.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(a.state + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    c.hp = g.hp;
    c.wp = g.wp;
    c.cs16 = g.cs16;
    c.pad = g.pad;
    c.h = g.h;
    c.w = g.w;
    c.nbx = g.nbx;
    c.nby = g.nby;
    c.ntiles = g.ntiles;
    c.pstride = (uint32_t)(c.hp * c.wp * 32);
    c.abl = trunk_abl_load();
    {
        const int wave = wave_id(), lane = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < TK::HPW; ++k) c.hoff[k] = halo_piece_off<TK::HQ>(wave + TK::WM * k, lane, c.wp);
        static_assert(TK::R == keep::ROWS_PER_WAVE && keep::RING_UNITS <= TK::NT, "trunk_keep.h describes this build");
        c.kbase = keep_epi_lds_off(wave, 0, lane & 31, lane >> 5);
        const int ru = (int)threadIdx.x < keep::RING_UNITS ? (int)threadIdx.x : 0;
        c.ring_src = keep_ring_src_off(ru, c.wp);
        c.ring_lds = keep_ring_lds_off(ru);
    }
    c.keep = a.keep;
    const int G = gridDim.x, b = (int)blockIdx.x;
    Stream st;
    st.item = 0;
    st.staged = 0;
    st.tseq = 0;
    st.issued = 0;
    st.m0 = st.m1 = st.m2 = st.m3 = 0;
    st.pend_t = -1;
    st.pend_v = 0;
    st.pend_mark = 0;
    st.dep_next = false;
    st.kept_next = false;
    if (b < c.ntiles) {
        st.issued += stage_chunk(c, src_of(c, recs[0], b), 0, 0, true, 0);  // layer 0 reads the trunk input only
        st.m0 = st.issued;
        for (int L = 0, step; L < a.nl; L += step) {
            const_rec& rec = recs[L];
            // a growth pair (layers L, L + 1) is one item per tile, pair-major: both phases of a tile
            // before the workgroup's next tile
            const bool pair = rec_pair(rec) == 1 && L + 1 < a.nl;
            step = pair ? 2 : 1;
            for (int t = b; t < c.ntiles; t += G) {
                int nxL, nxt;
                const bool nx_exists = next_item(L, step, t, b, G, c.ntiles, a.nl, nxL, nxt);
                const int kind = rec_kind(rec);
                if (pair) {
                    f32x16 pacc[TK::R];
                    run_tile<2, false, H, 1>(c, st, recs, L, t, nxL, nxt, nx_exists, pacc);
                    run_tile<1, false, H, 2>(c, st, recs, L + 1, t, nxL, nxt, nx_exists, pacc);
                } else if (kind == 0) run_tile<1, false, H>(c, st, recs, L, t, nxL, nxt, nx_exists);
                else if (kind == 2) run_tile<1, true, H>(c, st, recs, L, t, nxL, nxt, nx_exists);  // the backward chain's gathers
                else run_tile<2, false, H>(c, st, recs, L, t, nxL, nxt, nx_exists);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && st.pend_t >= 0)
        __hip_atomic_store(c.state + 4 + st.pend_t, st.pend_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid: every workgroup must be resident at once (tiles wait on other workgroups' tiles), so
// the grid is min(tiles, resident workgroups) with residency from the occupancy API (capped at
// what the build is made for); ISR_ERR when that is below one workgroup per CU.
template <bool H>
static int trunk_launch_k(const isr_chain_desc* cd, hipStream_t s) {
    if (cd->ha % TK::TH || cd->wa % tk::TW || cd->nl < 1 || cd->nl > 1024) return DISPATCH_UNSUPPORTED;
    const int nbx = cd->wa / tk::TW, nby = cd->ha / TK::TH;
    const long long ntiles = (long long)cd->n * nbx * nby;
    if (ntiles <= 0 || ntiles > (1 << 24)) return DISPATCH_UNSUPPORTED;
    static thread_local int cached_dev = -1, cached_per_cu = 0, cached_cus = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    const void* kern = (const void*)trunk_kernel<H>;
    if (dev != cached_dev) {
        (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, TK::LDS);
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, TK::NT, TK::LDS) != hipSuccess) return -1;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return -1;
        cached_dev = dev;
        cached_per_cu = per_cu < TK::BPC ? per_cu : TK::BPC;
        cached_cus = cus;
    }
    int per_cu = cached_per_cu;
#ifdef ISR_TUNING
    if (g_trunk_per_cu > 0 && g_trunk_per_cu < per_cu) per_cu = g_trunk_per_cu;
#endif
    if (per_cu < 1) return DISPATCH_NO_OCCUPANCY;
    const long long slots = (long long)per_cu * cached_cus;
    const int grid = (int)(ntiles < slots ? ntiles : slots);
    const int rec_off = (int)trunk_rec_off((int)ntiles);
    // growth pairs: ISR_TRUNK_PAIRS = 0 none, 1 only pairs sharing 8 chunks or more, 2 all (the A/B
    // switch of DESIGN.md section 5, Growth pairs), read once
    static const int pair_mode = getenv("ISR_TRUNK_PAIRS") ? atoi(getenv("ISR_TRUNK_PAIRS")) : TRUNK_PAIRS_ALL;
    trunk_prep_launch(cd, TK::TH, grid, pair_mode < 0 ? 0 : (pair_mode > 2 ? 2 : pair_mode), s);
    TrunkArgs a;
    a.state = cd->state;
    a.rec_off = rec_off;
    a.nl = cd->nl;
    a.acquire = cd->acquire;
    // kept tiles: ISR_TRUNK_KEEP = 0 phase 2 of a growth pair stages its chunks whole, 1 (default) the
    // tile and its weights stay in LDS, across the phase-2 hand-off and across a final conv followed by
    // a pair on the same tile, 2 across the phase-2 hand-off only (the A/B switch of DESIGN.md section
    // 5, Kept tiles), read once
    static const int keep_mode = getenv("ISR_TRUNK_KEEP") ? atoi(getenv("ISR_TRUNK_KEEP")) : 1;
    a.keep = keep_mode <= 0 ? TRUNK_KEEP_OFF : (keep_mode == 2 ? TRUNK_KEEP_ON : TRUNK_KEEP_ON | TRUNK_KEEP_BOUNDARY);
    hipLaunchKernelGGL((trunk_kernel<H>), dim3(grid), dim3(TK::NT), TK::LDS, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int trunk_launch(const isr_chain_desc* cd, hipStream_t s) {
    return cd->f16 ? trunk_launch_k<true>(cd, s) : trunk_launch_k<false>(cd, s);
}

#ifdef ISR_TUNING
int trunk_knobs_set(const int* k) {
    g_trunk_per_cu = k[1];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trunk_knobs), k, 4 * sizeof(int)) == hipSuccess ? 0 : -1;
}
int trunk_stamps_set(void* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_trunk_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -1; }
int trunk_item_stamps_set(void* p) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_item_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#else
int trunk_knobs_set(const int*) { return DISPATCH_UNSUPPORTED; }
int trunk_stamps_set(void*) { return DISPATCH_UNSUPPORTED; }
int trunk_item_stamps_set(void*) { return DISPATCH_UNSUPPORTED; }
#endif

}  // namespace isr
