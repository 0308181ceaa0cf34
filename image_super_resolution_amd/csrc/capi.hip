// extern "C" entry points of libisr.so (declared in include/isr.h).
// Validation happens here so that a bad descriptor never reaches a kernel:
// every kernel indexes its tiles without bounds checks.
#include <stdarg.h>
#include <initializer_list>
#include <stdio.h>
#include <string.h>

#include "isr_common.h"
#include "dispatch.h"
#include "blur_taps.h"
#include "resample_tables.h"
#include "yuv_coeffs.h"

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

using isr::DISPATCH_NO_OCCUPANCY;
using isr::DISPATCH_UNSUPPORTED;
using isr::DISPATCH_WS_TOO_SMALL;

static int launched(int rc, const char* what) {
    if (rc != 0) {
        hipError_t e = hipGetLastError();
        return fail(ISR_ERR_LAUNCH, "%s: launch failed: %s", what, hipGetErrorString(e));
    }
    g_err[0] = 0;
    return ISR_OK;
}

// The answer of a dispatcher that sizes its own grid and refuses one past a launch's limit.
static int grid_launched(int rc, const char* what) {
    if (rc == DISPATCH_UNSUPPORTED) return fail(ISR_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups", what);
    return launched(rc, what);
}

static int workspace_ok(const char* what, const void* workspace) {
    return workspace ? ISR_OK : fail(ISR_ERR_BAD_DESC, "%s: null workspace", what);
}

// The answer of a dispatcher that takes a workspace; need() is the size query's figure for the same call.
template <class Need>
static int workspace_launched(int rc, const char* what, size_t ws_bytes, Need need) {
    if (rc == DISPATCH_WS_TOO_SMALL)
        return fail(ISR_ERR_BAD_DESC, "%s: workspace of %zu bytes is smaller than %zu", what, ws_bytes, (size_t)need());
    return launched(rc, what);
}

// The answer of a setter that only a tuning build carries.
static int tuning_set(int rc, const char* what) {
    if (rc == DISPATCH_UNSUPPORTED) return fail(ISR_ERR_UNSUPPORTED, "%s: library built without -DISR_TUNING", what);
    return rc == 0 ? ISR_OK : fail(ISR_ERR_LAUNCH, "%s: hipMemcpyToSymbol failed", what);
}

// The batch rule of the uint8 [n, 3, h, w] entry points: n in [1, 65535] (a grid extent), h and w at least
// min_side (1, or a kernel's window: then a smaller image is unsupported, not malformed) and, with fits31,
// n*3*h*w below 2^31 (such kernels index the batch with an int).
static int batch_ok(const char* what, int n, int h, int w, bool fits31, int min_side = 1) {
    if (n < 1 || n > 65535) return fail(ISR_ERR_BAD_DESC, "%s: bad batch n=%d (n in [1, 65535])", what, n);
    if (h < min_side || w < min_side)
        return fail(min_side > 1 ? ISR_ERR_UNSUPPORTED : ISR_ERR_BAD_DESC, "%s: image %dx%d smaller than %d x %d", what,
                    h, w, min_side, min_side);
    if (fits31 && (long long)n * 3 * h * w >= (1ll << 31))
        return fail(ISR_ERR_UNSUPPORTED, "%s: n*3*h*w = %lld does not fit 31 bits (n=%d, %dx%d)", what,
                    (long long)n * 3 * h * w, n, h, w);
    return ISR_OK;
}

// Every pointer of the list a multiple of `align` (a null one passes: presence is checked apart).
static bool aligned(uintptr_t align, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p % align) return false;
    return true;
}

// A view must hold rows [-halo, ha + halo) and cols [-halo, wa + halo) of the
// computed region plus `ch` channels from coff, in whole 16-channel blocks.
static int view_ok(const isr_view& v, int ha, int wa, int halo, int ch, const char* name) {
    if (!v.data) return fail(ISR_ERR_BAD_DESC, "%s: null data", name);
    if (v.pad < halo) return fail(ISR_ERR_BAD_DESC, "%s: pad %d < required halo %d", name, v.pad, halo);
    if (v.hp < ha + 2 * v.pad || v.wp < wa + 2 * v.pad)
        return fail(ISR_ERR_BAD_DESC, "%s: buffer %dx%d (pad %d) smaller than computed region %dx%d", name, v.hp, v.wp,
                    v.pad, ha, wa);
    if (v.coff < 0 || v.coff + ch > v.cs)
        return fail(ISR_ERR_BAD_DESC, "%s: channels [%d,%d) exceed stride %d", name, v.coff, v.coff + ch, v.cs);
    if ((v.cs % 16) || (v.coff % 16) || ((uintptr_t)v.data % 16))
        return fail(ISR_ERR_BAD_DESC, "%s: channel count/offset must be multiples of 16 (channel-blocked layout) "
                    "and data 16-byte aligned", name);
    return ISR_OK;
}

// The same for a view the descriptor may leave out (null data).
static int opt_view_ok(const isr_view& v, int ha, int wa, int halo, int ch, const char* name) {
    return v.data ? view_ok(v, ha, wa, halo, ch, name) : ISR_OK;
}

// The tile-grid rule of the MFMA kernels' descriptors (all carry n, h, w, ha, wa): a non-empty problem whose
// computed region is whole ISR_TILE_H x ISR_TILE_W tiles and covers the valid one.
template <class D>
static int tile_grid_ok(const char* what, const D* d) {
    if (d->n <= 0 || d->h <= 0 || d->w <= 0)
        return fail(ISR_ERR_BAD_DESC, "%s: empty problem n=%d h=%d w=%d", what, d->n, d->h, d->w);
    if (d->ha % ISR_TILE_H || d->wa % ISR_TILE_W || d->ha < d->h || d->wa < d->w)
        return fail(ISR_ERR_BAD_DESC, "%s: computed region %dx%d must cover %dx%d and be a multiple of %dx%d", what,
                    d->ha, d->wa, d->h, d->w, ISR_TILE_H, ISR_TILE_W);
    return ISR_OK;
}

// The blocked-grid rule of the elementwise kernels' descriptors (all carry n, h, w, ha, wa, c): a non-empty
// problem of c channels, a multiple of c_mul and at most c_max (0: no limit), whose computed region covers the
// valid one.
template <class D>
static int blocked_grid_ok(const char* what, const D* d, int c_mul, int c_max = 0) {
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->c % c_mul || (c_max && d->c > c_max)) {
        char rule[48] = "";
        if (c_max) snprintf(rule, sizeof(rule), " (c %% %d == 0, c <= %d)", c_mul, c_max);
        else if (c_mul > 1) snprintf(rule, sizeof(rule), " (c %% %d == 0)", c_mul);
        return fail(ISR_ERR_BAD_DESC, "%s: bad problem n=%d h=%d w=%d c=%d%s", what, d->n, d->h, d->w, d->c, rule);
    }
    if (d->ha < d->h || d->wa < d->w)
        return fail(ISR_ERR_BAD_DESC, "%s: computed region smaller than valid (%dx%d < %dx%d)", what, d->ha, d->wa,
                    d->h, d->w);
    return ISR_OK;
}

// The three 3x3 weight packs (bf16, fp16, Winograd fp16) take the same shapes.
static int pack3x3_ok(const char* what, const float* w, const void* packed, int cout, int cin) {
    if (!w || !packed) return fail(ISR_ERR_BAD_DESC, "%s: null pointer", what);
    if (cin <= 0 || cin % 16) return fail(ISR_ERR_UNSUPPORTED, "%s: cin %d must be a positive multiple of 16", what, cin);
    if (cout <= 0 || cout % 32)
        return fail(ISR_ERR_UNSUPPORTED, "%s: cout %d must be a positive multiple of 32", what, cout);
    return ISR_OK;
}

// The rules the 8-bit and the 16-bit frame descriptors share (both carry n, h, w, layout, siting, src, dst).
template <class D>
static int yuv420_ok(const char* what, const D* d) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "%s: null descriptor", what);
    if (!d->src || !d->dst) return fail(ISR_ERR_BAD_DESC, "%s: null src / dst", what);
    if (d->dst == d->src) return fail(ISR_ERR_BAD_DESC, "%s: dst must not be src", what);
    if (int rc = batch_ok(what, d->n, d->h, d->w, false)) return rc;
    if (d->h < 2 || d->w < 2 || d->h % 2 || d->w % 2)
        return fail(ISR_ERR_BAD_DESC, "%s: 4:2:0 needs even h and w of at least 2, got %dx%d", what, d->h, d->w);
    if ((long long)d->h * d->w > (1ll << 28))
        return fail(ISR_ERR_UNSUPPORTED, "%s: h*w = %lld is more than 2^28", what, (long long)d->h * d->w);
    if (d->layout != ISR_YUV_I420 && d->layout != ISR_YUV_NV12)
        return fail(ISR_ERR_UNSUPPORTED, "%s: unknown layout %d (ISR_YUV_I420, NV12 = 0, 1)", what, d->layout);
    if (d->siting != ISR_YUV_SITING_LEFT && d->siting != ISR_YUV_SITING_CENTER)
        return fail(ISR_ERR_UNSUPPORTED, "%s: unknown siting %d (ISR_YUV_SITING_LEFT, CENTER = 0, 1)", what, d->siting);
    return ISR_OK;
}

extern "C" {

const char* isr_last_error(void) { return g_err; }
int isr_version(void) { return 1; }

// ---- multi-tensor optimiser ops ----

static int mt_ok(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int32_t n, const char* what) {
    if (!ts || !cs) return fail(ISR_ERR_BAD_DESC, "%s: null tensor / chunk table", what);
    if (n <= 0 || n > (1 << 30)) return fail(ISR_ERR_BAD_DESC, "%s: bad chunk count %d", what, n);
    return ISR_OK;
}

int isr_mt_adam_guarded(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int32_t n, const isr_adam_args* a,
                        const float* scale, const uint32_t* guard, isr_stream_t s) {
    if (int rc = mt_ok(ts, cs, n, "mt_adam")) return rc;
    if (!a) return fail(ISR_ERR_BAD_DESC, "mt_adam: null args");
    if (!(a->bc2_sqrt > 0.f) || !(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f))
        return fail(ISR_ERR_BAD_DESC, "mt_adam: bad betas / bias correction");
    return launched(isr::mt_adam_dispatch(ts, cs, n, a, scale, guard, (hipStream_t)s), "mt_adam");
}

int isr_mt_adam(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int32_t n, const isr_adam_args* a,
                const float* scale, isr_stream_t s) {
    return isr_mt_adam_guarded(ts, cs, n, a, scale, nullptr, s);
}

int isr_mt_sumsq(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int32_t n, float* partial, isr_stream_t s) {
    if (int rc = mt_ok(ts, cs, n, "mt_sumsq")) return rc;
    if (!partial) return fail(ISR_ERR_BAD_DESC, "mt_sumsq: null partial buffer");
    return launched(isr::mt_sumsq_dispatch(ts, cs, n, partial, (hipStream_t)s), "mt_sumsq");
}

int isr_clip_coef(const float* partial, int32_t n, float max_norm, float* out, isr_stream_t s) {
    if (!partial || !out || n <= 0) return fail(ISR_ERR_BAD_DESC, "clip_coef: bad arguments");
    return launched(isr::clip_coef_dispatch(partial, n, max_norm, out, (hipStream_t)s), "clip_coef");
}

int isr_mt_scale(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int32_t n, const float* coef, isr_stream_t s) {
    if (int rc = mt_ok(ts, cs, n, "mt_scale")) return rc;
    if (!coef) return fail(ISR_ERR_BAD_DESC, "mt_scale: null coefficient");
    return launched(isr::mt_axpby_dispatch(ts, cs, n, 0, coef, 0.f, nullptr, (hipStream_t)s), "mt_scale");
}

int isr_mt_lerp_guarded(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int32_t n, float d, const uint32_t* guard,
                        isr_stream_t s) {
    if (int rc = mt_ok(ts, cs, n, "mt_lerp")) return rc;
    return launched(isr::mt_axpby_dispatch(ts, cs, n, 1, nullptr, d, guard, (hipStream_t)s), "mt_lerp");
}

int isr_mt_lerp(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int32_t n, float d, isr_stream_t s) {
    return isr_mt_lerp_guarded(ts, cs, n, d, nullptr, s);
}

// ---- weight packs ----

size_t isr_conv3x3_packed_bytes(int32_t cout, int32_t cin) { return isr::conv3x3_packed_bytes(cout, cin); }
size_t isr_head9x9_packed_bytes(int32_t cout, int32_t cin) { (void)cin; return isr::head9x9_packed_bytes(cout); }
size_t isr_tail9x9_packed_bytes(int32_t cout, int32_t cin) { (void)cout; (void)cin; return isr::tail9x9_packed_bytes(); }
size_t isr_conv3x3_wino_packed_bytes(int32_t cout, int32_t cin) {
    if (cout <= 0 || cin <= 0) return 0;
    return isr::conv3x3_wino_packed_bytes(cout, cin);
}

int isr_pack_conv3x3(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s) {
    if (int rc = pack3x3_ok("pack_conv3x3", w, packed, cout, cin)) return rc;
    return launched(isr::conv3x3_pack(w, packed, cout, cin, (hipStream_t)s), "pack_conv3x3");
}

int isr_pack_conv3x3_f16(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s) {
    if (int rc = pack3x3_ok("pack_conv3x3_f16", w, packed, cout, cin)) return rc;
    return launched(isr::conv3x3_pack_f16(w, packed, cout, cin, (hipStream_t)s), "pack_conv3x3_f16");
}

int isr_pack_conv3x3_wino_f16(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s) {
    if (int rc = pack3x3_ok("pack_conv3x3_wino_f16", w, packed, cout, cin)) return rc;
    return launched(isr::conv3x3_wino_pack(w, packed, cout, cin, (hipStream_t)s), "pack_conv3x3_wino_f16");
}

int isr_pack_conv3x3_dgrad(const float* w, void* packed, int32_t cout, int32_t cin, float scale, int32_t sub2,
                           isr_stream_t s) {
    if (!w || !packed) return fail(ISR_ERR_BAD_DESC, "pack_conv3x3_dgrad: null pointer");
    if (cin <= 0 || cin % 32 || cout <= 0 || cout % 32)
        return fail(ISR_ERR_UNSUPPORTED, "pack_conv3x3_dgrad: cin %d / cout %d must be multiples of 32", cin, cout);
    if (sub2 && cout % 128) return fail(ISR_ERR_UNSUPPORTED, "pack_conv3x3_dgrad: sub2 needs cout %% 128 == 0");
    return launched(isr::conv3x3_pack_dgrad(w, packed, cout, cin, scale, sub2, (hipStream_t)s), "pack_conv3x3_dgrad");
}

int isr_pack_conv3x3_batch(const isr_pack_item* items, int32_t n, isr_stream_t s) {
    if (!items || n <= 0 || n > 65535) return fail(ISR_ERR_BAD_DESC, "pack_conv3x3_batch: bad item table (n=%d)", n);
    return launched(isr::conv3x3_pack_batch(items, n, (hipStream_t)s), "pack_conv3x3_batch");
}

static int pack_head_any(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s, bool h) {
    if (!w || !packed) return fail(ISR_ERR_BAD_DESC, "pack_head9x9: null pointer");
    if (cout != 64 || cin < 1 || cin > 3) return fail(ISR_ERR_UNSUPPORTED, "pack_head9x9: need cout 64, cin <= 3 (got %d, %d)", cout, cin);
    return launched(isr::head9x9_pack(w, packed, cout, cin, (hipStream_t)s, h), "pack_head9x9");
}
int isr_pack_head9x9(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s) {
    return pack_head_any(w, packed, cout, cin, s, false);
}
int isr_pack_head9x9_f16(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s) {
    return pack_head_any(w, packed, cout, cin, s, true);
}

static int pack_tail_any(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s, bool h) {
    if (!w || !packed) return fail(ISR_ERR_BAD_DESC, "pack_tail9x9: null pointer");
    if (cout != 3 || cin != 64) return fail(ISR_ERR_UNSUPPORTED, "pack_tail9x9: need cout 3, cin 64 (got %d, %d)", cout, cin);
    return launched(isr::tail9x9_pack(w, packed, cout, cin, (hipStream_t)s, h), "pack_tail9x9");
}
int isr_pack_tail9x9(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s) {
    return pack_tail_any(w, packed, cout, cin, s, false);
}
int isr_pack_tail9x9_f16(const float* w, void* packed, int32_t cout, int32_t cin, isr_stream_t s) {
    return pack_tail_any(w, packed, cout, cin, s, true);
}

// ---- the 3x3 conv ----

static int conv3x3_validate(const isr_conv_desc* d) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "conv3x3: null descriptor");
    if (int rc = tile_grid_ok("conv3x3", d)) return rc;
    if (d->cin <= 0 || d->cin % 16) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: cin %d must be a multiple of 16", d->cin);
    if (d->cout <= 0 || d->cout % 32)
        return fail(ISR_ERR_UNSUPPORTED, "conv3x3: cout %d must be a positive multiple of 32", d->cout);
    if (!d->wpack) return fail(ISR_ERR_BAD_DESC, "conv3x3: null weights");
    if (d->shuffle != 1 && d->shuffle != 2) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: shuffle must be 1 or 2");
    if (d->taps < 0 || d->taps > 2) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: taps must be 0, 1 or 2");
    if (d->taps && d->cout % 64) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: a 2x2 tap window needs cout %% 64 == 0");
    const int up = d->shuffle == 2 ? 2 : 1;  // a shuffled store's y and m are on the (2h x 2w) grid, cout / 4 channels
    if (d->x_sub2) {
        if (d->cin % 128) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: x_sub2 needs cin %% 128 == 0 (got %d)", d->cin);
        if (d->shuffle != 1) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: x_sub2 with a shuffled store");
        if (int rc = view_ok(d->x, 2 * d->ha, 2 * d->wa, 2, d->cin / 4, "conv3x3.x")) return rc;
    } else if (int rc = view_ok(d->x, d->ha, d->wa, 1, d->cin, "conv3x3.x")) {
        return rc;
    }
    if (d->m.data) {
        if (d->y2.data) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: mask epilogue takes no second output");
        if (d->m_c0 < 0 || d->m_c0 % 32) return fail(ISR_ERR_BAD_DESC, "conv3x3: m_c0 %d must be a multiple of 32", d->m_c0);
        if (up == 2 && d->m_c0) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: a shuffled store masks all channels (m_c0 = 0)");
        if (int rc = view_ok(d->m, up * d->ha, up * d->wa, 0, d->cout / (up * up), "conv3x3.m")) return rc;
    }
    if (d->r1_cn < 0 || d->r1_cn % 32) return fail(ISR_ERR_BAD_DESC, "conv3x3: r1_cn %d must be a multiple of 32", d->r1_cn);
    if (up == 2) {
        if (d->cout % 64) return fail(ISR_ERR_UNSUPPORTED, "conv3x3: pixel shuffle needs cout %% 64 == 0");
        if (d->r1.data || d->r2.data || d->y2.data)
            return fail(ISR_ERR_UNSUPPORTED, "conv3x3: pixel shuffle store takes no residual / second output");
    }
    if (int rc = view_ok(d->y, up * d->ha, up * d->wa, 0, d->cout / (up * up), "conv3x3.y")) return rc;
    if (int rc = opt_view_ok(d->y2, d->ha, d->wa, 0, d->cout, "conv3x3.y2")) return rc;
    if (int rc = opt_view_ok(d->r1, d->ha, d->wa, 0, d->cout, "conv3x3.r1")) return rc;
    if (int rc = opt_view_ok(d->r2, d->ha, d->wa, 0, d->cout, "conv3x3.r2")) return rc;
    if (d->bias && ((uintptr_t)d->bias % 16)) return fail(ISR_ERR_BAD_DESC, "conv3x3: bias must be 16-byte aligned");
    if (d->f16 != 0 && d->f16 != 1) return fail(ISR_ERR_BAD_DESC, "conv3x3: f16 must be 0 or 1");
    if (d->f16 && (d->m.data || d->x_sub2 || d->taps))
        return fail(ISR_ERR_UNSUPPORTED, "conv3x3: fp16 activations are forward-only (no mask, x_sub2 or tap window)");
    return ISR_OK;
}

int isr_conv3x3_check(const isr_conv_desc* d) { return conv3x3_validate(d); }

int isr_conv3x3_fwd(const isr_conv_desc* d, isr_stream_t s) {
    if (int rc = conv3x3_validate(d)) return rc;
    return launched(isr::conv3x3_fwd_dispatch(d, (hipStream_t)s), "conv3x3");
}

int isr_conv3x3_fwd_variant(const isr_conv_desc* d, int32_t variant, isr_stream_t s) {
    if (int rc = conv3x3_validate(d)) return rc;
    const int rc = isr::conv3x3_fwd_variant(d, variant, (hipStream_t)s);
    if (rc == DISPATCH_UNSUPPORTED)
        return fail(ISR_ERR_UNSUPPORTED, "conv3x3: variant %d not available for cout %d / cin %d", variant, d->cout, d->cin);
    return launched(rc, "conv3x3");
}

// The Winograd form's own restrictions first (each names its field), then the direct form's
// descriptor rules; nothing touches the GPU before both pass.
int isr_conv3x3_wino_fwd(const isr_conv_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "conv3x3_wino: null descriptor");
    if (d->f16 != 1) return fail(ISR_ERR_UNSUPPORTED, "conv3x3_wino: f16 must be 1 (fp16 storage only, got %d)", d->f16);
    if (d->shuffle != 1) return fail(ISR_ERR_UNSUPPORTED, "conv3x3_wino: shuffle must be 1 (plain store, got %d)", d->shuffle);
    if (d->m.data) return fail(ISR_ERR_UNSUPPORTED, "conv3x3_wino: m (mask epilogue) is not supported");
    if (d->x_sub2) return fail(ISR_ERR_UNSUPPORTED, "conv3x3_wino: x_sub2 is not supported");
    if (d->taps) return fail(ISR_ERR_UNSUPPORTED, "conv3x3_wino: taps (tap window) is not supported");
    if (int rc = conv3x3_validate(d)) return rc;
    return launched(isr::conv3x3_wino_fwd_dispatch(d, (hipStream_t)s), "conv3x3_wino");
}

// ---- the persistent chain ----

static bool chain_grid_ok(int n, int ha, int wa) { return n > 0 && ha > 0 && wa > 0 && ha % 16 == 0 && wa % 32 == 0; }

// (the round-2 chain's progress words, (tiles + 7) / 4 * 4, were always fewer than the trunk's)
size_t isr_conv_chain_state_words(int32_t n, int32_t ha, int32_t wa) {
    return chain_grid_ok(n, ha, wa) ? isr::trunk_state_words(n, ha, wa) : 0;
}

// The A/B forms that lost against a shipping kernel were removed from both builds.
#define ISR_REMOVED_FORM "is a removed A/B form (its measurements: DESIGN.md section 5)"

int isr_conv_chain_variant(const isr_chain_desc* c, int32_t variant, isr_stream_t s) {
    if (!c || !c->layers || !c->kinds || !c->state || c->nl <= 0 || c->nl > 1024)
        return fail(ISR_ERR_BAD_DESC, "conv chain: null layers / kinds / state or nl not in [1, 1024]");
    if (!chain_grid_ok(c->n, c->ha, c->wa))
        return fail(ISR_ERR_BAD_DESC, "conv chain: bad grid n=%d ha=%d wa=%d", c->n, c->ha, c->wa);
    if (c->f16 != 0 && c->f16 != 1) return fail(ISR_ERR_BAD_DESC, "conv chain: f16 must be 0 or 1");
    if (variant != 0) return fail(ISR_ERR_UNSUPPORTED, "conv chain: variant %d " ISR_REMOVED_FORM, variant);
    const int rc = isr::trunk_launch(c, (hipStream_t)s);
    if (rc == DISPATCH_NO_OCCUPANCY) return fail(ISR_ERR_LAUNCH, "conv chain: the occupancy query admits no workgroup per CU");
    if (rc == DISPATCH_UNSUPPORTED) return fail(ISR_ERR_UNSUPPORTED, "conv chain: unsupported grid or layer count");
    return launched(rc, "conv chain");
}

int isr_conv_chain(const isr_chain_desc* c, isr_stream_t s) { return isr_conv_chain_variant(c, 0, s); }

int isr_tuning_trunk_knobs(int32_t ablate, int32_t per_cu, int32_t k2, int32_t k3) {
    const int k[4] = {ablate, per_cu, k2, k3};
    return tuning_set(isr::trunk_knobs_set(k), "trunk knobs");
}
int isr_tuning_trunk_item_stamps(void* buf) { return tuning_set(isr::trunk_item_stamps_set(buf), "trunk item stamps"); }
int isr_tuning_trunk_stamps(void* buf) { return tuning_set(isr::trunk_stamps_set(buf), "trunk stamps"); }
int isr_tuning_conv_stamps(void* buf) { return tuning_set(isr::conv_stamps_set(buf), "conv stamps"); }

int isr_tuning_chain_knobs(int32_t, int32_t, int32_t, int32_t) {
    return fail(ISR_ERR_UNSUPPORTED, "chain knobs: the round-2 chain kernel that read them " ISR_REMOVED_FORM);
}

int isr_tuning_tail_stamps(void*) {
    return fail(ISR_ERR_UNSUPPORTED, "tail stamps: the 4-wave tail walk that wrote them " ISR_REMOVED_FORM);
}

// ---- the 9x9 head and tail ----

int isr_head9x9_fwd(const isr_head_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "head9x9: null descriptor");
    if (int rc = tile_grid_ok("head9x9", d)) return rc;
    if (d->cout != 64) return fail(ISR_ERR_UNSUPPORTED, "head9x9: cout must be 64");
    if (!d->x || !d->wpack) return fail(ISR_ERR_BAD_DESC, "head9x9: null input or weights");
    if (int rc = view_ok(d->y, d->ha, d->wa, 0, 64, "head9x9.y")) return rc;
    if (int rc = opt_view_ok(d->y2, d->ha, d->wa, 0, 64, "head9x9.y2")) return rc;
    if (int rc = opt_view_ok(d->m, d->ha, d->wa, 0, 64, "head9x9.m")) return rc;
    if (d->bias && ((uintptr_t)d->bias % 16)) return fail(ISR_ERR_BAD_DESC, "head9x9: bias must be 16-byte aligned");
    if (d->f16 != 0 && d->f16 != 1) return fail(ISR_ERR_BAD_DESC, "head9x9: f16 must be 0 or 1");
    if (d->f16 && d->m.data) return fail(ISR_ERR_UNSUPPORTED, "head9x9: fp16 activations are forward-only (no mask)");
    return launched(isr::head9x9_fwd_dispatch(d, (hipStream_t)s), "head9x9");
}

static int tail_validate(const isr_tail_desc* d) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "tail9x9: null descriptor");
    if (int rc = tile_grid_ok("tail9x9", d)) return rc;
    if (d->cin != 64) return fail(ISR_ERR_UNSUPPORTED, "tail9x9: cin must be 64");
    if (!d->y || !d->wpack) return fail(ISR_ERR_BAD_DESC, "tail9x9: null output or weights");
    if (int rc = view_ok(d->x, d->ha, d->wa, 4, 64, "tail9x9.x")) return rc;
    if (d->f16 != 0 && d->f16 != 1) return fail(ISR_ERR_BAD_DESC, "tail9x9: f16 must be 0 or 1");
    return ISR_OK;
}

int isr_tail9x9_fwd(const isr_tail_desc* d, isr_stream_t s) {
    if (int rc = tail_validate(d)) return rc;
    return launched(isr::tail9x9_fwd_dispatch(d, (hipStream_t)s), "tail9x9");
}

int isr_tail9x9_fwd_variant(const isr_tail_desc* d, int32_t variant, isr_stream_t s) {
    if (int rc = tail_validate(d)) return rc;
    if (variant != 0 && variant != 3 && variant != 5)
        return fail(ISR_ERR_UNSUPPORTED, "tail9x9: variant %d " ISR_REMOVED_FORM, variant);
    return launched(isr::tail9x9_fwd_variant(d, variant, (hipStream_t)s), "tail9x9");
}

int32_t isr_tail9x9_segment_rows(const isr_tail_desc* d, int32_t cus) {
    if (int rc = tail_validate(d)) return rc;
    const int sh = isr::tail_segment_rows(d, cus > 0 ? cus : isr::cu_count());
    if (sh < 0) return fail(ISR_ERR_BAD_DESC, "tail9x9: no segment height divides ha = %d", d->ha);
    g_err[0] = 0;
    return sh;
}

// ---- weight gradients ----

static int wgrad_validate(const isr_wgrad_desc* d) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "wgrad3x3: null descriptor");
    if (int rc = tile_grid_ok("wgrad3x3", d)) return rc;
    if (d->cin <= 0 || d->cin % 32 || d->cout <= 0 || d->cout % 32)
        return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3: cin %d / cout %d must be multiples of 32", d->cin, d->cout);
    if (!d->dw) return fail(ISR_ERR_BAD_DESC, "wgrad3x3: null dw");
    if (d->splits < 0) return fail(ISR_ERR_BAD_DESC, "wgrad3x3: negative split count");
    if (d->taps < 0 || d->taps > 1) return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3: taps must be 0 or 1");
    if (d->x_sub2) {
        if (d->cin % 128) return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3: x_sub2 needs cin %% 128 == 0 (got %d)", d->cin);
        if (d->g_sub2) return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3: x_sub2 with g_sub2");
        if (int rc = view_ok(d->x, 2 * d->ha, 2 * d->wa, 2, d->cin / 4, "wgrad3x3.x")) return rc;
    } else if (int rc = view_ok(d->x, d->ha, d->wa, 1, d->cin, "wgrad3x3.x")) {
        return rc;
    }
    if (d->g_sub2) {
        if (d->cout % 128) return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3: g_sub2 needs cout %% 128 == 0");
        return view_ok(d->g, 2 * d->ha, 2 * d->wa, 0, d->cout / 4, "wgrad3x3.g");
    }
    return view_ok(d->g, d->ha, d->wa, 0, d->cout, "wgrad3x3.g");
}

// production: 0 and 16 (the compiler-read reference of the same tiles); tuning builds also 1-15
static bool wgrad_variant_built(int32_t variant) {
#ifdef ISR_TUNING
    return variant >= 0 && variant <= 16;
#else
    return variant == 0 || variant == 16;
#endif
}

size_t isr_wgrad3x3_variant_workspace_bytes(const isr_wgrad_desc* d, int32_t variant) {
    if (wgrad_validate(d) != ISR_OK || !wgrad_variant_built(variant)) return 0;
    return isr::wgrad3x3_workspace_bytes(d, variant);
}

size_t isr_wgrad3x3_workspace_bytes(const isr_wgrad_desc* d) { return isr_wgrad3x3_variant_workspace_bytes(d, 0); }

static int wgrad3x3_parts(const isr_wgrad_desc* d, int32_t variant, void* workspace, size_t ws_bytes,
                          isr_stream_t s, int parts) {
    if (int rc = wgrad_validate(d)) return rc;
    if (int rc = workspace_ok("wgrad3x3", workspace)) return rc;
    if (!wgrad_variant_built(variant)) return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3: no variant %d in this library%s",
                                                   variant, variant >= 1 && variant <= 15 ? " (tuning form: build with "
                                                   "-DISR_TUNING)" : "");
    const int rc = isr::wgrad3x3_dispatch(d, variant, workspace, ws_bytes, (hipStream_t)s, parts);
    if (rc == DISPATCH_UNSUPPORTED)
        return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3: variant %d needs ha %% stage rows == 0 and cout / cin multiples "
                    "of its tile", variant);
    return workspace_launched(rc, "wgrad3x3", ws_bytes, [&] { return isr::wgrad3x3_workspace_bytes(d, variant); });
}

int isr_wgrad3x3_variant(const isr_wgrad_desc* d, int32_t variant, void* workspace, size_t ws_bytes,
                         isr_stream_t s) {
    return wgrad3x3_parts(d, variant, workspace, ws_bytes, s, 3);
}
int isr_wgrad3x3(const isr_wgrad_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s) {
    return wgrad3x3_parts(d, 0, workspace, ws_bytes, s, 3);
}
int isr_wgrad3x3_partials(const isr_wgrad_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s) {
    return wgrad3x3_parts(d, 0, workspace, ws_bytes, s, 1);
}
int isr_wgrad3x3_reduce(const isr_wgrad_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s) {
    return wgrad3x3_parts(d, 0, workspace, ws_bytes, s, 2);
}

static int wgrad_group_validate(const isr_wgrad_desc* ds, int32_t n) {
    if (!ds || n < 1 || n > 5) return fail(ISR_ERR_BAD_DESC, "wgrad3x3 group: null descriptors or n not in [1, 5]");
    for (int t = 0; t < n; ++t) {
        if (int rc = wgrad_validate(&ds[t])) return rc;
        if (ds[t].g_sub2 || ds[t].x_sub2 || ds[t].taps || ds[t].n != ds[0].n || ds[t].ha != ds[0].ha ||
            ds[t].wa != ds[0].wa)
            return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3 group: member %d is not a plain 3x3 conv on the first "
                        "member's grid", t);
    }
    return ISR_OK;
}

size_t isr_wgrad3x3_group_workspace_bytes(const isr_wgrad_desc* descs, int32_t n) {
    if (wgrad_group_validate(descs, n) != ISR_OK) return 0;
    return isr::wgrad3x3_group_workspace_bytes(descs, n, 0);
}

int isr_wgrad3x3_group_variant(const isr_wgrad_desc* descs, int32_t n, int32_t variant, void* workspace,
                               size_t ws_bytes, isr_stream_t s) {
    if (int rc = wgrad_group_validate(descs, n)) return rc;
    if (int rc = workspace_ok("wgrad3x3 group", workspace)) return rc;
    if (variant != 0 && variant != 1) return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3 group: no variant %d", variant);
    const int rc = isr::wgrad3x3_group_dispatch(descs, n, workspace, ws_bytes, (hipStream_t)s, variant);
    if (rc == DISPATCH_UNSUPPORTED)
        return fail(ISR_ERR_UNSUPPORTED, "wgrad3x3 group: a member's cout / cin / ha does not fit the tile");
    return workspace_launched(rc, "wgrad3x3 group", ws_bytes,
                              [&] { return isr::wgrad3x3_group_workspace_bytes(descs, n, variant); });
}

int isr_wgrad3x3_group(const isr_wgrad_desc* descs, int32_t n, void* workspace, size_t ws_bytes, isr_stream_t s) {
    return isr_wgrad3x3_group_variant(descs, n, 0, workspace, ws_bytes, s);
}

static int wgrad9_validate(const isr_wgrad9_desc* d) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "wgrad9x9: null descriptor");
    if (int rc = tile_grid_ok("wgrad9x9", d)) return rc;
    if (!d->p || !d->dw) return fail(ISR_ERR_BAD_DESC, "wgrad9x9: null p / dw");
    if (d->splits < 0) return fail(ISR_ERR_BAD_DESC, "wgrad9x9: negative split count");
    return view_ok(d->q, d->ha, d->wa, d->head ? 0 : 4, 64, "wgrad9x9.q");
}

size_t isr_wgrad9x9_workspace_bytes(const isr_wgrad9_desc* d) {
    if (wgrad9_validate(d) != ISR_OK) return 0;
    return isr::wgrad9x9_workspace_bytes(d);
}

int isr_wgrad9x9(const isr_wgrad9_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s) {
    if (int rc = wgrad9_validate(d)) return rc;
    if (int rc = workspace_ok("wgrad9x9", workspace)) return rc;
    return workspace_launched(isr::wgrad9x9_dispatch(d, workspace, ws_bytes, (hipStream_t)s), "wgrad9x9", ws_bytes,
                              [&] { return isr::wgrad9x9_workspace_bytes(d); });
}

// ---- elementwise glue, layout, pool, BatchNorm ----

int isr_ew_combine(const isr_ew_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "ew_combine: null descriptor");
    if (int rc = blocked_grid_ok("ew_combine", d, 16)) return rc;
    if (int rc = view_ok(d->y, d->ha, d->wa, 0, d->c, "ew.y")) return rc;
    if (int rc = view_ok(d->a, d->ha, d->wa, 0, d->c, "ew.a")) return rc;
    if (int rc = opt_view_ok(d->b, d->ha, d->wa, 0, d->c, "ew.b")) return rc;
    if (int rc = opt_view_ok(d->m, d->ha, d->wa, 0, d->c, "ew.m")) return rc;
    return launched(isr::ew_combine_dispatch(d, (hipStream_t)s), "ew_combine");
}

int isr_sr_transform(const isr_sr_transform_desc* d, isr_stream_t s) {
    if (!d || !d->crops || !d->hr || !d->lr) return fail(ISR_ERR_BAD_DESC, "sr_transform: null descriptor / buffer");
    if (d->scale < 2 || d->scale > 4) return fail(ISR_ERR_UNSUPPORTED, "sr_transform: scale %d not in {2, 3, 4}", d->scale);
    if (d->n <= 0 || d->t <= 0 || d->t % d->scale || (long long)d->n * 3 * d->t * d->t >= (1ll << 31))
        return fail(ISR_ERR_BAD_DESC, "sr_transform: bad batch n=%d t=%d scale=%d", d->n, d->t, d->scale);
    for (int c = 0; c < 3; ++c)
        if (!(d->std[c] != 0.f)) return fail(ISR_ERR_BAD_DESC, "sr_transform: std[%d] is zero", c);
    return launched(isr::sr_transform_dispatch(d, (hipStream_t)s), "sr_transform");
}

int isr_pixel_shuffle2(const isr_ew_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "pixel_shuffle2: null descriptor");
    if (int rc = blocked_grid_ok("pixel_shuffle2", d, 16)) return rc;
    if (d->h % 2 || d->w % 2) return fail(ISR_ERR_BAD_DESC, "pixel_shuffle2: output %dx%d must be even", d->h, d->w);
    if (d->ha % 2 || d->wa % 2)
        return fail(ISR_ERR_BAD_DESC, "pixel_shuffle2: computed region %dx%d must be even", d->ha, d->wa);
    if (d->b.data || d->m.data) return fail(ISR_ERR_UNSUPPORTED, "pixel_shuffle2: takes no b / m operand");
    if (int rc = view_ok(d->y, d->ha, d->wa, 0, d->c, "pixel_shuffle2.y")) return rc;
    if (int rc = view_ok(d->a, d->ha / 2, d->wa / 2, 0, 4 * d->c, "pixel_shuffle2.a")) return rc;
    return launched(isr::pixel_shuffle2_dispatch(d, (hipStream_t)s), "pixel_shuffle2");
}

int isr_pixel_unshuffle2(const isr_ew_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "pixel_unshuffle2: null descriptor");
    if (int rc = blocked_grid_ok("pixel_unshuffle2", d, 64)) return rc;
    if (d->b.data) return fail(ISR_ERR_UNSUPPORTED, "pixel_unshuffle2: takes no b operand");
    if (int rc = view_ok(d->y, d->ha, d->wa, 0, d->c, "pixel_unshuffle2.y")) return rc;
    if (int rc = view_ok(d->a, 2 * d->ha, 2 * d->wa, 0, d->c / 4, "pixel_unshuffle2.a")) return rc;
    if (int rc = opt_view_ok(d->m, 2 * d->ha, 2 * d->wa, 0, d->c / 4, "pixel_unshuffle2.m")) return rc;
    return launched(isr::pixel_unshuffle2_dispatch(d, (hipStream_t)s), "pixel_unshuffle2");
}

static int convert_validate(const isr_convert_desc* d, const char* who) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "%s: null descriptor", who);
    if (int rc = blocked_grid_ok(who, d, 1)) return rc;  // any c: the view holds it rounded up to whole blocks
    if (!d->nchw) return fail(ISR_ERR_BAD_DESC, "%s: null nchw pointer", who);
    const int blocked = (d->c + 15) / 16 * 16;
    if (int rc = view_ok(d->v, d->ha, d->wa, 0, blocked, who)) return rc;
    return opt_view_ok(d->m, d->ha, d->wa, 0, blocked, who);
}

int isr_nchw_to_blocked(const isr_convert_desc* d, isr_stream_t s) {
    if (int rc = convert_validate(d, "nchw_to_blocked")) return rc;
    return launched(isr::nchw_to_blocked_dispatch(d, (hipStream_t)s), "nchw_to_blocked");
}

int isr_blocked_to_nchw(const isr_convert_desc* d, isr_stream_t s) {
    if (int rc = convert_validate(d, "blocked_to_nchw")) return rc;
    return launched(isr::blocked_to_nchw_dispatch(d, (hipStream_t)s), "blocked_to_nchw");
}

static int pool_run(const isr_pool_desc* d, int bwd, isr_stream_t s, const char* what) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "maxpool2: null descriptor");
    if (d->n <= 0 || d->h < 2 || d->w < 2 || d->c <= 0 || d->c % 16)
        return fail(ISR_ERR_BAD_DESC, "maxpool2: bad problem n=%d h=%d w=%d c=%d", d->n, d->h, d->w, d->c);
    if (d->hao < d->h / 2 || d->wao < d->w / 2) return fail(ISR_ERR_BAD_DESC, "maxpool2: output region too small");
    if (int rc = view_ok(d->x, 2 * d->hao, 2 * d->wao, 0, d->c, "maxpool2.x")) return rc;
    if (int rc = view_ok(d->y, d->hao, d->wao, 0, d->c, "maxpool2.y")) return rc;
    if (bwd)
        if (int rc = view_ok(d->g, 2 * d->hao, 2 * d->wao, 0, d->c, "maxpool2.g")) return rc;
    return launched(isr::maxpool2_dispatch(d, bwd, (hipStream_t)s), what);
}

int isr_maxpool2_fwd(const isr_pool_desc* d, isr_stream_t s) { return pool_run(d, 0, s, "maxpool2_fwd"); }
int isr_maxpool2_bwd(const isr_pool_desc* d, isr_stream_t s) { return pool_run(d, 1, s, "maxpool2_bwd"); }

// op: 0 stats (reads z), 1 finalize (no view), 2 apply (z, y, r1, r2), 3 bwd_reduce (z, y), 4 bwd_apply (z, y, dz)
static int bn_run(const isr_bn_desc* d, int op, isr_stream_t s, const char* what) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "bn: null descriptor");
    if (int rc = blocked_grid_ok("bn", d, 16, 1024)) return rc;
    if (!d->acc || !d->save) return fail(ISR_ERR_BAD_DESC, "bn: null acc / save");
    if (op != 1)
        if (int rc = view_ok(d->z, d->ha, d->wa, 0, d->c, "bn.z")) return rc;
    if (op >= 2)
        if (int rc = view_ok(d->y, d->ha, d->wa, 0, d->c, "bn.y")) return rc;
    if (op == 2) {
        if (int rc = opt_view_ok(d->r1, d->ha, d->wa, 0, d->c, "bn.r1")) return rc;
        if (int rc = opt_view_ok(d->r2, d->ha, d->wa, 0, d->c, "bn.r2")) return rc;
    }
    if (op == 4)
        if (int rc = opt_view_ok(d->dz, d->ha, d->wa, 0, d->c, "bn.dz")) return rc;
    if ((op == 2 || op == 4) && (!d->gamma || (op == 2 && !d->beta)))
        return fail(ISR_ERR_BAD_DESC, "bn: null gamma / beta");
    if (op == 1 && (!d->running_mean) != (!d->running_var)) return fail(ISR_ERR_BAD_DESC, "bn: running stats pair");
    return launched(isr::bn_dispatch(d, op, (hipStream_t)s), what);
}

int isr_bn_stats(const isr_bn_desc* d, isr_stream_t s) { return bn_run(d, 0, s, "bn_stats"); }
int isr_bn_finalize(const isr_bn_desc* d, isr_stream_t s) { return bn_run(d, 1, s, "bn_finalize"); }
int isr_bn_apply(const isr_bn_desc* d, isr_stream_t s) { return bn_run(d, 2, s, "bn_apply"); }
int isr_bn_bwd_reduce(const isr_bn_desc* d, isr_stream_t s) { return bn_run(d, 3, s, "bn_bwd_reduce"); }
int isr_bn_bwd_apply(const isr_bn_desc* d, isr_stream_t s) { return bn_run(d, 4, s, "bn_bwd_apply"); }

// Nothing is launched for a refused descriptor; the size query validates the same way (out and the
// image pointers are not needed to size the workspace, so it accepts them null).
static int metrics_validate(const isr_metrics_desc* d, bool need_ptrs) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "image_metrics: null descriptor");
    if (need_ptrs && (!d->a || !d->b || !d->out)) return fail(ISR_ERR_BAD_DESC, "image_metrics: null a / b / out");
    if (int rc = batch_ok("image_metrics", d->n, d->h, d->w, false)) return rc;
    if (d->border < 0) return fail(ISR_ERR_BAD_DESC, "image_metrics: negative border %d", d->border);
    const long long hc = (long long)d->h - 2ll * d->border, wc = (long long)d->w - 2ll * d->border;
    if (hc < 11 || wc < 11)
        return fail(ISR_ERR_UNSUPPORTED, "image_metrics: %dx%d less a border of %d leaves %lldx%lld, smaller than the "
                    "11-pixel SSIM window", d->h, d->w, d->border, hc, wc);
    return ISR_OK;
}

size_t isr_image_metrics_workspace_bytes(const isr_metrics_desc* d) {
    if (metrics_validate(d, false) != ISR_OK) return 0;
    return isr::image_metrics_workspace_bytes(d);
}

int isr_image_metrics(const isr_metrics_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s) {
    if (int rc = metrics_validate(d, true)) return rc;
    if (int rc = workspace_ok("image_metrics", workspace)) return rc;
    return workspace_launched(isr::image_metrics_dispatch(d, workspace, ws_bytes, (hipStream_t)s), "image_metrics",
                              ws_bytes, [&] { return isr::image_metrics_workspace_bytes(d); });
}

// ---- training-data degradations (degrade.hip) ----

static int jpeg_validate(const isr_jpeg_desc* d, bool need_ptrs) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "jpeg_roundtrip: null descriptor");
    if (need_ptrs && (!d->src || !d->dst || !d->quality))
        return fail(ISR_ERR_BAD_DESC, "jpeg_roundtrip: null src / dst / quality");
    if (int rc = batch_ok("jpeg_roundtrip", d->n, d->h, d->w, true)) return rc;
    if (d->h % 16 || d->w % 16)
        return fail(ISR_ERR_UNSUPPORTED, "jpeg_roundtrip: %dx%d is not whole 4:2:0 MCUs: h and w must be multiples "
                    "of 16", d->h, d->w);
    if (need_ptrs && !(aligned(16, {d->src, d->dst}) && aligned(4, {d->quality})))
        return fail(ISR_ERR_BAD_DESC, "jpeg_roundtrip: src and dst must be 16-byte aligned, quality 4-byte aligned");
    return ISR_OK;
}

size_t isr_jpeg_roundtrip_workspace_bytes(const isr_jpeg_desc* d) {
    if (jpeg_validate(d, false) != ISR_OK) return 0;
    return isr::jpeg_roundtrip_workspace_bytes(d);
}

int isr_jpeg_roundtrip(const isr_jpeg_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s) {
    if (int rc = jpeg_validate(d, true)) return rc;
    if (!workspace || !aligned(16, {workspace}))
        return fail(ISR_ERR_BAD_DESC, "jpeg_roundtrip: null or not 16-byte aligned workspace");
    return workspace_launched(isr::jpeg_roundtrip_dispatch(d, workspace, ws_bytes, (hipStream_t)s), "jpeg_roundtrip",
                              ws_bytes, [&] { return isr::jpeg_roundtrip_workspace_bytes(d); });
}

int isr_hls_l_moments(const isr_hls_moments_desc* d, isr_stream_t s) {
    if (!d || !d->src || !d->out || !d->partials)
        return fail(ISR_ERR_BAD_DESC, "hls_l_moments: null descriptor / src / out / partials");
    if (int rc = batch_ok("hls_l_moments", d->n, d->h, d->w, false)) return rc;
    if (!aligned(8, {d->out, d->partials}))
        return fail(ISR_ERR_BAD_DESC, "hls_l_moments: out and partials must be 8-byte aligned");
    return launched(isr::hls_l_moments_dispatch(d, (hipStream_t)s), "hls_l_moments");
}

int isr_iso_noise(const isr_iso_noise_desc* d, isr_stream_t s) {
    if (!d || !d->src || !d->dst || !d->lum_noise || !d->hue_noise || !d->apply)
        return fail(ISR_ERR_BAD_DESC, "iso_noise: null descriptor / src / dst / lum_noise / hue_noise / apply");
    if (int rc = batch_ok("iso_noise", d->n, d->h, d->w, false)) return rc;
    if (!aligned(4, {d->lum_noise, d->hue_noise, d->apply}))
        return fail(ISR_ERR_BAD_DESC, "iso_noise: lum_noise, hue_noise and apply must be 4-byte aligned");
    const long long hw = (long long)d->h * d->w;
    if ((hw + 255) / 256 >= (1ll << 31))
        return fail(ISR_ERR_UNSUPPORTED, "iso_noise: %dx%d needs more than 2^31 - 1 workgroups per image", d->h, d->w);
    return launched(isr::iso_noise_dispatch(d, (hipStream_t)s), "iso_noise");
}

static int resample_axis_check(const char* what, int filter, int in_size, int out_size) {
    switch (isr::resample_check(filter, in_size, out_size)) {
        case 0: return ISR_OK;
        case 1: return fail(ISR_ERR_UNSUPPORTED, "%s: unknown filter %d (ISR_RESAMPLE_NEAREST..LANCZOS = 0..5)", what, filter);
        case 2: return fail(ISR_ERR_UNSUPPORTED, "%s: sizes %d -> %d outside [1, %d]", what, in_size, out_size,
                            isr::RESAMPLE_MAX_SIZE);
        default: return fail(ISR_ERR_UNSUPPORTED, "%s: ratio %d -> %d outside [1/%d, %d]", what, in_size, out_size,
                             isr::RESAMPLE_MAX_RATIO, isr::RESAMPLE_MAX_RATIO);
    }
}

int isr_resample_ksize(int filter, int in_size, int out_size) {
    if (resample_axis_check("resample_ksize", filter, in_size, out_size) != ISR_OK) return 0;
    g_err[0] = 0;
    return isr::resample_ksize(filter, in_size, out_size);
}

int isr_resample_tables(int filter, int in_size, int out_size, int32_t* bounds, int32_t* coeffs) {
    if (!bounds || !coeffs) return fail(ISR_ERR_BAD_DESC, "resample_tables: null bounds / coeffs");
    if (int rc = resample_axis_check("resample_tables", filter, in_size, out_size)) return rc;
    isr::resample_tables(filter, in_size, out_size, bounds, coeffs);
    g_err[0] = 0;
    return ISR_OK;
}

int isr_resample_u8(const isr_resample_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "resample_u8: null descriptor");
    if (!d->src || !d->bounds_x || !d->coeffs_x || !d->bounds_y || !d->coeffs_y)
        return fail(ISR_ERR_BAD_DESC, "resample_u8: null src / tables");
    if (!d->dst_u8 && !d->lr_f32 && !d->hr_f32) return fail(ISR_ERR_BAD_DESC, "resample_u8: no output requested");
    if (d->n < 1 || d->n > 65535 || d->nf < 1)
        return fail(ISR_ERR_BAD_DESC, "resample_u8: bad batch n=%d nf=%d (n in [1, 65535], nf >= 1)", d->n, d->nf);
    // filter 1 stands in for the size and ratio rules, which are the same for every filter
    if (int rc = resample_axis_check("resample_u8 (height)", 1, d->in_h, d->out_h)) return rc;
    if (int rc = resample_axis_check("resample_u8 (width)", 1, d->in_w, d->out_w)) return rc;
    if (d->ksize_x < 1 || d->ksize_x > ISR_RESAMPLE_MAX_KSIZE || d->ksize_y < 1 || d->ksize_y > ISR_RESAMPLE_MAX_KSIZE)
        return fail(ISR_ERR_UNSUPPORTED, "resample_u8: ksize %d / %d outside [1, %d]", d->ksize_x, d->ksize_y,
                    ISR_RESAMPLE_MAX_KSIZE);
    if (d->hr_f32 && (d->in_h % d->out_h || d->in_w % d->out_w))
        return fail(ISR_ERR_UNSUPPORTED, "resample_u8: hr_f32 needs an integer ratio on both axes, got %dx%d -> %dx%d",
                    d->in_h, d->in_w, d->out_h, d->out_w);
    if (int rc = batch_ok("resample_u8", d->n, d->in_h, d->in_w, true)) return rc;
    if (int rc = batch_ok("resample_u8", d->n, d->out_h, d->out_w, true)) return rc;
    if (d->dst_u8 == d->src) return fail(ISR_ERR_BAD_DESC, "resample_u8: dst_u8 must not be src");
    if (!(aligned(4, {d->src, d->dst_u8, d->bounds_x, d->coeffs_x, d->bounds_y, d->coeffs_y, d->filter_id}) &&
          aligned(16, {d->lr_f32, d->hr_f32})))
        return fail(ISR_ERR_BAD_DESC, "resample_u8: src, dst_u8, tables and filter_id must be 4-byte aligned, lr_f32 "
                    "and hr_f32 16-byte aligned");
    if (d->lr_f32 || (d->hr_f32 && d->hr_norm))
        for (int c = 0; c < 3; ++c)
            if (!(d->std[c] != 0.f)) return fail(ISR_ERR_BAD_DESC, "resample_u8: std[%d] is zero", c);
    return grid_launched(isr::resample_u8_dispatch(d, (hipStream_t)s), "resample_u8");
}

int isr_blur_taps(int kind, int ksize, const double* params, int32_t* taps) {
    if (!taps) return fail(ISR_ERR_BAD_DESC, "blur_taps: null table");
    if (!params && (kind == ISR_BLUR_GAUSSIAN || kind == ISR_BLUR_MOTION))
        return fail(ISR_ERR_BAD_DESC, "blur_taps: kind %d needs params", kind);
    switch (isr::blur_taps(kind, ksize, params, taps)) {
        case 0: g_err[0] = 0; return ISR_OK;
        case 1: return fail(ISR_ERR_UNSUPPORTED, "blur_taps: unknown kind %d (ISR_BLUR_BOX, GAUSSIAN, MOTION = 0..2)", kind);
        case 2: return fail(ISR_ERR_UNSUPPORTED, "blur_taps: ksize %d is not 3, 5 or 7", ksize);
        case 3: return fail(ISR_ERR_UNSUPPORTED, "blur_taps: sigma_x, sigma_y and angle must be finite");
        case 4: return fail(ISR_ERR_UNSUPPORTED, "blur_taps: motion end points (%g, %g) (%g, %g) must be integers in "
                            "[0, %d]", params[0], params[1], params[2], params[3], ksize - 1);
        case 5: return fail(ISR_ERR_UNSUPPORTED, "blur_taps: motion end points are equal (%g, %g)", params[0], params[1]);
        default: return fail(ISR_ERR_UNSUPPORTED, "blur_taps: the centre tap would be negative (kind %d, ksize %d)", kind,
                             ksize);
    }
}

int isr_blur_u8(const isr_blur_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "blur_u8: null descriptor");
    if (!d->src || !d->dst || !d->ksize || !d->median || !d->taps)
        return fail(ISR_ERR_BAD_DESC, "blur_u8: null src / dst / ksize / median / taps");
    if (int rc = batch_ok("blur_u8", d->n, d->h, d->w, true, ISR_BLUR_MAX_K)) return rc;  // the k x k window
    if (d->dst == d->src) return fail(ISR_ERR_BAD_DESC, "blur_u8: dst must not be src");
    if (!aligned(4, {d->ksize, d->median, d->taps}))
        return fail(ISR_ERR_BAD_DESC, "blur_u8: ksize, median and taps must be 4-byte aligned");
    return grid_launched(isr::blur_u8_dispatch(d, (hipStream_t)s), "blur_u8");
}

int isr_yuv_coeffs(int matrix, int full_range, int32_t* fwd, int32_t* inv) {
    if (!fwd || !inv) return fail(ISR_ERR_BAD_DESC, "yuv_coeffs: null fwd / inv");
    if (isr::yuv_coeffs(matrix, full_range, fwd, inv))
        return fail(ISR_ERR_UNSUPPORTED, "yuv_coeffs: unknown matrix %d (ISR_YUV_BT601, BT709 = 0, 1)", matrix);
    g_err[0] = 0;
    return ISR_OK;
}

int isr_yuv420_to_rgb_u8(const isr_yuv_desc* d, isr_stream_t s) {
    if (int rc = yuv420_ok("yuv420_to_rgb_u8", d)) return rc;
    return launched(isr::yuv_dispatch(d, 1, (hipStream_t)s), "yuv420_to_rgb_u8");
}

int isr_rgb_to_yuv420_u8(const isr_yuv_desc* d, isr_stream_t s) {
    if (int rc = yuv420_ok("rgb_to_yuv420_u8", d)) return rc;
    return launched(isr::yuv_dispatch(d, 0, (hipStream_t)s), "rgb_to_yuv420_u8");
}

int isr_yuv_coeffs_depth(int matrix, int full_range, int depth, int32_t* fwd, int32_t* inv) {
    if (!fwd || !inv) return fail(ISR_ERR_BAD_DESC, "yuv_coeffs_depth: null fwd / inv");
    switch (isr::yuv_coeffs_depth(matrix, full_range, depth, fwd, inv)) {
        case 0: break;
        case 1: return fail(ISR_ERR_UNSUPPORTED, "yuv_coeffs_depth: unknown matrix %d (ISR_YUV_BT601, BT709 = 0, 1)", matrix);
        default: return fail(ISR_ERR_UNSUPPORTED, "yuv_coeffs_depth: depth %d (8 or 10)", depth);
    }
    g_err[0] = 0;
    return ISR_OK;
}

static int yuv16_ok(const char* what, const isr_yuv16_desc* d, int to_rgb) {
    if (int rc = yuv420_ok(what, d)) return rc;
    if (d->depth != 10) return fail(ISR_ERR_UNSUPPORTED, "%s: depth %d (10 only)", what, d->depth);
    if (d->shift < 0 || d->shift + d->depth > 16)
        return fail(ISR_ERR_UNSUPPORTED, "%s: shift %d + depth %d does not fit a 16-bit word", what, d->shift, d->depth);
    if (d->rgb_kind != ISR_RGB_U16 && d->rgb_kind != ISR_RGB_NORM_F32 && d->rgb_kind != ISR_RGB_TANH_F32)
        return fail(ISR_ERR_UNSUPPORTED, "%s: unknown rgb_kind %d (ISR_RGB_U16, NORM_F32, TANH_F32 = 0, 1, 2)", what,
                    d->rgb_kind);
    if (d->rgb_kind == (to_rgb ? ISR_RGB_TANH_F32 : ISR_RGB_NORM_F32))
        return fail(ISR_ERR_UNSUPPORTED, "%s: rgb_kind %d belongs to the other direction (%s)", what, d->rgb_kind,
                    to_rgb ? "ISR_RGB_TANH_F32 is an input of rgb_to_yuv420_16" : "ISR_RGB_NORM_F32 is an output of yuv420_to_rgb_16");
    const void* frames = to_rgb ? d->src : (const void*)d->dst;
    const void* rgb = to_rgb ? (const void*)d->dst : d->src;
    if (!aligned(2, {frames})) return fail(ISR_ERR_BAD_DESC, "%s: frames of 16-bit words must be 2-byte aligned", what);
    if (!aligned(d->rgb_kind == ISR_RGB_U16 ? 2 : 4, {rgb}))
        return fail(ISR_ERR_BAD_DESC, "%s: the RGB side must be %s", what,
                    d->rgb_kind == ISR_RGB_U16 ? "2-byte aligned (uint16)" : "4-byte aligned (fp32)");
    return ISR_OK;
}

int isr_yuv420_to_rgb_16(const isr_yuv16_desc* d, isr_stream_t s) {
    if (int rc = yuv16_ok("yuv420_to_rgb_16", d, 1)) return rc;
    return launched(isr::yuv16_dispatch(d, 1, (hipStream_t)s), "yuv420_to_rgb_16");
}

int isr_rgb_to_yuv420_16(const isr_yuv16_desc* d, isr_stream_t s) {
    if (int rc = yuv16_ok("rgb_to_yuv420_16", d, 0)) return rc;
    return launched(isr::yuv16_dispatch(d, 0, (hipStream_t)s), "rgb_to_yuv420_16");
}

// ---- dihedral transforms ----
// The shape rule of the three entry points: n in [1, max_n], c in [1, 65535], h, w >= 1, one plane below 2^31
// elements (a tile's coordinates are ints).
static int dihedral_shape_ok(const char* what, int n, int max_n, int c, int h, int w) {
    if (n < 1 || n > max_n) return fail(ISR_ERR_BAD_DESC, "%s: bad batch n=%d (n in [1, %d])", what, n, max_n);
    if (c < 1 || c > 65535) return fail(ISR_ERR_BAD_DESC, "%s: bad channel count c=%d (c in [1, 65535])", what, c);
    if (h < 1 || w < 1) return fail(ISR_ERR_BAD_DESC, "%s: image %dx%d smaller than 1 x 1", what, h, w);
    if ((long long)h * w >= (1ll << 31))
        return fail(ISR_ERR_UNSUPPORTED, "%s: a plane of h*w = %lld does not fit 31 bits (%dx%d)", what, (long long)h * w,
                    h, w);
    return ISR_OK;
}

int isr_dihedral_inverse(int op) {
    if (op < 0 || op > 7) return fail(ISR_ERR_BAD_DESC, "dihedral_inverse: op %d is not in 0..7", op);
    return isr::dihedral_inverse(op);
}

int isr_dihedral(const isr_dihedral_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "dihedral: null descriptor");
    if (!d->x || !d->y) return fail(ISR_ERR_BAD_DESC, "dihedral: null x / y");
    if (d->x == d->y) return fail(ISR_ERR_BAD_DESC, "dihedral: y must not be x");
    if (d->elem != 1 && d->elem != 4) return fail(ISR_ERR_UNSUPPORTED, "dihedral: elem %d is not 1 or 4 bytes", d->elem);
    if (!aligned(d->elem, {d->x, d->y}) || !aligned(4, {d->ops}))
        return fail(ISR_ERR_BAD_DESC, "dihedral: x and y must be aligned to elem = %d bytes, ops 4-byte aligned", d->elem);
    if (int rc = dihedral_shape_ok("dihedral", d->n, 65535, d->c, d->h, d->w)) return rc;
    if (d->ops && d->h != d->w)
        return fail(ISR_ERR_UNSUPPORTED, "dihedral: per-image ops need square images (h == w), not %dx%d", d->h, d->w);
    if (!d->ops && (d->op < 0 || d->op > 7)) return fail(ISR_ERR_UNSUPPORTED, "dihedral: op %d is not in 0..7", d->op);
    return grid_launched(isr::dihedral_dispatch(d, (hipStream_t)s), "dihedral");
}

int isr_ensemble_expand_u8(const isr_ensemble_expand_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "ensemble_expand_u8: null descriptor");
    if (!d->x || !d->even || !d->odd) return fail(ISR_ERR_BAD_DESC, "ensemble_expand_u8: null x / even / odd");
    if (d->x == d->even || d->x == d->odd || d->even == d->odd)
        return fail(ISR_ERR_BAD_DESC, "ensemble_expand_u8: x, even and odd must not be the same buffer");
    if (int rc = dihedral_shape_ok("ensemble_expand_u8", d->n, 16383, 3, d->h, d->w)) return rc;
    return grid_launched(isr::ensemble_expand_u8_dispatch(d, (hipStream_t)s), "ensemble_expand_u8");
}

int isr_ensemble_reduce(const isr_ensemble_reduce_desc* d, isr_stream_t s) {
    if (!d) return fail(ISR_ERR_BAD_DESC, "ensemble_reduce: null descriptor");
    if (!d->even || !d->odd || !d->y) return fail(ISR_ERR_BAD_DESC, "ensemble_reduce: null even / odd / y");
    if (d->y == (const void*)d->even || d->y == (const void*)d->odd || d->even == d->odd)
        return fail(ISR_ERR_BAD_DESC, "ensemble_reduce: even, odd and y must not be the same buffer");
    if (!aligned(4, {d->even, d->odd}) || !aligned(d->y_u8 ? 1 : 4, {d->y}))
        return fail(ISR_ERR_BAD_DESC, "ensemble_reduce: even, odd and an fp32 y must be 4-byte aligned");
    if (int rc = dihedral_shape_ok("ensemble_reduce", d->n, 16383, 3, d->h, d->w)) return rc;
    return grid_launched(isr::ensemble_reduce_dispatch(d, (hipStream_t)s), "ensemble_reduce");
}

}  // extern "C"
