/*
 * isr.h — C-ABI of libisr.so, the MI355X (gfx950) kernels behind the
 * image_super_resolution_amd drop-in.
 *
 * The reference (thnak/image_super_resolution) has no FFI/plugin layer: its hot
 * path is torch.nn modules dispatching to ATen convolutions.  Each entry point
 * below replaces one group of those module forwards (cited per function,
 * paths relative to the reference root).  A host binds these with ctypes (see
 * INTEGRATION.md); no torch types cross this boundary.
 *
 * Conventions
 *  - Activations are channel-blocked 2-byte floats ("NC16HW16c": bf16, or fp16 on the
 *    forward descriptors with f16 = 1, the inference default since round 6) in caller-owned device
 *    buffers laid out as [N][cs/16][hp][wp][16] with a zero border of `pad`
 *    pixels on every side: each 16-channel block is a contiguous plane, so a
 *    K-chunk of a convolution reads whole cache lines.  The caller zero-fills a
 *    buffer once; kernels never write the border and write exact zeros at
 *    computed positions outside the valid h x w region, so the border /
 *    alignment slack always reads as the conv's zero padding.
 *  - Computed regions are tile-aligned: ha % ISR_TILE_H == 0, wa % ISR_TILE_W == 0.
 *  - The library never allocates, frees or synchronises; every call takes an
 *    explicit stream and is hipGraph-capturable.
 *  - Return 0 on success, a negative ISR_ERR_* otherwise; isr_last_error()
 *    returns a thread-local message for the last failure.
 */
#ifndef ISR_H
#define ISR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* isr_stream_t; /* == hipStream_t */

#define ISR_OK 0
#define ISR_ERR_BAD_DESC (-1)
#define ISR_ERR_UNSUPPORTED (-2)
#define ISR_ERR_LAUNCH (-3)

#define ISR_TILE_H 32
#define ISR_TILE_W 32

/* A channel slice [coff, coff + k) of a channel-blocked bf16 / fp16 buffer
 * [N][cs/16][hp][wp][16] with border `pad` (cs, coff multiples of 16).
 * Interior pixel (n, y, x), view channel c (ch = coff + c) lives at
 *   data + ((((n*(cs/16) + ch/16)*hp + y + pad)*wp + x + pad)*16 + ch%16) * 2 bytes. */
typedef struct isr_view {
    void* data;
    int32_t hp, wp, cs, pad, coff;
} isr_view;

/* 3x3 stride-1 'same' convolution with fused epilogue:
 *   v = act(conv(x, W) + bias);  v = v*s1 + r1 (if r1);  v = v*s2 + r2 (if r2)
 *   store v to y (PixelShuffle(2)-permuted when shuffle == 2) and to y2 (if set).
 * act is LeakyReLU(slope) (slope = 1 → identity, 0 → ReLU).
 * Replaces: Conv._forward_impl (utils/models.py:97-98, BN folded by
 * fuse_conv_and_bn :366-406), ConvWithoutBN._forward_impl (:195-196),
 * the torch.cat chain + residual of RDB.forward (:265-271; the caller points
 * y at a channel slice of the dense-block buffer), RRDB.forward (:316-317, as
 * r2), ResNet/EResNet trunk add (:615, :647) and Scaler (:572-589: conv →
 * PixelShuffle(2) → LeakyReLU via shuffle == 2). */
typedef struct isr_conv_desc {
    int32_t n, h, w;   /* batch; valid conv height/width (input == output size) */
    int32_t ha, wa;    /* computed (tile-aligned) extent; ha % 32 == 0, wa % 32 == 0 */
    int32_t cin, cout; /* cin % 16 == 0; cout % 32 == 0 (cout % 64 != 0 runs 32-cout tiles) */
    isr_view x;        /* input (cin channels from x.coff) */
    isr_view y;        /* output; for shuffle == 2 its grid is (2h, 2w), cout/4 channels */
    isr_view y2;       /* optional duplicate output (y2.data == NULL → none) */
    isr_view r1, r2;   /* optional residuals (data == NULL → none), cout channels */
    const void* wpack; /* from isr_pack_conv3x3 */
    const float* bias; /* [cout] fp32 or NULL */
    float slope, s1, s2; /* s2 multiplies after r1 even without r2: set 1.0 when unused */
    int32_t shuffle;   /* 1 = plain store, 2 = PixelShuffle(2) store */
    /* Backward-pass extensions (all zero in the forward).  The epilogue order is
     * v = act(acc + bias); v = v*s1 + r1; v = v*s2 + r2; v *= mask; store.
     * Used by the generator backward (utils/models.py forward graph, autograd
     * of train.py:57 / :102): input-gradient convs accumulate into the dense-block
     * gradient buffer and apply LeakyReLU' of the forward activation. */
    isr_view m;        /* optional mask source (data == NULL → none), same grid as y */
    float mslope;      /* output channel c >= m_c0 is multiplied by (m[c] > 0 ? 1 : mslope); with shuffle == 2
                          m is on the shuffled grid and masks every channel (m_c0 = 0) */
    int32_t m_c0;      /* first masked output channel, multiple of 32 */
    int32_t r1_cn;     /* r1 is added only to output channels < r1_cn (0 → all); multiple of 32 */
    int32_t x_sub2;    /* 1: input channel c' = s*(cin/4) + c reads x at pixel (2y + (s>>1), 2x + (s&1)),
                          channel c (x is on the 2h x 2w grid, pad >= 2): the transpose of
                          PixelShuffle(2) (utils/models.py:583) folded into the load; cin % 128 == 0 */
    int32_t taps;      /* 0: all 3x3 taps; 1: only taps {0,1}^2; 2: only taps {1,2}^2 (cout % 64 == 0).
                          A stride-2 3x3 conv (Discriminator, utils/models.py:533-542) is taps=1 over the
                          x_sub2 view with 4*cin phase-expanded weights; its input gradient is taps=2
                          over the output gradient with shuffle == 2 (4*cin phase outputs). */
    int32_t f16;       /* 0: activations (x, y, y2, r1, r2) and wpack are bf16; 1: fp16 (the inference
                          path: 10 mantissa bits instead of 7, the storage type of the reference's own
                          fp16 autocast, train.py:54 / rs.py), wpack from isr_pack_conv3x3_f16.  fp16 is
                          forward-only: m.data == NULL, x_sub2 == 0, taps == 0. */
} isr_conv_desc;

/* 9x9 head conv, 3 → cout (=64) channels, input NCHW (fp32 already normalised,
 * or uint8 with Normalize fused), + bias + LeakyReLU(slope), NHWC bf16 out.
 * Replaces: ResNet.conv0 / EResNet.conv0 (utils/models.py:596, :625) and the
 * Normalize of Model.init_normalize (:731-732; utils/datasets.py:65-71). */
typedef struct isr_head_desc {
    int32_t n, h, w, ha, wa;
    int32_t cout;          /* 64 */
    const void* x;         /* NCHW [n][3][h][w] */
    int32_t x_u8;          /* 0: fp32 input used as is; 1: uint8, (v/255 - mean)/std fused */
    float mean[3], inv_std[3];
    isr_view y, y2;
    const void* wpack;     /* from isr_pack_head9x9 */
    const float* bias;     /* [cout] or NULL */
    float slope;
    /* backward use (zero in the forward): with fp32 input, mean 0, inv_std 1,
     * slope 1 and 180°-rotated, transposed weights this is the input gradient of
     * the 9x9 tail conv (utils/models.py:607, :636); m masks it with
     * LeakyReLU'(m) of slope mslope (the last Scaler's activation). */
    isr_view m;
    float mslope;
    int32_t f16;           /* 1: y / y2 fp16 and wpack from isr_pack_head9x9_f16 (forward only, m.data == NULL) */
} isr_head_desc;

/* 9x9 tail conv, cin (=64) → 3 channels, + bias + tanh, NCHW out (fp32, or
 * uint8 with TanhToArrayImage fused: round_half_even((t+1)/2*255)).
 * Replaces: ResNet.conv2 / EResNet.conv2 (utils/models.py:607, :636) and
 * TanhToArrayImage.forward (:448-451). */
typedef struct isr_tail_desc {
    int32_t n, h, w, ha, wa; /* valid / computed extent of the tail (= output size) */
    int32_t cin;             /* 64 */
    isr_view x;              /* NHWC bf16, pad >= 4 */
    const void* wpack;       /* from isr_pack_tail9x9 */
    const float* bias;       /* [3] or NULL */
    void* y;                 /* NCHW [n][3][h][w] */
    int32_t y_u8;            /* 0: fp32 tanh output; 1: uint8 image */
    int32_t f16;             /* 1: x fp16 and wpack from isr_pack_tail9x9_f16 */
} isr_tail_desc;

/* Weight / bias gradient of a 3x3 'same' conv (the bwd-weight half of autograd
 * through Conv / ConvWithoutBN / RDB / Scaler, utils/models.py:75-111, 174-199,
 * 245-271, 572-589, driven by train.py:57 / :102):
 *   dw[co][ci][ky][kx] = scale * sum_{n,y,x} g[n][co][y][x] * x[n][ci][y+ky-1][x+kx-1]
 *   db[co]             = scale * sum_{n,y,x} g[n][co][y][x]
 * g must be zero outside the valid h x w region (every isr kernel writes zeros there).
 * Needs a caller-owned workspace of isr_wgrad3x3_workspace_bytes(desc) bytes
 * (split-K partial sums); dw / db are overwritten. */
typedef struct isr_wgrad_desc {
    int32_t n, h, w, ha, wa; /* conv output grid (= input grid) */
    int32_t cin, cout;       /* multiples of 32 */
    isr_view x;              /* forward input, cin channels, pad >= 1 */
    isr_view g;              /* gradient w.r.t. the conv output, cout channels */
    int32_t g_sub2;          /* 1: g is the PixelShuffle(2)'d gradient on the 2h x 2w grid with cout/4
                                channels (Scaler, utils/models.py:583); cout % 128 == 0 */
    float scale;
    float* dw;               /* [cout][cin][3][3] fp32 */
    float* db;               /* [cout] fp32 or NULL */
    int32_t splits;          /* split-K count; 0 = library choice */
    int32_t x_sub2;          /* 1: x is read as PixelShuffle(2)^T of a 2h x 2w buffer (pad >= 2): kernel input
                                channel s*(cin/4) + c = x[c] at (2y + (s>>1), 2x + (s&1)); cin % 128 == 0.
                                With taps == 1 this is the weight gradient of a stride-2 conv (Discriminator,
                                utils/models.py:533-542) on its phase decomposition. */
    int32_t taps;            /* 0: all 3x3 taps; 1: only taps {0,1}^2 (dw at other taps left undefined) */
} isr_wgrad_desc;

/* Weight / bias gradients of the 9x9 convs (same workspace contract):
 *   head = 1: conv0 3 → 64 (utils/models.py:596, :625): p = the (normalised)
 *             network input, q = gradient wrt conv0's pre-activation output;
 *             dw [64][3][9][9], db [64].
 *   head = 0: conv2 64 → 3 (utils/models.py:607, :636): p = gradient wrt
 *             conv2's pre-tanh output, q = conv2's input (pad >= 4);
 *             dw [3][64][9][9], db [3].
 * dw[co][ci][ky][kx] = scale * sum_{n,y,x} gout[co][y][x] * in[ci][y+ky-4][x+kx-4]. */
typedef struct isr_wgrad9_desc {
    int32_t n, h, w, ha, wa;
    int32_t head;
    const float* p;          /* NCHW fp32 [n][3][h][w] */
    isr_view q;              /* 64 channels, zero outside h x w */
    float scale;
    float* dw;
    float* db;               /* or NULL */
    int32_t splits;          /* 0 = library choice */
} isr_wgrad9_desc;

size_t isr_wgrad9x9_workspace_bytes(const isr_wgrad9_desc* d);
int isr_wgrad9x9(const isr_wgrad9_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s);

size_t isr_wgrad3x3_workspace_bytes(const isr_wgrad_desc* d);
int isr_wgrad3x3(const isr_wgrad_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s);
/* isr_wgrad3x3 in two launches: the split-K partial sums into `workspace`, then their reduction
 * into dw / db (same descriptor and workspace; the caller orders the second after the first, on
 * another stream too, and keeps the workspace untouched in between).  Lets a caller take the
 * reductions off the stream that chains the weight-gradient kernels (train_engine.py). */
/* Up to 5 weight gradients over one pixel grid in one launch (plus one reduce launch): the 5 convs
 * of an RDB (utils/models.py:265-271) read one dense buffer and one gradient buffer; their (co, ci)
 * tile pairs share one grid, so ~5x fewer split-K partials fill the chip.  Members: plain 3x3
 * (g_sub2 = x_sub2 = taps = 0), cin / cout multiples of 32, the same n / ha / wa; `splits` is
 * ignored.  Each member's dw / db / scale as in isr_wgrad3x3; one workspace of
 * isr_wgrad3x3_group_workspace_bytes(descs, n) bytes. */
size_t isr_wgrad3x3_group_workspace_bytes(const isr_wgrad_desc* descs, int32_t n);
int isr_wgrad3x3_group(const isr_wgrad_desc* descs, int32_t n, void* workspace, size_t ws_bytes, isr_stream_t s);
/* The grouped launch by an explicit form: 0 = production (isr_wgrad3x3_group: asm transposing
 * LDS reads with counted waits), 1 = the same tiles and splits with compiler-visible LDS reads
 * (the bit-identical reference the production form is tested against); same workspace size. */
int isr_wgrad3x3_group_variant(const isr_wgrad_desc* descs, int32_t n, int32_t variant, void* workspace,
                               size_t ws_bytes, isr_stream_t s);
int isr_wgrad3x3_partials(const isr_wgrad_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s);
int isr_wgrad3x3_reduce(const isr_wgrad_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s);
/* The same computation by an explicit kernel variant, with its own workspace size: 0 = production
 * (isr_wgrad3x3), 16 = the production tiles and split counts with compiler-visible LDS reads (the
 * bit-identical reference of the asm-read forms); 1..15 = earlier tile forms, in tuning builds only
 * (-DISR_TUNING; a production library returns ISR_ERR_UNSUPPORTED / 0 bytes for them). */
size_t isr_wgrad3x3_variant_workspace_bytes(const isr_wgrad_desc* d, int32_t variant);
int isr_wgrad3x3_variant(const isr_wgrad_desc* d, int32_t variant, void* workspace, size_t ws_bytes, isr_stream_t s);

/* Elementwise combine on channel-blocked views (backward glue):
 *   y = (a*sa + b*sb) * (m > 0 ? 1 : mslope)   over c channels; b, m optional;
 * y is zero outside the valid h x w region.  Replaces the autograd sum at the
 * generator trunk (utils/models.py:615, :647: inputs + conv1(residual(inputs)))
 * and conv0's LeakyReLU backward. */
typedef struct isr_ew_desc {
    int32_t n, h, w, ha, wa, c;
    isr_view y, a, b, m;
    float sa, sb, mslope;
} isr_ew_desc;
int isr_ew_combine(const isr_ew_desc* d, isr_stream_t s);

/* PixelShuffle(2) + LeakyReLU(mslope) between channel-blocked views (same descriptor):
 *   y[c] at (y, x) = act(sa * a[4c + 2*(y%2) + (x%2)] at (y/2, x/2)),  c < d->c
 * (n, h, w, ha, wa) is the OUTPUT grid (even); a holds 4c channels on the
 * (h/2) x (w/2) grid; b and m must be NULL.  Zeros outside the valid region.
 * Replaces: Denoise.residual_conv1 = Sequential(PixelShuffle(2), LeakyReLU(0.2))
 * (utils/models.py:687) applied to the output of a ResidualBlock1 (:202-209),
 * whose residual add precedes the shuffle so it cannot ride a conv epilogue. */
int isr_pixel_shuffle2(const isr_ew_desc* d, isr_stream_t s);
/* Its transpose, the PixelShuffle(2) input gradient (Denoise training, train.py:204-205):
 *   y[4c + s] at (y, x) = sa * a[c] at (2y + s/2, 2x + s%2) * (m there > 0 ? 1 : mslope)
 * (n, h, w, ha, wa) is the OUTPUT (half-resolution) grid, d->c its channel count
 * (multiple of 64); a and the optional LeakyReLU' mask source m hold c/4 channels on
 * the 2h x 2w grid (rows / cols up to 2ha / 2wa are read); b must be NULL. */
int isr_pixel_unshuffle2(const isr_ew_desc* d, isr_stream_t s);

/* Training-data transform of SR_dataset (utils/datasets.py:344-355) over a batch of uint8 HR
 * crops in ONE launch: lr = Normalize(cv2 INTER_LINEAR uint8 resize by `scale`, :302-304: at the
 * integer factors the block's centre pixel (odd) or its centre 2x2 mean rounded half up (even)),
 * hr = 2x/255 - 1 (PIL_to_tanh, :96-106) or Normalize(x) when hr_norm (SRGAN mode, :336-339).
 * crops [n][3][t][t] uint8, hr [n][3][t][t] fp32, lr [n][3][t/scale][t/scale] fp32, all
 * contiguous; scale in {2, 3, 4}, t % scale == 0; Normalize(v) = (v/255 - mean[c]) / std[c]. */
typedef struct isr_sr_transform_desc {
    const uint8_t* crops;
    float* hr;
    float* lr;
    int32_t n, t, scale, hr_norm;
    float mean[3], std[3];
} isr_sr_transform_desc;
int isr_sr_transform(const isr_sr_transform_desc* d, isr_stream_t s);

/* Layout conversion between NCHW fp32 tensors and channel-blocked views
 * (network / loss boundaries: the VGG19 input, utils/loss.py:16-24, and the
 * gradient it receives).  to_blocked writes channels [0, round16(c)) of v (zeros
 * past c and outside the valid region), v = x*scale[c] + shift[c] (NULL → 1 / 0),
 * then the optional LeakyReLU' mask m (ReLU' with mslope 0); to_nchw reads
 * channels [0, c) of v into nchw, applying scale/shift. */
typedef struct isr_convert_desc {
    int32_t n, h, w, ha, wa, c;
    void* nchw;
    isr_view v;
    const float* scale;
    const float* shift;
    isr_view m;
    float mslope;
} isr_convert_desc;
int isr_nchw_to_blocked(const isr_convert_desc* d, isr_stream_t s);
int isr_blocked_to_nchw(const isr_convert_desc* d, isr_stream_t s);

/* 2x2 stride-2 max pool (torchvision vgg19.features MaxPool2d, used by
 * TruncatedVGG19 utils/models.py:454-510).  Input grid h x w (even), output
 * (h/2) x (w/2) with computed region hao x wao (multiples of 32).
 * fwd: y = maxpool(x).  bwd: g (input grid) = y (output gradient) routed to the
 * first maximum of each window, times (x > 0 ? 1 : mslope). */
typedef struct isr_pool_desc {
    int32_t n, h, w, c, hao, wao;
    isr_view x, y, g;
    float mslope;
} isr_pool_desc;
int isr_maxpool2_fwd(const isr_pool_desc* d, isr_stream_t s);
int isr_maxpool2_bwd(const isr_pool_desc* d, isr_stream_t s);

/* Train-mode BatchNorm2d (the `bn` of Conv, utils/models.py:75-111, trained by
 * train.py with ResNet; nn.BatchNorm2d semantics: biased batch variance for the
 * normalisation, unbiased for running_var, momentum update), on channel-blocked
 * views of c channels.  Statistics accumulate in acc[2][c] (double, caller-zeroed
 * before each reduce); finalize writes save[2][c] = (mean, 1/sqrt(var + eps)).
 *   isr_bn_stats      acc += (sum z, sum z^2)
 *   isr_bn_finalize   save, running_mean / running_var update
 *   isr_bn_apply      y = ((LeakyReLU_slope(a z + b)) * s1 + r1) * s2 + r2,  a = gamma * invstd,
 *                     b = beta - mean * a  (r1 / r2 optional; zero outside the valid region)
 *   isr_bn_bwd_reduce acc += (sum g, sum g * xhat),  g = y view (gradient wrt the BN output)
 *   isr_bn_bwd_apply  dz = gscale * a * (g - mean(g) - xhat * mean(g xhat))  into dz (or over y when
 *                     dz.data == NULL); dgamma = gscale * sum(g xhat), dbeta = gscale * sum(g) */
typedef struct isr_bn_desc {
    int32_t n, h, w, ha, wa, c;
    isr_view z, y, r1, r2, dz;
    float s1, s2, slope;
    const float* gamma;
    const float* beta;
    float* running_mean;      /* NULL: no running-stat update */
    float* running_var;
    float momentum, eps;
    double* acc;
    float* save;
    float* dgamma;
    float* dbeta;
    float gscale;
} isr_bn_desc;
int isr_bn_stats(const isr_bn_desc* d, isr_stream_t s);
int isr_bn_finalize(const isr_bn_desc* d, isr_stream_t s);
int isr_bn_apply(const isr_bn_desc* d, isr_stream_t s);
int isr_bn_bwd_reduce(const isr_bn_desc* d, isr_stream_t s);
int isr_bn_bwd_apply(const isr_bn_desc* d, isr_stream_t s);

/* Weight packing (device fp32 OIHW → device bf16 kernel layout).  Replaces the
 * one-off fuse step's weight preparation (utils/models.py:741-751); BN folding
 * itself is done by the caller before packing. */
size_t isr_conv3x3_packed_bytes(int32_t cout, int32_t cin);
int isr_pack_conv3x3(const float* w_oihw, void* packed, int32_t cout, int32_t cin, isr_stream_t s);
/* Input-gradient (dgrad) packing of a layer's [cout][cin][3][3] weights: the
 * result is an isr_conv3x3_fwd weight set for the conv cout → cin with the
 * kernel rotated by 180° and multiplied by `scale` (isr_conv3x3_packed_bytes(cin,
 * cout) bytes).  sub2 = 1 orders its input channels for isr_conv_desc.x_sub2
 * (the Scaler backward, utils/models.py:583). */
int isr_pack_conv3x3_dgrad(const float* w_oihw, void* packed, int32_t cout, int32_t cin, float scale, int32_t sub2,
                           isr_stream_t s);
/* Many isr_pack_conv3x3 / isr_pack_conv3x3_dgrad in one launch (items: device array). */
typedef struct isr_pack_item {
    const float* w; /* layer weights [cout][cin][3][3] fp32 (dgrad with src_cin > 0: [cout][src_cin][3][3]) */
    void* out;      /* packed bf16, isr_conv3x3_packed_bytes(cout, cin) bytes */
    int32_t cout, cin;
    int32_t dgrad;  /* 0: forward pack; 1: dgrad pack (as isr_pack_conv3x3_dgrad) */
    int32_t sub2;
    float scale;
    /* dgrad window (0, 0 = the whole layer): pack only the layer's input channels
     * [src_n0, src_n0 + cin) of a layer with src_cin input channels, i.e. the slice of the
     * transposed conv that produces those channels.  `out` may point inside a larger pack: a
     * conv whose input concatenates several layers' output gradients (the RDB input-gradient
     * "gather" convs of the training backward) is packed as one item per input block, at
     * packed offset (block's first input channel / 16) * 9 * cin * 16 elements. */
    int32_t src_n0, src_cin;
    int32_t pad_;
} isr_pack_item;
int isr_pack_conv3x3_batch(const isr_pack_item* items, int32_t n, isr_stream_t s);
size_t isr_head9x9_packed_bytes(int32_t cout, int32_t cin);
int isr_pack_head9x9(const float* w_oihw, void* packed, int32_t cout, int32_t cin, isr_stream_t s);
size_t isr_tail9x9_packed_bytes(int32_t cout, int32_t cin);
int isr_pack_tail9x9(const float* w_oihw, void* packed, int32_t cout, int32_t cin, isr_stream_t s);
/* The same three packs in fp16 (same layouts and sizes), for descriptors with f16 = 1. */
int isr_pack_conv3x3_f16(const float* w_oihw, void* packed, int32_t cout, int32_t cin, isr_stream_t s);
int isr_pack_head9x9_f16(const float* w_oihw, void* packed, int32_t cout, int32_t cin, isr_stream_t s);
int isr_pack_tail9x9_f16(const float* w_oihw, void* packed, int32_t cout, int32_t cin, isr_stream_t s);

int isr_conv3x3_fwd(const isr_conv_desc* d, isr_stream_t s);
/* Tuning entry point: same contract as isr_conv3x3_fwd with an explicit kernel
 * variant (0 = the production choice).  The production library carries variant 0
 * only; the tile / pipeline alternatives (1-3, 8, 9) and the timing-only ablations
 * (4-7) exist in a library built with -DISR_TUNING (lib/libisr_tuning.so).  Every
 * non-ablation variant writes the same outputs as variant 0 (up to fp32 summation
 * order).  Returns ISR_ERR_UNSUPPORTED for a variant this library does not carry. */
int isr_conv3x3_fwd_variant(const isr_conv_desc* d, int32_t variant, isr_stream_t s);
/* Tuning builds (-DISR_TUNING) only: per-block wall-clock stamps of later conv3x3
 * launches into `buf` (8 x uint64 per block: entry, first chunk landed, main loop
 * done, epilogue done [s_memrealtime, 100 MHz], -, -, HW_ID, XCC_ID); NULL stops.
 * A default build returns ISR_ERR_UNSUPPORTED. */
int isr_tuning_conv_stamps(void* buf);
/* Kept for the ABI: no shipping tail kernel writes stamps (the 4-wave walk that did was removed,
 * DESIGN.md section 5).  Returns ISR_ERR_UNSUPPORTED in every build. */
int isr_tuning_tail_stamps(void* buf);
/* Kept for the ABI: the round-2 chain kernel that read these knobs was removed (DESIGN.md
 * section 5).  Returns ISR_ERR_UNSUPPORTED in every build. */
int isr_tuning_chain_knobs(int32_t delay_ticks, int32_t delay_shift, int32_t k2, int32_t k3);
/* Validation only: ISR_OK when isr_conv3x3_fwd would accept `d` (nothing launched). */
int isr_conv3x3_check(const isr_conv_desc* d);

/* The same 3x3 conv + fused epilogue by 1-D Winograd F(2,3) along x (fp16 inference, opt-in):
 * 4 MFMA products per output pair and kernel row instead of 6.  Per kernel row ky, input
 * channel c and output pair j (outputs x = 2j, 2j+1; inputs d0..d3 = x[2j-1 .. 2j+2]; taps
 * g0..g2 = W[co][c][ky][0..2]):
 *   V0 = d0 - d2   V1 = d1 + d2   V2 = d2 - d1   V3 = d1 - d3     (each rounded once to fp16)
 *   U0 = g0   U1 = (g0+g1+g2)/2   U2 = (g0-g1+g2)/2   U3 = g2     (fp32 from the fp32 weights,
 *                                                                  rounded once to fp16 at pack time)
 *   M_p = sum_{ky,c} U_p * V_p       (fp32 accumulation, one accumulator set per p = 0..3)
 *   y(2j) = M0 + M1 + M2             y(2j+1) = M1 - M2 - M3       (fp32)
 * followed by isr_conv3x3_fwd's epilogue in its order (v = act(y + bias); v = v*s1 + r1;
 * v = v*s2 + r2; store to y and y2, rounded once to fp16; exact zeros outside the valid region).
 * The result is NOT bit-identical to isr_conv3x3_fwd: the input transform rounds to fp16 and the
 * products differ.  Same descriptor and views; supported: f16 == 1, shuffle == 1, no mask,
 * x_sub2 == 0, taps == 0, cin % 16 == 0, cout % 32 == 0; bias, slope, r1 / s1 / r1_cn, r2 / s2
 * and y2 as in the direct form (r1 is always read in the epilogue); y may be a higher channel
 * slice of x's buffer (the in-place growth convs).  wpack is from isr_pack_conv3x3_wino_f16:
 * fp16 [cin/16][ky 3][p 4][cout][hpos 2][8], element U_p of W[n][c16*16 + h*8 + e][ky][0..2]
 * with h = hpos ^ ((n >> 3) & 1); isr_conv3x3_wino_packed_bytes = cout*cin*12*2 bytes. */
size_t isr_conv3x3_wino_packed_bytes(int32_t cout, int32_t cin);
int isr_pack_conv3x3_wino_f16(const float* w_oihw, void* packed, int32_t cout, int32_t cin, isr_stream_t s);
int isr_conv3x3_wino_fwd(const isr_conv_desc* d, isr_stream_t s);

/* Persistent chain of RDB convs (the RRDB trunk, utils/models.py:245-317) in ONE launch:
 * layer i is layers[i] (device memory), each a descriptor isr_conv3x3_check accepts, of
 * kind kinds[i]: 0 = growth conv (cout 32), 1 = RDB final conv (cin 192, cout 64); all
 * layers share n, ha, wa (plain 3x3, no x_sub2 / taps / shuffle / mask).  Replaces nl
 * isr_conv3x3_fwd calls with the same outputs.  Tiles of layer i start as soon as their
 * 3x3 tile neighbourhood of layer i-1 is done (tile-level dependencies, no grid barrier).
 * `state` (device, isr_conv_chain_state_words(n, ha, wa) uint32 words, zeroed ONCE by the
 * caller before first use, then owned by the library across calls: a generation counter in
 * state[0] replaces per-call zeroing); after a call, state[1] == state[0] means a dependency
 * wait gave up (results invalid — not expected unless the device is shared); state[2] is a
 * sticky give-up counter that only grows (never reset): ANY change since the last value a host
 * saw means a launch in between gave up (one add per giving-up wave or refused launch, so it
 * is not a count of failed launches); state[3] belongs to the host (the library never writes it:
 * isr_mt_adam_guarded / isr_mt_lerp_guarded compare it with state[2]).  1 <= nl <= 1024.
 * acquire = 1 adds an agent-scope acquire before each tile's loads (otherwise the
 * hand-off relies on sc1 loads). */
typedef struct isr_chain_desc {
    const isr_conv_desc* layers;
    const int32_t* kinds;
    int32_t nl;
    int32_t n, ha, wa;
    uint32_t* state;
    int32_t acquire;
    int32_t f16;    /* every layer's isr_conv_desc.f16 (the table lives in device memory): 1 = fp16 */
} isr_chain_desc;
size_t isr_conv_chain_state_words(int32_t n, int32_t ha, int32_t wa);
int isr_conv_chain(const isr_chain_desc* c, isr_stream_t s);
/* The same with a variant id.  Only 0 exists: trunk.hip, two 4-wave workgroups per CU (4 output
 * rows per wave, one K-chunk in flight), one continuous K-chunk stream per workgroup across its
 * (layer, tile) items, waits only before the chunks the previous layer wrote, the RDB residual
 * folded into the MFMAs.  It needs every view to share (hp, wp, cs, pad), a bias, cin >= 64, and
 * r1 (if any) == the layer's own input with slope 1 and 1/s1 exact in the storage type (bf16, or
 * fp16 with f16); a table that breaks this makes the launch give up: state[1] == state[0].  It
 * produces the outputs of the per-layer isr_conv3x3_fwd calls bit for bit.  Every other id (1-9
 * were A/B forms that measured slower) returns ISR_ERR_UNSUPPORTED in every build; DESIGN.md
 * section 5 keeps their history. */
int isr_conv_chain_variant(const isr_chain_desc* c, int32_t variant, isr_stream_t s);
/* Tuning builds only: per (layer 75..89, tile) stamps of later production chain launches into
 * `buf` (8 x uint64: entry, chunk 0 landed, main loop done, stores issued, deferred wait start,
 * wait met; s_memrealtime ticks, 100 MHz); NULL stops. */
int isr_tuning_trunk_stamps(void* buf);
/* Tuning builds only: ablations of later production chain launches (timing only, outputs wrong):
 * bit 1 = no halo LDS-DMA, 4 = no epilogue stores, 8 = no weight LDS-DMA, 16 = no dependency
 * waits;
 * per_cu > 0 caps the resident workgroups per CU (the grid). */
int isr_tuning_trunk_knobs(int32_t ablate, int32_t per_cu, int32_t k2, int32_t k3);
/* Tuning builds only: per-item cycle stamps (s_memtime) of later production chain launches into
 * `buf` (uint64 [grid][2 layers: 77, 79][16 items][2 waves][8]: item top, own DMA landed, barrier
 * passed, refill issued, MFMAs issued) for each workgroup's first tile; NULL stops. */
int isr_tuning_trunk_item_stamps(void* buf);

int isr_head9x9_fwd(const isr_head_desc* d, isr_stream_t s);
int isr_tail9x9_fwd(const isr_tail_desc* d, isr_stream_t s);
/* The same with the kernel chosen: 0 = production (= 5), 5 = row-streaming walk down a 32-column
 * strip with 8 waves (two per SIMD, each T row computed once), 3 = one 8-row tile per block (76 KB
 * LDS, 2 blocks / CU; the fallback for outputs past 2 GiB).  Bit-identical.  Every other id (A/B
 * forms that measured slower) returns ISR_ERR_UNSUPPORTED in every build; DESIGN.md section 5
 * keeps their history.  Same descriptor rules as isr_tail9x9_fwd. */
int isr_tail9x9_fwd_variant(const isr_tail_desc* d, int32_t variant, isr_stream_t s);
/* What isr_tail9x9_fwd would run for `d` on a device of `cus` compute units (cus <= 0: the current
 * device's): the walk's segment height in rows, 8 .. 512, a power of two — 512 halved while it does
 * not divide ha or while n * (wa / 32) * (ha / rows) < cus — or 0 when the per-tile kernel is taken
 * because the output of one image reaches 2 GiB (3 * h * w * element size >= 2^31).  Same descriptor
 * rules as isr_tail9x9_fwd: a negative ISR_ERR_* with isr_last_error() set on a bad descriptor.
 * Launches nothing and follows no pointer of the descriptor. */
int32_t isr_tail9x9_segment_rows(const isr_tail_desc* d, int32_t cus);

/* ---- multi-tensor optimiser ops (one launch over every parameter) ---------
 * A tensor is n fp32 elements at each non-null pointer (same element order);
 * a chunk is elements [start, start + len) of tensor t.  The host builds the
 * tensor and chunk tables in device memory (len <= 65536 recommended).
 * Replaces: torch.optim.Adam.step (train.py:264-267, stepped at :58/:102/:118),
 * clip_grad_norm_(params, 10) (train.py:57, :101, :116), ModelEMA.update
 * (utils/models.py:31-40). */
typedef struct isr_mt_tensor {
    float* p; /* param (Adam), EMA tensor (lerp) */
    float* g; /* grad (Adam, sumsq, scale), model tensor (lerp) */
    float* m; /* exp_avg */
    float* v; /* exp_avg_sq */
    int64_t n;
} isr_mt_tensor;

typedef struct isr_mt_chunk {
    int32_t t, len;
    int64_t start;
} isr_mt_chunk;

/* torch.optim.Adam (amsgrad=False, maximize=False): g' = g*scale (+ wd*p);
 * m = lerp(m, g', 1-beta1); v = beta2*v + (1-beta2)*g'^2;
 * p += step * m / (sqrt(v)/bc2_sqrt + eps), step = -lr/(1-beta1^t), bc2_sqrt = sqrt(1-beta2^t). */
typedef struct isr_adam_args {
    float step, beta1, beta2, eps, weight_decay, bc2_sqrt;
} isr_adam_args;

/* `scale` (device, nullable): gradient multiplier applied on the fly (e.g. a clip coefficient). */
int isr_mt_adam(const isr_mt_tensor* tensors, const isr_mt_chunk* chunks, int32_t nchunks, const isr_adam_args* a,
                const float* scale, isr_stream_t s);
/* partial[k] = sum of g^2 over chunk k. */
int isr_mt_sumsq(const isr_mt_tensor* tensors, const isr_mt_chunk* chunks, int32_t nchunks, float* partial,
                 isr_stream_t s);
/* out[0] = sqrt(sum partial), out[1] = max_norm / (out[0] + 1e-6) clamped to at most 1 — clip_grad_norm_'s
 * coefficient.  A NaN norm gives a NaN coefficient, as torch.clamp(coef, max=1.0) does. */
int isr_clip_coef(const float* partial, int32_t n, float max_norm, float* out, isr_stream_t s);
/* g *= *coef over every chunk (clip_grad_norm_'s in-place scaling). */
int isr_mt_scale(const isr_mt_tensor* tensors, const isr_mt_chunk* chunks, int32_t nchunks, const float* coef,
                 isr_stream_t s);
/* p = p*d + (1-d)*g over every chunk (ModelEMA.update: p = EMA tensor, g = model tensor). */
int isr_mt_lerp(const isr_mt_tensor* tensors, const isr_mt_chunk* chunks, int32_t nchunks, float d, isr_stream_t s);
/* The same two updates, skipped on the device (no host synchronisation) when guard[0] != guard[1]:
 * pass `isr_chain_desc.state + 2` of the trunk launch that produced this step's forward (state[2]
 * the sticky give-up counter, state[3] the count the host has accepted, zero-initialised with the
 * state), so a forward whose dependency wait gave up never reaches the parameters or the EMA.
 * guard = NULL is the unguarded call. */
int isr_mt_adam_guarded(const isr_mt_tensor* tensors, const isr_mt_chunk* chunks, int32_t nchunks,
                        const isr_adam_args* a, const float* scale, const uint32_t* guard, isr_stream_t s);
int isr_mt_lerp_guarded(const isr_mt_tensor* tensors, const isr_mt_chunk* chunks, int32_t nchunks, float d,
                        const uint32_t* guard, isr_stream_t s);

/* ---- image-quality metrics ------------------------------------------------
 * Squared error on RGB and on BT.601 luma, and SSIM on luma, of n image pairs in one pass over
 * both inputs.  The reference computes no metric: it only defines the luma and the 4-pixel crop
 * (Ychannel, utils/datasets.py:159-166, which nothing calls) and writes a val_images.json that
 * nothing reads (utils/general.py:107-111); PSNR / PSNR-Y / SSIM-Y follow the literature.
 * Each input is NCHW fp32 or uint8 with a per-channel affine into [0, 1] (uint8: 1/255, 0; tanh
 * space [-1, 1]: 0.5, 0.5; Normalize'd: std, mean), optionally clamped to [0, 1] and quantised to
 * the 8-bit value an image file would hold.  On the region left after cropping `border` pixels
 * from every side (hc = h - 2*border, wc = w - 2*border), per image:
 *   out[0] mse_rgb = mean over 3*hc*wc values of (a - b)^2
 *   out[1] mse_y   = mean over hc*wc of (Ya - Yb)^2, Y = (65.481 r + 128.553 g + 24.966 b + 16) / 255,
 *                    the difference formed from the channel differences (the +16 cancels)
 *   out[2] ssim_y  = mean SSIM (Wang et al. 2004) of Y*255: 11 x 11 Gaussian window, sigma 1.5,
 *                    normalised to sum 1, valid positions only ((hc - 10)*(wc - 10) windows, no
 *                    padding), biased window-weighted variances, C1 = (0.01*255)^2, C2 = (0.03*255)^2
 *   out[3]         = the number of SSIM windows
 * all on the [0, 1] scale, so PSNR = -10 log10(mse).  Moments and sums are fp64.  When both inputs
 * are uint8 with scale 1/255 and shift 0, mse_rgb is the exact integer sum of squares divided once
 * by 3*hc*wc*255^2.  No atomics: block partial sums go to the caller-owned workspace
 * (isr_image_metrics_workspace_bytes) and a second launch on the same stream adds them in a fixed
 * order, so two calls on the same inputs give the same bits.
 * A null pointer or n, h, w < 1 is ISR_ERR_BAD_DESC; hc < 11 or wc < 11 is ISR_ERR_UNSUPPORTED
 * (workspace size 0); nothing is launched then. */
typedef struct isr_metrics_desc {
    int32_t n, h, w;        /* images, NCHW [n][3][h][w], both inputs the same shape */
    int32_t border;         /* pixels cropped from every side before any metric (Ychannel: 4) */
    const void* a;          /* the estimate (SR) */
    const void* b;          /* the ground truth (HR) */
    int32_t a_u8, b_u8;     /* 0: fp32, 1: uint8 */
    float a_scale[3], a_shift[3];   /* value in [0,1] = v * scale[c] + shift[c] */
    float b_scale[3], b_shift[3];
    int32_t clamp;          /* 1: clamp both to [0,1] after the affine */
    int32_t quantize;       /* 1: round_half_even(x*255)/255 after the clamp (the metric of the saved image) */
    double* out;            /* [n][4]: mse_rgb, mse_y, ssim_y, valid SSIM windows (all on the [0,1] scale) */
} isr_metrics_desc;
size_t isr_image_metrics_workspace_bytes(const isr_metrics_desc* d);
int isr_image_metrics(const isr_metrics_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s);

/* ---- training-data degradations ---------------------------------------------
 * The second and third stage of the reference's Noisy_dataset (utils/datasets.py:374-377:
 * albumentations ISONoise and ImageCompression after GaussNoise), on uint8 crops that are already
 * on the device.  Every image is contiguous planar uint8 [n][3][h][w], RGB.  A null pointer or
 * n, h, w < 1 is ISR_ERR_BAD_DESC, an unsupported shape ISR_ERR_UNSUPPORTED; nothing is launched
 * then.  dst may be src.
 *
 * isr_jpeg_roundtrip: the decoded pixels of a baseline 4:2:0 JPEG of each image at quality[i]
 * (a device array; 1..100, 0 copies the image through unchanged, which is how a per-sample
 * probability is applied without a host sync; values above 100 act as 100, below 0 as 0).
 * Arithmetic as libjpeg: encode = JFIF RGB->YCbCr in 16-bit fixed point, h2v2 chroma downsample
 * ((sum of four + bias 1, 2, 1, 2, ...) >> 2), level shift, 8x8 DCT-II (fp32), IJG base tables
 * scaled by s = q < 50 ? 5000/q : 200 - 2q as clamp((base*s + 50)/100, 1, 255), quantised rounding
 * half away from zero; decode = dequantise, IDCT (fp32), + 128, round, clamp, h2v2 "fancy" triangle
 * upsample of the chroma planes (3:1 vertically then horizontally, biases 8 / 7, >> 4, edges
 * replicated at the component border, across MCU borders), fixed-point YCbCr->RGB, clamp.  The
 * coefficients (u, v) in {0, 4}^2 are integer sums / 8 and are carried as integers through both
 * transforms, so a flat region's quantisation ties round the same way on every run.  libjpeg's
 * integer DCT differs from the fp32 one by a few flipped coefficients.
 * h and w must be multiples of 16 (whole MCUs; otherwise ISR_ERR_UNSUPPORTED), src, dst and the
 * workspace 16-byte aligned, n*3*h*w < 2^31, n <= 65535.  Two launches on `s`; the workspace
 * (isr_jpeg_roundtrip_workspace_bytes, n*h*w*3/2) holds Y, Cb and Cr between them. */
typedef struct isr_jpeg_desc {
    int32_t n, h, w;
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* quality; /* device, [n] */
} isr_jpeg_desc;
size_t isr_jpeg_roundtrip_workspace_bytes(const isr_jpeg_desc* d);
int isr_jpeg_roundtrip(const isr_jpeg_desc* d, void* workspace, size_t ws_bytes, isr_stream_t s);

/* isr_hls_l_moments: per image the mean and the population standard deviation of the HLS
 * lightness L = (max(r,g,b) + min(r,g,b)) / 2 on the [0, 1] scale (cv2.meanStdDev of the L plane),
 * out[i] = {mean, std}.  max + min is an integer <= 510: its sum and sum of squares are
 * accumulated as 64-bit integers (block partials in the caller-owned `partials`, added by a second
 * launch; no atomics), N*S2 - S1^2 is formed in 128 bits and divided once, so the result is exact
 * to fp64 rounding and the same on every call; a flat image has std == 0 exactly.  Any h, w >= 1;
 * n <= 65535. */
#define ISR_HLS_PARTIAL_BLOCKS 32
typedef struct isr_hls_moments_desc {
    int32_t n, h, w;
    const uint8_t* src;
    double* out;        /* [n][2] */
    uint64_t* partials; /* scratch, [n][ISR_HLS_PARTIAL_BLOCKS][2] */
} isr_hls_moments_desc;
int isr_hls_l_moments(const isr_hls_moments_desc* d, isr_stream_t s);

/* isr_iso_noise: albumentations' ISONoise given its two noise planes.  Per pixel of an image
 * with apply[i] != 0 (apply[i] == 0 copies it through), in fp32, one rounding per operation:
 *   r, g, b = src / 255;  vmax, vmin;  sm = vmax + vmin;  d = vmax - vmin;  L = sm * 0.5
 *   d == 0: H = S = 0;  else S = L < 0.5 ? d / sm : d / (2 - sm),  k = 60 / d,
 *           H = (g-b)k | (b-r)k + 120 | (r-g)k + 240 for vmax == r | g | b,  H < 0: H += 360
 *   H += hue_noise;  H < 0: H += 360;  H > 360: H -= 360
 *   L = L + (lum_noise / 255) * (1 - L)
 *   S == 0: r = g = b = L;  else p2 = L <= 0.5 ? L(1 + S) : (L + S) - L*S,  p1 = 2L - p2,
 *           hh = H * (1/60);  hh -= 6 floor(hh * (1/6));  sector = clamp(floor(hh), 0, 5);
 *           f = hh - sector;  fall = p1 + (p2-p1)(1-f);  rise = p1 + (p2-p1)f;
 *           (r, g, b) = (p2,rise,p1) (fall,p2,p1) (p1,p2,rise) (p1,fall,p2) (rise,p1,p2) (p2,p1,fall)
 *   dst = (uint8) trunc(clamp(255 * (r, g, b), 0, 255))
 * lum_noise (Poisson counts) and hue_noise (degrees) are fp32 [n][h][w].  This formula is the
 * contract: it restates the published albumentations / OpenCV arithmetic and is not pinned against
 * either library.  Any h, w >= 1; n <= 65535. */
typedef struct isr_iso_noise_desc {
    int32_t n, h, w;
    const uint8_t* src;
    uint8_t* dst;
    const float* lum_noise;
    const float* hue_noise;
    const int32_t* apply; /* device, [n] */
} isr_iso_noise_desc;
int isr_iso_noise(const isr_iso_noise_desc* d, isr_stream_t s);

/* ---- PIL-exact resampling (LR synthesis) --------------------------------------
 * Pillow's Image.resize on 8-bit images (Imaging/Resample.c), bit for bit: two separable passes,
 * horizontal first, with a uint8 image between them; each pass accumulates pixel * k in int32, k
 * the normalised double weight rounded to 22 fractional bits, from 1 << 21, then >> 22 and clip
 * to 0..255.  On a downscale the filter's support is scaled by in/out (the antialiasing); the taps
 * are clamped at the image edge and the shortened kernel renormalised.  Covers the reference's
 * Random_low_rs (bicubic, antialias) and image_reader (BICUBIC / BILINEAR / BOX / NEAREST)
 * degradations (utils/datasets.py:23-32, :218-246).
 *
 * The coefficient tables are made on the host, in double, in Pillow's order of operations (plain
 * C++, no GPU): isr_resample_ksize is the taps per output pixel (0 when refused),
 * isr_resample_tables fills bounds [out_size][2] = (first source index, tap count) and coeffs
 * [out_size][ksize] (rows zero-padded).  NEAREST is a one-tap table (source index
 * floor((dst + 0.5) * in / out) in Pillow's running-sum form, coefficient 1 << 22), so one kernel
 * serves all six filters.  Refused with ISR_ERR_UNSUPPORTED: an unknown filter, a size outside
 * [1, 16384], and a ratio in_size / out_size outside [1/8, 8] — the bound that fixes the kernel's
 * footprint (at most ISR_RESAMPLE_MAX_KSIZE = 49 taps per axis). */
#define ISR_RESAMPLE_NEAREST 0
#define ISR_RESAMPLE_BOX 1
#define ISR_RESAMPLE_BILINEAR 2
#define ISR_RESAMPLE_HAMMING 3
#define ISR_RESAMPLE_BICUBIC 4
#define ISR_RESAMPLE_LANCZOS 5
#define ISR_RESAMPLE_MAX_KSIZE 49
int isr_resample_ksize(int filter, int in_size, int out_size);
int isr_resample_tables(int filter, int in_size, int out_size, int32_t* bounds, int32_t* coeffs);

/* isr_resample_u8: src uint8 planar [n][3][in_h][in_w] -> any non-empty subset of
 *   dst_u8 [n][3][out_h][out_w]   the resized image q,
 *   lr_f32 [n][3][out_h][out_w]   ((float)q / 255 - mean[c]) / std[c]  (isr_sr_transform's lr),
 *   hr_f32 [n][3][in_h][in_w]     2x/255 - 1, or (x/255 - mean[c]) / std[c] when hr_norm
 *                                 (isr_sr_transform's hr); only when in_h = sy * out_h and
 *                                 in_w = sx * out_w for integers sy, sx (ISR_ERR_UNSUPPORTED else).
 * The tables are DEVICE copies of isr_resample_tables' output for nf >= 1 filter variants, laid out
 * bounds_* [nf][out][2], coeffs_* [nf][out][ksize_*] with one ksize per axis (rows zero-padded to
 * it; 1 <= ksize <= 49).  filter_id (device int32 [n], or NULL = variant 0) picks each image's
 * variant on the device; ids outside [0, nf) are clamped.  in/out per axis must lie in [1/8, 8];
 * bounds are clamped to the image in the kernel, so a bad table gives wrong pixels, never a wild
 * access.  One launch on `s`: no workspace, no allocation, no synchronisation.  src and dst_u8
 * 4-byte aligned, lr_f32 and hr_f32 16-byte aligned, the tables and filter_id 4-byte aligned;
 * n <= 65535, n*3*in_h*in_w and n*3*out_h*out_w < 2^31; dst_u8 must not be src. */
typedef struct isr_resample_desc {
    int32_t n, in_h, in_w, out_h, out_w;
    int32_t nf, ksize_x, ksize_y;
    const uint8_t* src;
    const int32_t* bounds_x; /* device, [nf][out_w][2] */
    const int32_t* coeffs_x; /* device, [nf][out_w][ksize_x] */
    const int32_t* bounds_y; /* device, [nf][out_h][2] */
    const int32_t* coeffs_y; /* device, [nf][out_h][ksize_y] */
    const int32_t* filter_id; /* device, [n], or NULL */
    uint8_t* dst_u8; /* or NULL */
    float* lr_f32;   /* or NULL */
    float* hr_f32;   /* or NULL */
    int32_t hr_norm;
    float mean[3], std[3];
} isr_resample_desc;
int isr_resample_u8(const isr_resample_desc* d, isr_stream_t s);

/* ---- Blur degradations (LR synthesis) -----------------------------------------
 * The blur family of the reference's commented LR stages (utils/datasets.py:291-305: Blur,
 * GaussianBlur, MotionBlur, MedianBlur) on 8-bit images, in integer arithmetic from host-made
 * tables.
 *
 * isr_blur_taps (host, plain C++, no GPU) fills a 7 x 7 table of fixed-point taps with
 * ISR_BLUR_BITS = 16 fractional bits.  ksize must be 3, 5 or 7; the k x k window sits in the centre
 * of the table, the rest is zero.  The fp64 weights w (below), one rounding per operation, are
 * summed in row-major order and divided by the sum; tap = floor(w * 65536 + 0.5); then the centre
 * tap receives 65536 - (sum of the taps), so every table sums to exactly 65536 and has no negative
 * tap.  A parameter set whose centre tap would become negative is refused.
 *   ISR_BLUR_BOX       no params (NULL allowed): w = 1 on the k x k window.
 *   ISR_BLUR_GAUSSIAN  params = {sigma_x, sigma_y, angle_rad}.  With (dx, dy) the tap's offset from the
 *                      centre, u = (dx cos a + dy sin a) / sigma_x, v = (dy cos a - dx sin a) / sigma_y,
 *                      w = exp(-0.5 (u u + v v)).  A sigma <= 0 stands for cv2's rule
 *                      0.3 ((k - 1) 0.5 - 1) + 0.8 (albumentations' GaussianBlur at sigma_limit = 0).
 *   ISR_BLUR_MOTION    params = {x1, y1, x2, y2}: integer end points in [0, k - 1]^2 (x = column, y = row
 *                      of the window), not equal (albumentations' MotionBlur).  w = 1 on the pixels of
 *                      the line, which is this algorithm and nothing else (parity with cv2.line is not
 *                      pinned):
 *                          dx = |x2 - x1|, sx = x1 < x2 ? 1 : -1, dy = -|y2 - y1|, sy = y1 < y2 ? 1 : -1,
 *                          err = dx + dy, (x, y) = (x1, y1);
 *                          loop: mark (x, y); stop if (x, y) == (x2, y2); e2 = 2 err;
 *                                if e2 >= dy: err += dy, x += sx;   if e2 <= dx: err += dx, y += sy.
 *                      A line that misses the centre pixel leaves it the rounding residual alone.
 * Refused with ISR_ERR_UNSUPPORTED: an unknown kind, another ksize, a sigma or angle that is not
 * finite, end points that are not integers of the grid or are equal, a negative centre tap;
 * ISR_ERR_BAD_DESC: a null table, null params for a kind that has some. */
#define ISR_BLUR_MAX_K 7
#define ISR_BLUR_BITS 16
#define ISR_BLUR_BOX 0
#define ISR_BLUR_GAUSSIAN 1
#define ISR_BLUR_MOTION 2
int isr_blur_taps(int kind, int ksize, const double* params, int32_t* taps /* [49] */);

/* isr_blur_u8: src uint8 planar [n][3][h][w] -> dst of the same shape, per image i:
 *   ksize[i] not in {3, 5, 7}   dst = src (a copy-through; median[i] and the table are ignored);
 *   median[i] == 0              acc = sum over the k x k window of tap * pixel (int32, formed in
 *                               unsigned arithmetic: a table too large wraps),
 *                               dst = clip((acc + 32768) >> 16, 0, 255), the shift arithmetic (floor);
 *                               border reflect-101 (-1 -> 1, h -> h - 2: cv2's default for blur,
 *                               GaussianBlur and filter2D).  The window is the centre k x k of image
 *                               i's table taps[i][7][7] (row-major, row = vertical offset): taps
 *                               outside it are not read.  Any table with sum |tap| <= 2^23 is exact
 *                               (a sharpening kernel with negative taps, say); the clip makes it safe;
 *   median[i] != 0              the exact median of the k x k window, border replicated (cv2's
 *                               medianBlur, Pillow's MedianFilter): the smallest v with at least
 *                               (k k + 1) / 2 window pixels <= v.
 * ksize, median and taps are DEVICE arrays.  Source indices are clamped to the image after the border
 * rule, so no value in them can make the kernel read or write outside the images.  One launch on `s`:
 * no workspace, no allocation, no synchronisation.  h, w >= 7; n in [1, 65535]; n*3*h*w < 2^31; dst
 * must not be src; ksize, median and taps 4-byte aligned (src and dst: any alignment; 4-byte aligned
 * with w % 4 == 0 takes the dword loads and stores). */
typedef struct isr_blur_desc {
    int32_t n, h, w;
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* ksize;  /* device, [n]: 3, 5 or 7; any other value copies that image through */
    const int32_t* median; /* device, [n]: non-zero = median of the k x k window */
    const int32_t* taps;   /* device, [n][49]: a linear image's table */
} isr_blur_desc;
int isr_blur_u8(const isr_blur_desc* d, isr_stream_t s);

/* ---- YUV 4:2:0 video frames ----------------------------------------------------
 * 8-bit 4:2:0 Y'CbCr frames <-> planar uint8 RGB [n][3][h][w], in integer arithmetic from host-made
 * coefficients: what a video source hands over and a video sink takes (the video path's
 * FrameUpscaler.x / .y), in place of packed rgb24 / bgr24.  h and w even and at least 2.
 *
 * A frame is 3 h w / 2 bytes; a batch is n frames back to back.
 *   ISR_YUV_I420   planes Y [h][w], U [h/2][w/2], V [h/2][w/2], back to back (ffmpeg's yuv420p)
 *   ISR_YUV_NV12   plane Y [h][w], then [h/2] rows of w bytes U0 V0 U1 V1 ...
 *
 * isr_yuv_coeffs (host, plain C++, no GPU) makes the coefficients with ISR_YUV_BITS = 16 fractional
 * bits: fix(v) = floor(v * 65536 + 0.5) of the exact fp64 value, one rounding per operation.
 *   matrix  ISR_YUV_BT601 (Kr 0.299, Kb 0.114) or ISR_YUV_BT709 (Kr 0.2126, Kb 0.0722); Kg = 1 - Kr - Kb
 *   range   limited (full_range 0): sy = 219/255, sc = 224/255, oy = 16; full: sy = sc = 1, oy = 0
 *   fwd[9]  rows Y, Cb, Cr over (R, G, B):
 *             Y  = sy (Kr, Kg, Kb)
 *             Cb = sc (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb))
 *             Cr = sc (1 - Kr, -Kg, -Kb) / (2 (1 - Kr))
 *           The R and B entries are fix()ed; the G entry is then set so that the Y row sums to exactly
 *           fix(sy) and each chroma row to exactly 0: a grey pixel gives Cb = Cr = 128.
 *   inv[5]  cy = 1/sy, crv = 2 (1 - Kr) / sc, cbu = 2 (1 - Kb) / sc, cgu = -cbu Kb / Kg,
 *           cgv = -crv Kr / Kg, in this order, each fix()ed.
 * Refused: an unknown matrix ISR_ERR_UNSUPPORTED; a null pointer ISR_ERR_BAD_DESC.
 *
 * Chroma siting: ISR_YUV_SITING_LEFT (MPEG-2 / H.264 / HEVC: the chroma sample sits on the even luma
 * column, midway between the two luma rows) or ISR_YUV_SITING_CENTER (JPEG / MPEG-1: the centre of the
 * 2 x 2 block).  clamp8 clips to [0, 255]; >> is an arithmetic (flooring) shift; every stored value is
 * rounded once.
 *
 * isr_rgb_to_yuv420_u8: src planar RGB [n][3][h][w] -> dst frames.
 *   Y[y][x] = clamp8((fwdY . (R, G, B) + oy 65536 + 32768) >> 16)
 *   C[i][j] = clamp8((fwdC . S + 128 65536 D + 32768 D) >> (16 + log2 D)), with S the integer footprint
 *   sums of R, G and B:
 *     center  the 2 x 2 block (rows 2i, 2i+1, columns 2j, 2j+1), D = 4
 *     left    columns 2j-1, 2j, 2j+1 with weights 1, 2, 1 over rows 2i and 2i+1, D = 8; column -1
 *             replicates column 0
 *
 * isr_yuv420_to_rgb_u8: src frames -> dst planar RGB [n][3][h][w].  Chroma is upsampled as integer
 * numerators (indices past an edge replicate the edge):
 *   horizontal, left    H[2j] = 2 C[j],            H[2j+1] = C[j] + C[j+1]
 *   horizontal, center  H[2j] = 3 C[j] + C[j-1],   H[2j+1] = 3 C[j] + C[j+1]
 *   vertical, both      row 2i = 3 H_i + H_(i-1),  row 2i+1 = 3 H_i + H_(i+1)
 * giving U*, V* with D = 8 (left) or 16 (center); then
 *   R = clamp8((cy D (Y - oy) + crv (V* - 128 D) + 32768 D) >> (16 + log2 D))
 *   G = clamp8((cy D (Y - oy) + cgu (U* - 128 D) + cgv (V* - 128 D) + 32768 D) >> (16 + log2 D))
 *   B = clamp8((cy D (Y - oy) + cbu (U* - 128 D) + 32768 D) >> (16 + log2 D))
 * All sums fit int32 for the coefficients isr_yuv_coeffs makes (the largest is about 5.9e8; other
 * coefficients wrap, they cannot make an access go wild).  Y outside [16, 235] and chroma of 0 or 255 are legal inputs: only the final clamp
 * limits the result.
 *
 * Both are one launch on `s`, stateless: no device table, no workspace, no allocation, no
 * synchronisation.  n in [1, 65535]; h, w even, >= 2, h w <= 2^28; dst must not be src; src and dst: any
 * alignment (16-byte accesses are used per plane where w % 16 == 0 and that plane's address allows). */
#define ISR_YUV_BITS 16
#define ISR_YUV_BT601 0
#define ISR_YUV_BT709 1
#define ISR_YUV_I420 0
#define ISR_YUV_NV12 1
#define ISR_YUV_SITING_LEFT 0
#define ISR_YUV_SITING_CENTER 1
int isr_yuv_coeffs(int matrix, int full_range, int32_t* fwd /* [9] */, int32_t* inv /* [5] */);

typedef struct isr_yuv_desc {
    int32_t n, h, w;        /* of the RGB image = of the luma plane */
    int32_t layout;         /* ISR_YUV_I420 / ISR_YUV_NV12 */
    int32_t siting;         /* ISR_YUV_SITING_LEFT / ISR_YUV_SITING_CENTER */
    int32_t full_range;     /* 0: oy = 16; non-zero: oy = 0 */
    int32_t fwd[9], inv[5]; /* isr_yuv_coeffs' (each entry point reads its own) */
    const uint8_t* src;
    uint8_t* dst;
} isr_yuv_desc;
int isr_yuv420_to_rgb_u8(const isr_yuv_desc* d, isr_stream_t s);
int isr_rgb_to_yuv420_u8(const isr_yuv_desc* d, isr_stream_t s);

/* ---- YUV 4:2:0 video frames of more than 8 bits ---------------------------------
 * 10-bit 4:2:0 frames (ffmpeg's yuv420p10le and p010le: what HEVC Main10 and AV1 decoders hand over)
 * <-> RGB at the same depth, or straight to the head's normalised fp32 input and from the tail's fp32
 * tanh, so that a 10-bit side of the video path has no 8-bit step.  d = depth = 10 below.
 *
 * A sample is a 16-bit little-endian word; a frame is 3 h w bytes, in the layout of the 8-bit section
 * with words for bytes (ISR_YUV_I420: three planes of words; ISR_YUV_NV12: a Y plane, then rows of w
 * words U0 V0 U1 V1 ...).  `shift` is the sample's position in its word: 0 for yuv420p10le, 6 for p010le.
 *   read    sample = (word >> shift) & (2^d - 1): bits outside the field are ignored
 *   write   word = sample << shift: every other bit is 0
 *
 * isr_yuv_coeffs_depth (host, plain C++, no GPU) makes the coefficients as isr_yuv_coeffs does, same
 * fix(), same ISR_YUV_BITS, same closing of the rows (Y sums to fix(sy), chroma to 0: a grey pixel gives
 * Cb = Cr = 2^(d-1) exactly), with
 *   limited  sy = 219 2^(d-8) / (2^d - 1), sc = 224 2^(d-8) / (2^d - 1), oy = 16 2^(d-8)
 *   full     sy = sc = 1, oy = 0
 * depth 8 gives isr_yuv_coeffs' integers exactly.  Refused: an unknown matrix and a depth other than 8 or
 * 10 ISR_ERR_UNSUPPORTED; a null pointer ISR_ERR_BAD_DESC.
 *
 * The RGB side, `rgb_kind`:
 *   ISR_RGB_U16       both directions: planar uint16 [n][3][h][w] of 0 .. 2^d - 1 (on input the low d bits
 *                     of each word are read)
 *   ISR_RGB_NORM_F32  yuv -> rgb only: fp32 [n][3][h][w], the head's input
 *                       x = ((float)v / (float)(2^d - 1) - mean[c]) * inv_std[c]
 *                     one IEEE division, one subtraction, one multiplication, each rounded once
 *   ISR_RGB_TANH_F32  rgb -> yuv only: fp32 [n][3][h][w] t, the tail's output, quantised as the tail does
 *                     for uint8:
 *                       v = 0 unless t > -1 (NaN, -inf: 0); v = 2^d - 1 if t >= 1; otherwise
 *                       v = clamp(rint((t + 1.0f) * 0.5f * (float)(2^d - 1))), round-half-even, each
 *                     operation rounded once in fp32
 *
 * The arithmetic is the 8-bit section's with oy as above, 128 -> 2^(d-1), 255 -> 2^d - 1 (clampd clips to
 * [0, 2^d - 1]), the same sitings, edge replication and D, every stored integer rounded once:
 *   Y[y][x] = clampd((fwdY . (R, G, B) + oy 65536 + 32768) >> 16)
 *   C[i][j] = clampd((fwdC . S + 2^(d-1) 65536 D + 32768 D) >> (16 + log2 D))
 *   R = clampd((cy D (Y - oy) + crv (V* - 2^(d-1) D) + 32768 D) >> (16 + log2 D))
 *   G = clampd((cy D (Y - oy) + cgu (U* - 2^(d-1) D) + cgv (V* - 2^(d-1) D) + 32768 D) >> (16 + log2 D))
 *   B = clampd((cy D (Y - oy) + cbu (U* - 2^(d-1) D) + 32768 D) >> (16 + log2 D))
 * Bounds at d = 10 over isr_yuv_coeffs_depth's four tables (the kernels mask every sample to d bits, so
 * these hold for any frame):
 *   rgb -> yuv  the Y sum is at most 65536 1023 + 64 65536 + 32768 < 7.2e7; a chroma sum is at most
 *               0.5 65536 (8 1023) + 512 65536 8 + 32768 8 < 5.4e8 (left, D = 8): int32 holds both.
 *   yuv -> rgb  center siting, D = 16.  The luma term cy D (Y - oy) + 32768 D lies in [-7.9e7, 1.175e9]
 *               (limited: cy = 76533, Y - oy in [-64, 959]) and each chroma product within +-1.138e9
 *               (cbu <= 138846, bt709 limited, |U* - 512 D| <= 8192): each fits int32 on its own.
 *               Their sums do not all fit: the blue sum reaches 1.175e9 + 1.135e9 = 2.31e9 (bt709
 *               limited; bt601 limited 2.26e9) and the red sum 2.138e9, 0.4 % under 2^31 - 1.  So the red
 *               and the blue sum are formed in 64 bits.  The green sum has two negative coefficients and
 *               is at most 1.175e9 + 8192 (25750 + 53435) = 1.824e9 (bt601 limited) and at least
 *               -7.8e7 - 8176 (25750 + 53435) = -7.3e8: int32.  Left siting (D = 8) halves every term.
 * Other coefficients wrap in the 32-bit terms; they cannot move an access.
 *
 * isr_yuv420_to_rgb_16: src frames -> dst RGB (ISR_RGB_U16 or ISR_RGB_NORM_F32).
 * isr_rgb_to_yuv420_16: src RGB (ISR_RGB_U16 or ISR_RGB_TANH_F32) -> dst frames.
 * Both are one launch on `s`, stateless: no device table, no workspace, no allocation, no
 * synchronisation.  n in [1, 65535]; h, w even, >= 2, h w <= 2^28; dst must not be src.  Frames and
 * uint16 RGB must be 2-byte aligned and fp32 RGB 4-byte aligned (else ISR_ERR_BAD_DESC); 16-byte accesses
 * are used per plane where w % 16 == 0 and that plane's address allows, element accesses otherwise and
 * at a ragged right edge.  Refused before any launch: null pointers, odd or too small h, w
 * (ISR_ERR_BAD_DESC); an unknown layout, siting or rgb_kind, a kind of the other direction, a depth other
 * than 10, shift < 0 or shift + depth > 16 (ISR_ERR_UNSUPPORTED). */
#define ISR_RGB_U16 0
#define ISR_RGB_NORM_F32 1
#define ISR_RGB_TANH_F32 2
int isr_yuv_coeffs_depth(int matrix, int full_range, int depth, int32_t* fwd /* [9] */, int32_t* inv /* [5] */);

typedef struct isr_yuv16_desc {
    int32_t n, h, w;        /* of the RGB image = of the luma plane */
    int32_t layout;         /* ISR_YUV_I420 / ISR_YUV_NV12 */
    int32_t siting;         /* ISR_YUV_SITING_LEFT / ISR_YUV_SITING_CENTER */
    int32_t full_range;     /* 0: oy = 16 2^(depth-8); non-zero: oy = 0 */
    int32_t depth;          /* 10 */
    int32_t shift;          /* the sample's position in its word: 0 (yuv420p10le) .. 16 - depth (p010le) */
    int32_t rgb_kind;       /* ISR_RGB_U16 / ISR_RGB_NORM_F32 / ISR_RGB_TANH_F32 */
    int32_t fwd[9], inv[5]; /* isr_yuv_coeffs_depth's (each entry point reads its own) */
    float mean[3], inv_std[3]; /* ISR_RGB_NORM_F32 */
    const void* src;
    void* dst;
} isr_yuv16_desc;
int isr_yuv420_to_rgb_16(const isr_yuv16_desc* d, isr_stream_t s);
int isr_rgb_to_yuv420_16(const isr_yuv16_desc* d, isr_stream_t s);

/* ---- dihedral transforms: the eight flips and rotations of an image -------------
 * An op id is k = r + 4 f with r in 0..3 and f in {0, 1}: with f set, first mirror the image along its
 * width (column j <-> column w - 1 - j); then turn it r quarter turns counter-clockwise.  An odd r swaps
 * height and width.  With x the h x w source and y the result, y[i][j] is
 *   k = 0  x[i][j]                 (h x w)      k = 4  x[i][w - 1 - j]            (h x w)
 *   k = 1  x[j][w - 1 - i]         (w x h)      k = 5  x[j][i]                    (w x h, the transpose)
 *   k = 2  x[h - 1 - i][w - 1 - j] (h x w)      k = 6  x[h - 1 - i][j]            (h x w)
 *   k = 3  x[h - 1 - j][i]         (w x h)      k = 7  x[h - 1 - j][w - 1 - i]    (w x h)
 * The inverse of k is (4 - k) % 4 for k < 4 and k itself for k >= 4 (a reflection undoes itself):
 * isr_dihedral_inverse (host only; ISR_ERR_BAD_DESC for k outside 0..7, which sets isr_last_error()).
 * Values are moved, never changed: every entry point below is exact.
 *
 * isr_dihedral: x [n][c][h][w] -> y [n][c][h'][w'], elements of `elem` bytes (1: uint8, 4: fp32 or any
 * other 4-byte type).  With ops == NULL every image takes the uniform `op` (0..7, else
 * ISR_ERR_UNSUPPORTED).  With ops a DEVICE array int32 [n], image i takes ops[i] & 7 (any value is
 * therefore safe; it is never read on the host) and h == w is required (ISR_ERR_UNSUPPORTED otherwise:
 * the results would not share a shape).  One launch on `s`, no workspace, no synchronisation.
 * Refused before any launch: a null descriptor, null x or y, x == y (ISR_ERR_BAD_DESC); x, y not
 * aligned to elem bytes, ops not 4-byte aligned (ISR_ERR_BAD_DESC); n or c outside [1, 65535], h or
 * w < 1 (ISR_ERR_BAD_DESC); h * w >= 2^31 or more than 2^31 - 1 workgroups (ISR_ERR_UNSUPPORTED); elem
 * other than 1 or 4 (ISR_ERR_UNSUPPORTED).  uint8 planes that are 4-byte aligned with w and h multiples of
 * 4 take dword loads and stores; any other shape and alignment is served bytewise at the ragged places. */
typedef struct isr_dihedral_desc {
    int32_t n, c, h, w;  /* the source's shape */
    int32_t elem;        /* bytes per element: 1 or 4 */
    int32_t op;          /* the uniform op, 0..7 (read when ops is NULL) */
    const int32_t* ops;  /* device, [n], or NULL */
    const void* x;
    void* y;
} isr_dihedral_desc;
int isr_dihedral(const isr_dihedral_desc* d, isr_stream_t s);
int isr_dihedral_inverse(int op);

/* isr_ensemble_expand_u8: the eight transformed copies of each image of x uint8 [n][3][h][w], in one
 * launch.  Member k of image i (op k applied to it) is image (k / 2) * n + i of `even` [4n][3][h][w] for
 * k = 0, 2, 4, 6 and of `odd` [4n][3][w][h] for k = 1, 3, 5, 7: two batches, because the odd members have
 * the transposed shape (square images use the same form).  n in [1, 16383] (4n is a batch of the other
 * entry points); otherwise the rules of isr_dihedral; x, even and odd must be three different buffers. */
typedef struct isr_ensemble_expand_desc {
    int32_t n, h, w;
    const uint8_t* x;
    uint8_t* even;
    uint8_t* odd;
} isr_ensemble_expand_desc;
int isr_ensemble_expand_u8(const isr_ensemble_expand_desc* d, isr_stream_t s);

/* isr_ensemble_reduce: the self-ensemble's average.  even fp32 [4n][3][h][w] and odd fp32 [4n][3][w][h]
 * hold a network's outputs (tanh range, [-1, 1]) for the members in isr_ensemble_expand_u8's order, at the
 * OUTPUT size h x w.  Per output element the eight members are read where the inverse op of each puts
 * that element, added in fp32 in the fixed order s = m0; s = s + m1; ...; s = s + m7, and m = s * 0.125f.
 * y_u8 == 0 stores m as fp32 [n][3][h][w]; otherwise uint8 with the generator tail's own expression,
 * q = rintf((m + 1.f) / 2.f * 255.f) (ties to even), clamped to [0, 255].  No atomics and no workspace:
 * the result is the same bits on every run.  even and odd must be 4-byte aligned (16-byte aligned rows
 * take 16-byte loads), y aligned to its element; n in [1, 16383]; otherwise the rules of isr_dihedral. */
typedef struct isr_ensemble_reduce_desc {
    int32_t n, h, w;  /* the output's shape */
    const float* even;
    const float* odd;
    void* y;
    int32_t y_u8;
} isr_ensemble_reduce_desc;
int isr_ensemble_reduce(const isr_ensemble_reduce_desc* d, isr_stream_t s);

const char* isr_last_error(void);
int isr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ISR_H */
