// Every isr:: function that capi.hip calls across translation units, declared once.  capi.hip includes
// this, and so does every .hip that defines one of them, so a definition whose parameter list or return
// type disagrees fails to compile (a copied prototype with a wrong return type would link).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "isr.h"

namespace isr {

// What a *_dispatch / *_launch / *_set answers; capi.hip turns it into an ISR_ERR_* and a message.
enum : int {
    DISPATCH_OK = 0,
    DISPATCH_LAUNCH = -1,         // a HIP call failed (hipGetLastError() says which)
    DISPATCH_UNSUPPORTED = -2,    // no kernel for this shape / variant / build
    DISPATCH_WS_TOO_SMALL = -3,   // the workspace is smaller than the size query's figure
    DISPATCH_NO_OCCUPANCY = -4,   // the occupancy query admits no workgroup per CU
};

// conv3x3.hip
int conv3x3_fwd_dispatch(const isr_conv_desc* d, hipStream_t s);
int conv3x3_fwd_variant(const isr_conv_desc* d, int variant, hipStream_t s);
int conv_stamps_set(void* p);
size_t conv3x3_packed_bytes(int cout, int cin);
int conv3x3_pack(const float* w, void* out, int cout, int cin, hipStream_t s);
int conv3x3_pack_f16(const float* w, void* out, int cout, int cin, hipStream_t s);
int conv3x3_pack_dgrad(const float* w, void* out, int cout, int cin, float scale, int sub2, hipStream_t s);
int conv3x3_pack_batch(const isr_pack_item* items, int n, hipStream_t s);
// conv3x3_wino.hip
size_t conv3x3_wino_packed_bytes(int cout, int cin);
int conv3x3_wino_pack(const float* w, void* out, int cout, int cin, hipStream_t s);
int conv3x3_wino_fwd_dispatch(const isr_conv_desc* d, hipStream_t s);
// trunk.hip
size_t trunk_state_words(int n, int ha, int wa);
int trunk_launch(const isr_chain_desc* c, hipStream_t s);
int trunk_stamps_set(void* p);
int trunk_knobs_set(const int* k);
int trunk_item_stamps_set(void* p);
// conv9x9.hip
int head9x9_fwd_dispatch(const isr_head_desc* d, hipStream_t s);
int tail9x9_fwd_dispatch(const isr_tail_desc* d, hipStream_t s);
int tail9x9_fwd_variant(const isr_tail_desc* d, int variant, hipStream_t s);
int tail_segment_rows(const isr_tail_desc* d, int cus);
size_t head9x9_packed_bytes(int cout);
size_t tail9x9_packed_bytes();
int head9x9_pack(const float* w, void* out, int cout, int cin, hipStream_t s, bool h);
int tail9x9_pack(const float* w, void* out, int cout, int cin, hipStream_t s, bool h);
// wgrad3x3.hip, wgrad9x9.hip
size_t wgrad3x3_workspace_bytes(const isr_wgrad_desc* d, int variant);
int wgrad3x3_dispatch(const isr_wgrad_desc* d, int variant, void* ws, size_t ws_bytes, hipStream_t s, int parts);
size_t wgrad3x3_group_workspace_bytes(const isr_wgrad_desc* ds, int n, int variant);
int wgrad3x3_group_dispatch(const isr_wgrad_desc* ds, int n, void* ws, size_t ws_bytes, hipStream_t s, int variant);
size_t wgrad9x9_workspace_bytes(const isr_wgrad9_desc* d);
int wgrad9x9_dispatch(const isr_wgrad9_desc* d, void* ws, size_t ws_bytes, hipStream_t s);
// elementwise.hip
int ew_combine_dispatch(const isr_ew_desc* d, hipStream_t s);
int pixel_shuffle2_dispatch(const isr_ew_desc* d, hipStream_t s);
int pixel_unshuffle2_dispatch(const isr_ew_desc* d, hipStream_t s);
int sr_transform_dispatch(const isr_sr_transform_desc* d, hipStream_t s);
int bn_dispatch(const isr_bn_desc* d, int op, hipStream_t s);
int nchw_to_blocked_dispatch(const isr_convert_desc* d, hipStream_t s);
int blocked_to_nchw_dispatch(const isr_convert_desc* d, hipStream_t s);
int maxpool2_dispatch(const isr_pool_desc* d, int backward, hipStream_t s);
// optim.hip
int mt_adam_dispatch(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int n, const isr_adam_args* a,
                     const float* scale, const uint32_t* guard, hipStream_t s);
int mt_sumsq_dispatch(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int n, float* partial, hipStream_t s);
int clip_coef_dispatch(const float* partial, int n, float max_norm, float* out, hipStream_t s);
int mt_axpby_dispatch(const isr_mt_tensor* ts, const isr_mt_chunk* cs, int n, int mode, const float* coef, float d,
                      const uint32_t* guard, hipStream_t s);
// metrics.hip, degrade.hip, resample.hip, blur.hip
size_t image_metrics_workspace_bytes(const isr_metrics_desc* d);
int image_metrics_dispatch(const isr_metrics_desc* d, void* ws, size_t ws_bytes, hipStream_t s);
size_t jpeg_roundtrip_workspace_bytes(const isr_jpeg_desc* d);
int jpeg_roundtrip_dispatch(const isr_jpeg_desc* d, void* ws, size_t ws_bytes, hipStream_t s);
int hls_l_moments_dispatch(const isr_hls_moments_desc* d, hipStream_t s);
int iso_noise_dispatch(const isr_iso_noise_desc* d, hipStream_t s);
int resample_u8_dispatch(const isr_resample_desc* d, hipStream_t s);
int blur_u8_dispatch(const isr_blur_desc* d, hipStream_t s);
// yuv.hip, yuv16.hip, dihedral.hip
int yuv_dispatch(const isr_yuv_desc* d, int to_rgb, hipStream_t s);
int yuv16_dispatch(const isr_yuv16_desc* d, int to_rgb, hipStream_t s);
int dihedral_dispatch(const isr_dihedral_desc* d, hipStream_t s);
int ensemble_expand_u8_dispatch(const isr_ensemble_expand_desc* d, hipStream_t s);
int ensemble_reduce_dispatch(const isr_ensemble_reduce_desc* d, hipStream_t s);
int dihedral_inverse(int op);

}  // namespace isr
