"""One refusal table for the uint8-batch entry points of the C ABI (isr_jpeg_roundtrip,
isr_hls_l_moments, isr_iso_noise, isr_resample_u8, isr_blur_u8) and isr_image_metrics, no GPU: per
row an entry point, a bad descriptor, the return code and what isr_last_error() must say (always the
entry point's name).  Every call is refused before anything is launched or dereferenced, so the
pointers are made-up aligned addresses."""
import ctypes

from image_super_resolution_amd import _lib

BAD_DESC, UNSUPPORTED = -1, -2
P = 0x10000  # aligned, never followed
F3 = ctypes.c_float * 3
WS = dict(workspace=P, ws_bytes=1 << 20)

# entry point -> (descriptor class, a descriptor that passes every check, takes a workspace)
ENTRIES = {
    "jpeg_roundtrip": (_lib.IsrJpegDesc, dict(n=2, h=32, w=48, src=P, dst=2 * P, quality=3 * P), True),
    "hls_l_moments": (_lib.IsrHlsMomentsDesc, dict(n=1, h=8, w=8, src=P, out=2 * P, partials=3 * P), False),
    "iso_noise": (_lib.IsrIsoNoiseDesc, dict(n=1, h=8, w=8, src=P, dst=2 * P, lum_noise=3 * P, hue_noise=4 * P,
                                            apply=5 * P), False),
    "resample_u8": (_lib.IsrResampleDesc,
                    dict(n=2, in_h=48, in_w=48, out_h=12, out_w=12, nf=1, ksize_x=17, ksize_y=17, src=P, bounds_x=P,
                         coeffs_x=P, bounds_y=P, coeffs_y=P, filter_id=None, dst_u8=2 * P, lr_f32=None, hr_f32=None,
                         hr_norm=0, mean=F3(0.5, 0.5, 0.5), std=F3(0.25, 0.25, 0.25)), False),
    "blur_u8": (_lib.IsrBlurDesc, dict(n=2, h=16, w=16, src=P, dst=2 * P, ksize=3 * P, median=4 * P, taps=5 * P),
                False),
    "image_metrics": (_lib.IsrMetricsDesc,
                      dict(n=2, h=75, w=43, border=4, a=P, b=P, a_u8=1, b_u8=1, a_scale=F3(1, 1, 1), a_shift=F3(),
                           b_scale=F3(1, 1, 1), b_shift=F3(), clamp=1, quantize=0, out=P), True),
}

# (entry point, descriptor fields to change (None: a null descriptor; workspace / ws_bytes: the call's), return code,
#  further substrings of the message)
TABLE = [
    ("jpeg_roundtrip", None, BAD_DESC, ()),
    ("jpeg_roundtrip", dict(n=1, h=24, w=32), UNSUPPORTED, ("16",)),
    ("jpeg_roundtrip", dict(ws_bytes=16), BAD_DESC, ("workspace",)),
    ("jpeg_roundtrip", dict(n=0), BAD_DESC, ()),
    ("jpeg_roundtrip", dict(n=65536), BAD_DESC, ()),
    ("jpeg_roundtrip", dict(h=0), BAD_DESC, ()),
    ("jpeg_roundtrip", dict(n=1, dst=None), BAD_DESC, ("null",)),
    ("jpeg_roundtrip", dict(n=4, h=16384, w=16384), UNSUPPORTED, ("31 bits",)),
    ("jpeg_roundtrip", dict(src=P + 4), BAD_DESC, ("aligned",)),
    ("jpeg_roundtrip", dict(quality=3 * P + 2), BAD_DESC, ("aligned",)),
    ("jpeg_roundtrip", dict(workspace=None), BAD_DESC, ("workspace",)),
    ("jpeg_roundtrip", dict(workspace=P + 8), BAD_DESC, ("workspace",)),
    ("hls_l_moments", None, BAD_DESC, ()),
    ("hls_l_moments", dict(h=0), BAD_DESC, ()),
    ("hls_l_moments", dict(n=0), BAD_DESC, ()),
    ("hls_l_moments", dict(n=65536), BAD_DESC, ()),
    ("hls_l_moments", dict(partials=None), BAD_DESC, ("null",)),
    ("hls_l_moments", dict(out=2 * P + 4), BAD_DESC, ("aligned",)),
    ("iso_noise", None, BAD_DESC, ()),
    ("iso_noise", dict(hue_noise=None), BAD_DESC, ("null",)),
    ("iso_noise", dict(w=-1), BAD_DESC, ()),
    ("iso_noise", dict(h=0), BAD_DESC, ()),
    ("iso_noise", dict(n=0), BAD_DESC, ()),
    ("iso_noise", dict(n=65536), BAD_DESC, ()),
    ("iso_noise", dict(lum_noise=3 * P + 2), BAD_DESC, ("aligned",)),
    ("iso_noise", dict(h=1 << 20, w=1 << 20), UNSUPPORTED, ("workgroups",)),
    ("resample_u8", None, BAD_DESC, ()),
    ("resample_u8", dict(out_h=13, hr_f32=0x30000), UNSUPPORTED, ("integer ratio",)),
    ("resample_u8", dict(in_w=109), UNSUPPORTED, ("ratio",)),
    ("resample_u8", dict(out_w=0), UNSUPPORTED, ("sizes",)),
    ("resample_u8", dict(in_h=0), UNSUPPORTED, ("sizes",)),
    ("resample_u8", dict(ksize_x=50), UNSUPPORTED, ("ksize",)),
    ("resample_u8", dict(n=4, in_h=16384, in_w=16384, out_h=4096, out_w=4096), UNSUPPORTED, ("31 bits",)),
    ("resample_u8", dict(dst_u8=None), BAD_DESC, ("no output",)),
    ("resample_u8", dict(src=None), BAD_DESC, ("null",)),
    ("resample_u8", dict(coeffs_y=None), BAD_DESC, ("null",)),
    ("resample_u8", dict(nf=0), BAD_DESC, ()),
    ("resample_u8", dict(n=0), BAD_DESC, ()),
    ("resample_u8", dict(n=65536), BAD_DESC, ()),
    ("resample_u8", dict(dst_u8=P), BAD_DESC, ("must not be src",)),
    ("resample_u8", dict(lr_f32=0x30004), BAD_DESC, ("aligned",)),
    ("resample_u8", dict(src=P + 2), BAD_DESC, ("aligned",)),
    ("blur_u8", None, BAD_DESC, ("null descriptor",)),
    ("blur_u8", dict(h=6), UNSUPPORTED, ("smaller than",)),
    ("blur_u8", dict(w=6), UNSUPPORTED, ("smaller than",)),
    ("blur_u8", dict(h=0), UNSUPPORTED, ("smaller than",)),
    ("blur_u8", dict(n=0), BAD_DESC, ()),
    ("blur_u8", dict(n=-1), BAD_DESC, ()),
    ("blur_u8", dict(n=65536), BAD_DESC, ()),
    ("blur_u8", dict(src=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(dst=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(ksize=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(median=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(taps=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(dst=P), BAD_DESC, ("must not be src",)),
    ("blur_u8", dict(taps=5 * P + 2), BAD_DESC, ("aligned",)),
    ("blur_u8", dict(n=4, h=16384, w=16384), UNSUPPORTED, ("31 bits",)),
    ("image_metrics", None, BAD_DESC, ("null descriptor",)),
    ("image_metrics", dict(n=1, h=64, w=64, a=None, b=None, out=None), BAD_DESC, ("null",)),
    ("image_metrics", dict(n=0, h=64, w=64), BAD_DESC, ()),
    ("image_metrics", dict(n=65536, h=64, w=64), BAD_DESC, ()),
    ("image_metrics", dict(n=1, h=0, w=64), BAD_DESC, ()),
    ("image_metrics", dict(n=1, h=64, w=-3), BAD_DESC, ()),
    ("image_metrics", dict(n=1, h=20, w=30, border=5), UNSUPPORTED, ("11-pixel", "window")),
    ("image_metrics", dict(workspace=None, ws_bytes=0), BAD_DESC, ("workspace",)),
    ("image_metrics", dict(ws_bytes=16), BAD_DESC, ("workspace",)),
]


def _refusal(lib, entry, change):
    """(return code, message) of one row's call."""
    cls, good, has_ws = ENTRIES[entry]
    call = dict(WS)
    if change is None:
        desc, call = None, dict(workspace=None, ws_bytes=0)
    else:
        call.update({k: v for k, v in change.items() if k in call})
        desc = ctypes.byref(cls(**{**good, **{k: v for k, v in change.items() if k not in call}}))
    fn = getattr(lib, "isr_" + entry)
    rc = fn(desc, call["workspace"], call["ws_bytes"], None) if has_ws else fn(desc, None)
    return rc, lib.isr_last_error().decode()


def test_refused_without_a_launch(built_lib):
    """Every row of the table; all rows that miss are reported together."""
    missed = []
    for entry, change, code, says in TABLE:
        rc, msg = _refusal(built_lib, entry, change)
        if rc != code or not all(s in msg for s in (entry, *says)):
            missed.append((entry, change, f"returned {rc}, expected {code}", msg, says))
    assert not missed, "\n".join(map(str, missed))


def test_good_descriptors_pass_the_size_queries(built_lib):
    """The table's starting points are not refused themselves, as far as that shows without a launch:
    the workspace queries validate the same descriptor (pointers apart) and size it."""
    lib = built_lib
    jpeg = _lib.IsrJpegDesc(**ENTRIES["jpeg_roundtrip"][1])
    assert lib.isr_jpeg_roundtrip_workspace_bytes(ctypes.byref(jpeg)) == 2 * 32 * 48 * 3 // 2
    assert lib.isr_jpeg_roundtrip_workspace_bytes(None) == 0
    assert lib.isr_jpeg_roundtrip_workspace_bytes(ctypes.byref(_lib.IsrJpegDesc(1, 24, 32, P, P, P))) == 0
    metrics = _lib.IsrMetricsDesc(**ENTRIES["image_metrics"][1])
    assert lib.isr_image_metrics_workspace_bytes(ctypes.byref(metrics)) > 16
    assert lib.isr_image_metrics_workspace_bytes(None) == 0
