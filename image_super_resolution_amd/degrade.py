"""Training-data degradations on the device (libisr's csrc/degrade.hip, include/isr.h): the JPEG
round trip and the ISO noise of the reference's Noisy_dataset (utils/datasets.py:374-377,
albumentations ImageCompression and ISONoise), on uint8 [n, 3, h, w] RGB crops that are already on
the GPU.  Nothing here synchronises with the host: per-image qualities and apply flags are device
tensors, and a quality of 0 / an apply flag of 0 copies the image through.

`resample_u8` is Pillow's Image.resize (antialiased bicubic ... nearest) on such a batch, bit for
bit: the LR models of the reference's Random_low_rs and image_reader (utils/datasets.py:23-32,
:218-246).  Its coefficient tables are made on the host by libisr (`resample_tables`, plain C++).

`blur_u8` (with `filter_u8`, `median_u8`) is the blur family the reference lists, commented out,
ahead of SR_dataset's Resize (utils/datasets.py:291-305: Blur, GaussianBlur, MotionBlur,
MedianBlur): an integer k x k correlation with 16-bit fixed-point taps (`blur_taps`, made on the host
by libisr) or the exact k x k median, k in {3, 5, 7} per image; data.LRDegrade chains it with the
two above and GaussNoise for the blind-SR LR model.

GPU-only, like the rest of the product path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .ops import _stream


def _checked(u8: torch.Tensor, what: str, on_device: bool = True) -> torch.Tensor:
    """The uint8 [n, 3, h, w] batch check of everything here and of data.py's transforms (`what` names the
    caller); with on_device the batch must also be on a HIP device.  Returns it contiguous."""
    if on_device and not (isinstance(u8, torch.Tensor) and u8.is_cuda):
        raise RuntimeError(f"{what}: the input must be a HIP device tensor (the degradations run on the MI355X HIP "
                           f"path only; got {getattr(u8, 'device', type(u8))})")
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[1] != 3:
        raise ValueError(f"{what}: expected uint8 [n, 3, h, w], got {getattr(u8, 'dtype', type(u8))} "
                         f"{tuple(getattr(u8, 'shape', ()))}")
    return u8.contiguous()


def _per_image(v, n: int, dtype, device, what: str) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        if v.numel() != n:
            raise ValueError(f"{what}: expected {n} values, got {tuple(v.shape)}")
        return v.to(device=device, dtype=dtype).reshape(n).contiguous()
    return torch.full((n,), v, dtype=dtype, device=device)


def _per_image_ints(v, n: int, device, what: str, host_range=None) -> torch.Tensor:
    """Device int32 [n] from an int (Python or numpy), an int sequence or an integer tensor [n]; float and
    bool tensors are refused.  A device tensor stays on the device and is never read back, so `host_range`
    = (lo, hi) bounds only what is on the host.  n None: the checks alone (jpeg_roundtrip's come first)."""
    bad = False
    if isinstance(v, torch.Tensor):
        if v.is_floating_point() or v.dtype == torch.bool:
            raise ValueError(f"{what} must be an integer tensor, got {v.dtype}")
    elif np.ndim(v):
        v = torch.tensor([int(k) for k in v], dtype=torch.int32)
    else:
        bad = int(v) != v
        v = v if bad else int(v)
    if host_range is not None and not bad:
        if not isinstance(v, torch.Tensor):
            bad = not host_range[0] <= v <= host_range[1]
        elif not v.is_cuda and v.numel():
            bad = not host_range[0] <= int(v.min()) <= int(v.max()) <= host_range[1]
    if bad:
        raise ValueError(f"{what} must be an integer" + ("" if host_range is None else " in {}..{}".format(*host_range)) +
                         f", got {v}")
    return v if n is None else _per_image(v, n, torch.int32, device, what)


def jpeg_roundtrip(u8: torch.Tensor, quality) -> torch.Tensor:
    """The decoded pixels of a baseline 4:2:0 JPEG of every image (libjpeg's arithmetic with an
    fp32 DCT; no entropy coding happens).  `quality`: an int, or an int tensor [n] (kept on the
    device); 1..100, and 0 returns that image unchanged.  h and w must be multiples of 16."""
    # a host quality is checked here; a device one is clamped by the kernel
    quality = _per_image_ints(quality, None, None, "jpeg_roundtrip: quality", host_range=(0, 100))
    x = _checked(u8, "jpeg_roundtrip")
    n, _, h, w = x.shape
    lib = _lib.load()
    with torch.cuda.device(x.device):
        q = _per_image(quality, n, torch.int32, x.device, "jpeg_roundtrip: quality")
        out = torch.empty_like(x)
        d = _lib.IsrJpegDesc(n, h, w, x.data_ptr(), out.data_ptr(), q.data_ptr())
        nbytes = lib.isr_jpeg_roundtrip_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            raise _lib.IsrError("isr_jpeg_roundtrip refused the descriptor: " +
                                lib.isr_last_error().decode(errors="replace"))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.isr_jpeg_roundtrip(ctypes.byref(d), ws.data_ptr(), nbytes, _stream()), "isr_jpeg_roundtrip")
    return out


def hls_l_moments(u8: torch.Tensor) -> torch.Tensor:
    """fp64 [n, 2]: mean and population standard deviation of the HLS lightness
    L = (max + min) / 2 of every image on the [0, 1] scale, from exact integer sums."""
    x = _checked(u8, "hls_l_moments")
    n, _, h, w = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty((n, 2), dtype=torch.float64, device=x.device)
        part = torch.empty((n, _lib.HLS_PARTIAL_BLOCKS, 2), dtype=torch.int64, device=x.device)
        d = _lib.IsrHlsMomentsDesc(n, h, w, x.data_ptr(), out.data_ptr(), part.data_ptr())
        _lib.check(_lib.load().isr_hls_l_moments(ctypes.byref(d), _stream()), "isr_hls_l_moments")
    return out


def iso_noise_planes(u8: torch.Tensor, lum_noise: torch.Tensor, hue_noise: torch.Tensor,
                     apply: torch.Tensor | None = None) -> torch.Tensor:
    """isr_iso_noise with the two noise planes given: fp32 [n, h, w] Poisson counts and degrees."""
    x = _checked(u8, "iso_noise")
    n, _, h, w = x.shape
    for name, t in (("lum_noise", lum_noise), ("hue_noise", hue_noise)):
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (n, h, w):
            raise ValueError(f"iso_noise: {name} must be a device fp32 [{n}, {h}, {w}] tensor, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    with torch.cuda.device(x.device):
        a = _per_image(1 if apply is None else apply, n, torch.int32, x.device, "iso_noise: apply")
        lum, hue = lum_noise.contiguous(), hue_noise.contiguous()
        out = torch.empty_like(x)
        d = _lib.IsrIsoNoiseDesc(n, h, w, x.data_ptr(), out.data_ptr(), lum.data_ptr(), hue.data_ptr(), a.data_ptr())
        _lib.check(_lib.load().isr_iso_noise(ctypes.byref(d), _stream()), "isr_iso_noise")
    return out


def iso_noise(u8: torch.Tensor, color_shift, intensity, generator: torch.Generator | None,
              apply: torch.Tensor | None = None) -> torch.Tensor:
    """albumentations' ISONoise: per image, Poisson luminance noise of rate
    std(L) * intensity * 255 (L the HLS lightness in [0, 1]) scaled into the headroom 1 - L, and
    Gaussian hue noise of sigma color_shift * 360 * intensity degrees.  `color_shift` and
    `intensity` are floats or tensors [n]; `apply` ([n], optional) selects the images that are
    changed.  The rates stay on the device; the draws come from `generator`."""
    x = _checked(u8, "iso_noise")
    n, _, h, w = x.shape
    with torch.cuda.device(x.device):
        cs = _per_image(color_shift, n, torch.float32, x.device, "iso_noise: color_shift")
        it = _per_image(intensity, n, torch.float32, x.device, "iso_noise: intensity")
        lam = (hls_l_moments(x)[:, 1] * it.double() * 255.0).float()
        lum = torch.poisson(lam.view(n, 1, 1).expand(n, h, w).contiguous(), generator=generator)
        hue = torch.randn((n, h, w), device=x.device, generator=generator) * (cs * 360.0 * it).view(n, 1, 1)
        return iso_noise_planes(x, lum, hue, apply)


RESAMPLE_FILTERS = ("nearest", "box", "bilinear", "hamming", "bicubic", "lanczos")  # index = ISR_RESAMPLE_*


def _filter_index(f) -> int:
    if isinstance(f, str):
        if f not in RESAMPLE_FILTERS:
            raise ValueError(f"resample: unknown filter {f!r}; one of {', '.join(RESAMPLE_FILTERS)}")
        return RESAMPLE_FILTERS.index(f)
    if int(f) != f or not 0 <= int(f) < len(RESAMPLE_FILTERS):
        raise ValueError(f"resample: filter id {f!r} not in 0..{len(RESAMPLE_FILTERS) - 1}")
    return int(f)


def resample_tables(filter, in_size: int, out_size: int):
    """Pillow's coefficient table of one axis from libisr's host code (no GPU): numpy int32
    bounds [out_size, 2] = (first source index, tap count) and coeffs [out_size, ksize] (22
    fractional bits, rows zero-padded).  `filter`: a name of RESAMPLE_FILTERS or its index."""
    f, lib = _filter_index(filter), _lib.load()
    in_size, out_size = int(in_size), int(out_size)
    ks = lib.isr_resample_ksize(f, in_size, out_size)
    if ks <= 0:
        raise _lib.IsrError("isr_resample_ksize refused: " + lib.isr_last_error().decode(errors="replace"))
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ks), dtype=np.int32)
    _lib.check(lib.isr_resample_tables(f, in_size, out_size, bounds.ctypes.data, coeffs.ctypes.data),
               "isr_resample_tables")
    return bounds, coeffs


_resample_cache: dict = {}


def _device_tables(device: torch.device, in_size: int, out_size: int, filters: tuple):
    """(bounds [nf, out, 2], coeffs [nf, out, ksize], ksize) on `device` for the filter variants
    `filters` (indices), padded to their common ksize; cached per (device, in, out, filters)."""
    key = (device.type, device.index, in_size, out_size, filters)
    hit = _resample_cache.get(key)
    if hit is None:
        tabs = [resample_tables(f, in_size, out_size) for f in filters]
        ks = max(c.shape[1] for _, c in tabs)
        bounds = np.stack([b for b, _ in tabs])
        coeffs = np.zeros((len(tabs), out_size, ks), dtype=np.int32)
        for i, (_, c) in enumerate(tabs):
            coeffs[i, :, :c.shape[1]] = c
        hit = (torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device), ks)
        _resample_cache[key] = hit
    return hit


def resample_launch(x: torch.Tensor, size, filters: tuple, filter_id: torch.Tensor | None, *, want_u8: bool = False,
                    want_lr: bool = False, want_hr: bool = False, hr_norm: bool = False, mean=(0.0, 0.0, 0.0),
                    std=(1.0, 1.0, 1.0)):
    """One isr_resample_u8 launch on a checked uint8 [n, 3, h, w] device batch: returns
    (dst_u8, lr_f32, hr_f32), None for what was not asked for.  `filters`: the variants' filter
    indices; `filter_id`: device int32 [n] picking a variant per image, or None for variant 0."""
    n, _, h, w = x.shape
    oh, ow = (int(v) for v in size)
    with torch.cuda.device(x.device):
        bx, cx, ksx = _device_tables(x.device, w, ow, filters)
        by, cy, ksy = _device_tables(x.device, h, oh, filters)
        dst = torch.empty((n, 3, oh, ow), dtype=torch.uint8, device=x.device) if want_u8 else None
        lr = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=x.device) if want_lr else None
        hr = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device) if want_hr else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        d = _lib.IsrResampleDesc(n, h, w, oh, ow, len(filters), ksx, ksy, x.data_ptr(), bx.data_ptr(), cx.data_ptr(),
                                 by.data_ptr(), cy.data_ptr(), ptr(filter_id), ptr(dst), ptr(lr), ptr(hr),
                                 int(hr_norm), (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std))
        _lib.check(_lib.load().isr_resample_u8(ctypes.byref(d), _stream()), "isr_resample_u8")
    return dst, lr, hr


def resample_u8(u8: torch.Tensor, size, filter="bicubic") -> torch.Tensor:
    """Pillow's Image.resize of every image to size = (h, w), bit for bit (two int32 passes with a
    uint8 image between them; antialiased on a downscale).  `filter`: a name of RESAMPLE_FILTERS
    for the whole batch, or an int tensor / sequence [n] of per-image indices into it (a device
    tensor stays on the device; the kernel clamps ids to 0..5).  Each axis' ratio must lie in
    [1/8, 8]."""
    x = _checked(u8, "resample_u8")
    n = x.shape[0]
    if isinstance(filter, (str, int)):
        return resample_launch(x, size, (_filter_index(filter),), None, want_u8=True)[0]
    with torch.cuda.device(x.device):
        ids = _per_image_ints(filter, n, x.device, "resample_u8: filter ids")
    return resample_launch(x, size, tuple(range(len(RESAMPLE_FILTERS))), ids, want_u8=True)[0]


BLUR_KINDS = ("box", "gaussian", "motion")  # index = ISR_BLUR_*
BLUR_MAX_K = 7
_BLUR_PARAMS = {"box": (), "gaussian": ("sigma_x", "sigma_y", "angle"), "motion": ("x1", "y1", "x2", "y2")}


def blur_taps(kind, ksize: int, **params) -> np.ndarray:
    """A 7 x 7 tap table from libisr's host code (isr_blur_taps, no GPU): numpy int32, 16
    fractional bits, the ksize x ksize window (3, 5 or 7) in the centre, summing to exactly 65536.
    `kind`: "box"; "gaussian" with sigma_x, sigma_y (<= 0 or absent: cv2's rule for the ksize)
    and angle in radians (default 0); "motion" with the integer end points x1, y1, x2, y2 of a
    Bresenham line inside the window."""
    if isinstance(kind, str):
        if kind not in BLUR_KINDS:
            raise ValueError(f"blur_taps: unknown kind {kind!r}; one of {', '.join(BLUR_KINDS)}")
        kind = BLUR_KINDS.index(kind)
    name = BLUR_KINDS[kind] if 0 <= int(kind) < len(BLUR_KINDS) else None
    names = _BLUR_PARAMS.get(name, ())
    extra = sorted(set(params) - set(names))
    if extra:
        raise ValueError(f"blur_taps: {name} takes no parameter {', '.join(extra)}")
    if name == "motion" and len(params) != 4:
        raise ValueError("blur_taps: motion needs x1, y1, x2 and y2")
    vals = (ctypes.c_double * 4)(*[float(params.get(n, 0.0)) for n in names])
    taps = np.zeros((BLUR_MAX_K, BLUR_MAX_K), dtype=np.int32)
    _lib.check(_lib.load().isr_blur_taps(int(kind), int(ksize), ctypes.cast(vals, ctypes.c_void_p), taps.ctypes.data),
               "isr_blur_taps")
    return taps


def _blur_tables(taps, n: int, device) -> torch.Tensor:
    """int32 [n, 49] on `device` from a [7, 7] table for the whole batch or [n, 7, 7] per image."""
    t = torch.from_numpy(np.ascontiguousarray(taps)) if isinstance(taps, np.ndarray) else taps
    if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError("blur: taps must be an integer array or tensor")
    if tuple(t.shape) == (BLUR_MAX_K, BLUR_MAX_K):
        t = t.unsqueeze(0).expand(n, -1, -1)
    if tuple(t.shape) != (n, BLUR_MAX_K, BLUR_MAX_K):
        raise ValueError(f"blur: taps must be [7, 7] or [{n}, 7, 7], got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.int32, non_blocking=True).reshape(n, BLUR_MAX_K * BLUR_MAX_K).contiguous()


def blur_u8(u8: torch.Tensor, ksize, median, taps) -> torch.Tensor:
    """One isr_blur_u8 launch on uint8 [n, 3, h, w] (h, w >= 7): per image, `ksize` 3, 5 or 7 (any
    other value copies the image through), `median` non-zero for the exact k x k median (border
    replicated), else the correlation with the centre k x k of the image's 7 x 7 `taps` (16
    fractional bits, border reflect-101, rounded half up and clipped).  ksize and median: an int or
    an int sequence / tensor [n]; taps: int32 [7, 7] or [n, 7, 7]; numpy, host or device tensors
    (device tensors stay on the device; nothing is read back)."""
    x = _checked(u8, "blur_u8")
    n, _, h, w = x.shape
    with torch.cuda.device(x.device):
        k = _per_image_ints(ksize, n, x.device, "blur_u8: ksize")
        m = _per_image_ints(median, n, x.device, "blur_u8: median")
        t = _blur_tables(taps, n, x.device)
        out = torch.empty_like(x)
        d = _lib.IsrBlurDesc(n, h, w, x.data_ptr(), out.data_ptr(), k.data_ptr(), m.data_ptr(), t.data_ptr())
        _lib.check(_lib.load().isr_blur_u8(ctypes.byref(d), _stream()), "isr_blur_u8")
    return out


def filter_u8(u8: torch.Tensor, taps, ksize=None) -> torch.Tensor:
    """The integer correlation of every image with `taps` (blur_taps' tables, or any int32 table with
    sum |tap| <= 2^23, negative taps included).  `ksize` (default 7) bounds the window that is read;
    zero taps inside it cost time, not accuracy."""
    return blur_u8(u8, BLUR_MAX_K if ksize is None else ksize, 0, taps)


_zero_taps = np.zeros((BLUR_MAX_K, BLUR_MAX_K), dtype=np.int32)


def median_u8(u8: torch.Tensor, ksize) -> torch.Tensor:
    """The exact ksize x ksize median of every image, border replicated (cv2.medianBlur, Pillow's
    MedianFilter).  `ksize`: 3, 5 or 7, an int or an int tensor [n]; 0 copies that image through."""
    return blur_u8(u8, ksize, 1, _zero_taps)
