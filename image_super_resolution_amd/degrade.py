"""Training-data degradations on the device (libisr's csrc/degrade.hip, include/isr.h): the JPEG
round trip and the ISO noise of the reference's Noisy_dataset (utils/datasets.py:374-377,
albumentations ImageCompression and ISONoise), on uint8 [n, 3, h, w] RGB crops that are already on
the GPU.  Nothing here synchronises with the host: per-image qualities and apply flags are device
tensors, and a quality of 0 / an apply flag of 0 copies the image through.

GPU-only, like the rest of the product path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ops import _stream


def _checked(u8: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(u8, torch.Tensor) or not u8.is_cuda:
        raise RuntimeError(f"{what}: the input must be a HIP device tensor (the degradations run on the MI355X HIP "
                           f"path only; got {getattr(u8, 'device', type(u8))})")
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[1] != 3:
        raise ValueError(f"{what}: expected uint8 [n, 3, h, w], got {u8.dtype} {tuple(u8.shape)}")
    return u8.contiguous()


def _per_image(v, n: int, dtype, device, what: str) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        if v.numel() != n:
            raise ValueError(f"{what}: expected {n} values, got {tuple(v.shape)}")
        return v.to(device=device, dtype=dtype).reshape(n).contiguous()
    return torch.full((n,), v, dtype=dtype, device=device)


def jpeg_roundtrip(u8: torch.Tensor, quality) -> torch.Tensor:
    """The decoded pixels of a baseline 4:2:0 JPEG of every image (libjpeg's arithmetic with an
    fp32 DCT; no entropy coding happens).  `quality`: an int, or an int tensor [n] (kept on the
    device); 1..100, and 0 returns that image unchanged.  h and w must be multiples of 16."""
    if isinstance(quality, torch.Tensor):
        if quality.is_floating_point() or quality.dtype == torch.bool:
            raise ValueError(f"jpeg_roundtrip: quality must be an integer tensor, got {quality.dtype}")
        if not quality.is_cuda:  # a host tensor is checked here; a device one is clamped by the kernel
            if quality.numel() and (int(quality.min()) < 0 or int(quality.max()) > 100):
                raise ValueError("jpeg_roundtrip: quality must be in 0..100 (0 = copy through)")
    else:
        if int(quality) != quality or not 0 <= int(quality) <= 100:
            raise ValueError(f"jpeg_roundtrip: quality must be an integer in 0..100 (0 = copy through), got {quality}")
        quality = int(quality)
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
