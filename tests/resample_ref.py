"""numpy restatement of Pillow's 8-bit resampler (Imaging/Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) and of its nearest rule:
the arithmetic libisr's isr_resample_tables / isr_resample_u8 are pinned to, bit for bit.

Two separable passes, horizontal first, with a uint8 image between them.  Each pass accumulates
pixel * k in 32-bit integers, k the normalised double weight rounded to 22 fractional bits; the
accumulator starts at 1 << 21, is shifted right by 22 and clipped to 0..255.  On a downscale the
filter's support is scaled by the ratio (the antialiasing); the taps are clamped at the image
edge and the shortened kernel renormalised.  The transcendental filters go through math.sin /
math.cos (the C library's, as Pillow's and libisr's do), never numpy's vectorised ones.
"""
from __future__ import annotations

import math

import numpy as np

FILTERS = ("nearest", "box", "bilinear", "hamming", "bicubic", "lanczos")
PRECISION_BITS = 32 - 8 - 2
SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def weight(name: str, x: float) -> float:
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    if x < 0.0:
        x = -x
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    if name == "hamming":
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))
    if name == "bicubic":
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    raise ValueError(name)


def ksize(name: str, in_size: int, out_size: int) -> int:
    if name == "nearest":
        return 1
    filterscale = max(in_size / out_size, 1.0)
    return int(math.ceil(SUPPORT[name] * filterscale)) * 2 + 1


def tables(name: str, in_size: int, out_size: int):
    """(bounds int32 [out, 2] = first, count; coeffs int32 [out, ksize], rows zero-padded)."""
    ks = ksize(name, in_size, out_size)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ks), dtype=np.int32)
    if name == "nearest":
        # src = floor((dst + 0.5) * in / out), in the form Pillow's ImagingScaleAffine computes it:
        # the source coordinate starts at half a step and is advanced by repeated addition, so a
        # product that would land exactly on an integer (2 -> 7 at dst 3) can fall just below it
        step = in_size / out_size
        xo = step * 0.5
        for xx in range(out_size):
            bounds[xx] = (min(int(xo), in_size - 1), 1)
            coeffs[xx, 0] = 1 << PRECISION_BITS
            xo += step
        return bounds, coeffs
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[name] * filterscale
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [weight(name, (x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        bounds[xx] = (xmin, xmax)
        for x, w in enumerate(k):
            coeffs[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
    return bounds, coeffs


def _sums(img: np.ndarray, bounds: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """The unclipped accumulators of one pass along the last axis: int64 [..., out]."""
    x = img.astype(np.int64)
    out = np.empty(img.shape[:-1] + (bounds.shape[0],), dtype=np.int64)
    for xx, (first, count) in enumerate(bounds):
        out[..., xx] = (1 << (PRECISION_BITS - 1)) + x[..., first:first + count] @ coeffs[xx, :count].astype(np.int64)
    return out


def _clip8(sums: np.ndarray) -> np.ndarray:
    return np.clip(sums >> PRECISION_BITS, 0, 255).astype(np.uint8)


def apply_tables(img: np.ndarray, tx, ty, return_sums: bool = False):
    """Both passes on uint8 [..., h, w] with (bounds, coeffs) pairs per axis."""
    sx = _sums(img, *tx)
    mid = _clip8(sx)
    sy = _sums(np.swapaxes(mid, -1, -2), *ty)
    out = np.ascontiguousarray(np.swapaxes(_clip8(sy), -1, -2))
    return (out, sx, sy) if return_sums else out


def resize(img: np.ndarray, size, name: str, return_sums: bool = False):
    """Image.resize of uint8 [..., h, w] planes to size = (out_h, out_w)."""
    h, w = img.shape[-2:]
    return apply_tables(img, tables(name, w, size[1]), tables(name, h, size[0]), return_sums)


def normalize(u8: np.ndarray, mean, std) -> np.ndarray:
    """albumentations' Normalize of uint8 [n, 3, h, w], as tests/test_gpu_data.py states it."""
    mean = np.array(mean, dtype=np.float32).reshape(1, 3, 1, 1)
    std = np.array(std, dtype=np.float32).reshape(1, 3, 1, 1)
    return (u8.astype(np.float32) - mean * 255.0) * (1.0 / (std * 255.0))
