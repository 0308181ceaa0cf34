"""numpy restatement of libisr's blur family (include/isr.h, csrc/blur_taps.h, csrc/blur.hip): the
arithmetic isr_blur_taps / isr_blur_u8 are pinned to, bit for bit.

Taps: fp64 weights on a k x k window (box; rotated anisotropic Gaussian; a Bresenham line), summed
in row-major order and divided by the sum, tap = floor(w * 2^16 + 0.5), the centre tap then takes
2^16 - sum(taps); the window sits in the centre of a 7 x 7 table.  The transcendental functions go
through math.exp / math.cos / math.sin (the C library's, as libisr's do), never numpy's.

Linear filter: acc = sum tap * pixel in integers, out = clip((acc + 2^15) >> 16, 0, 255), border
reflect-101.  Median: the exact median of the k x k window, border replicated.
"""
from __future__ import annotations

import math

import numpy as np

MAX_K = 7
BITS = 16
KINDS = ("box", "gaussian", "motion")


def cv2_sigma(k: int) -> float:
    return 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8


def bresenham(x1: int, y1: int, x2: int, y2: int):
    """The pixels of the integer all-octant Bresenham line, both end points included."""
    dx, dy = abs(x2 - x1), -abs(y2 - y1)
    sx, sy = (1 if x1 < x2 else -1), (1 if y1 < y2 else -1)
    err, x, y, out = dx + dy, x1, y1, []
    while True:
        out.append((x, y))
        if (x, y) == (x2, y2):
            return out
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy


def weights(kind: str, k: int, **p) -> list[list[float]]:
    """The unnormalised fp64 weights of the k x k window, [row][column]."""
    if kind not in KINDS:
        raise ValueError(f"kind {kind!r}")
    if k not in (3, 5, 7):
        raise ValueError(f"ksize {k}")
    c = k // 2
    if kind == "box":
        return [[1.0] * k for _ in range(k)]
    if kind == "gaussian":
        sx, sy, a = float(p.get("sigma_x", 0.0)), float(p.get("sigma_y", 0.0)), float(p.get("angle", 0.0))
        sx = cv2_sigma(k) if sx <= 0.0 else sx
        sy = cv2_sigma(k) if sy <= 0.0 else sy
        ca, sa = math.cos(a), math.sin(a)
        w = [[0.0] * k for _ in range(k)]
        for y in range(k):
            for x in range(k):
                dx, dy = float(x - c), float(y - c)
                u, v = (dx * ca + dy * sa) / sx, (dy * ca - dx * sa) / sy
                w[y][x] = math.exp(-0.5 * (u * u + v * v))
        return w
    x1, y1, x2, y2 = (p[n] for n in ("x1", "y1", "x2", "y2"))
    if any(int(v) != v or not 0 <= v <= k - 1 for v in (x1, y1, x2, y2)):
        raise ValueError("end points outside the grid")
    if (x1, y1) == (x2, y2):
        raise ValueError("end points equal")
    w = [[0.0] * k for _ in range(k)]
    for x, y in bresenham(int(x1), int(y1), int(x2), int(y2)):
        w[y][x] = 1.0
    return w


def taps(kind: str, k: int, **p) -> np.ndarray:
    """int32 [7, 7]: the table isr_blur_taps makes."""
    w = [v for row in weights(kind, k, **p) for v in row]
    s = 0.0
    for v in w:
        s += v
    t = [int(math.floor(v / s * float(1 << BITS) + 0.5)) for v in w]
    c = (k // 2) * k + k // 2
    t[c] += (1 << BITS) - sum(t)
    if t[c] < 0:
        raise ValueError("negative centre tap")
    out = np.zeros((MAX_K, MAX_K), dtype=np.int32)
    o = (MAX_K - k) // 2
    out[o:o + k, o:o + k] = np.array(t, dtype=np.int32).reshape(k, k)
    return out


def normalized(kind: str, k: int, **p) -> np.ndarray:
    """fp64 [k, k]: the normalised weights before rounding (for the comparison with scipy)."""
    w = np.array(weights(kind, k, **p), dtype=np.float64)
    return w / w.sum()


def _windows(img: np.ndarray, k: int, mode: str):
    """The k * k shifted views of uint8 [..., h, w] under the border `mode` of np.pad."""
    r = k // 2
    h, w = img.shape[-2:]
    pad = np.pad(img, [(0, 0)] * (img.ndim - 2) + [(r, r), (r, r)], mode=mode)
    for dy in range(k):
        for dx in range(k):
            yield dy, dx, pad[..., dy:dy + h, dx:dx + w]


def filter_sums(img: np.ndarray, table: np.ndarray, k: int = MAX_K) -> np.ndarray:
    """int64 [..., h, w]: sum tap * pixel over the centre k x k of the 7 x 7 `table`, reflect-101."""
    o = (MAX_K - k) // 2
    acc = np.zeros(img.shape, dtype=np.int64)
    for dy, dx, v in _windows(img, k, "reflect"):
        acc += int(table[o + dy, o + dx]) * v.astype(np.int64)
    return acc


def filter_u8(img: np.ndarray, table: np.ndarray, k: int = MAX_K) -> np.ndarray:
    return np.clip((filter_sums(img, table, k) + (1 << (BITS - 1))) >> BITS, 0, 255).astype(np.uint8)


def median_u8(img: np.ndarray, k: int) -> np.ndarray:
    stack = np.stack([v for _, _, v in _windows(img, k, "edge")])
    return np.sort(stack, axis=0)[k * k // 2]


def blur_u8(img: np.ndarray, ksize, median, tables) -> np.ndarray:
    """The mixed launch on uint8 [n, 3, h, w]: per image ksize, median flag and 7 x 7 table."""
    out = np.empty_like(img)
    for i in range(img.shape[0]):
        k = int(ksize[i])
        if k not in (3, 5, 7):
            out[i] = img[i]
        elif median[i]:
            out[i] = median_u8(img[i], k)
        else:
            out[i] = filter_u8(img[i], tables[i], k)
    return out
