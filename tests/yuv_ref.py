"""Numpy restatement of the YUV 4:2:0 arithmetic of include/isr.h (not collected): the integer
arithmetic isr_yuv_coeffs / isr_rgb_to_yuv420_u8 / isr_yuv420_to_rgb_u8 are pinned to, bit for
bit, in int64, and an fp64 "exact" version of the same filters and matrices with no rounding before
the end (what the integer version is measured against)."""
import math

import numpy as np

BITS = 16
ONE = 1 << BITS
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}  # index = ISR_YUV_BT601 / BT709
LAYOUTS = ("i420", "nv12")     # index = ISR_YUV_I420 / NV12
SITINGS = ("left", "center")   # index = ISR_YUV_SITING_LEFT / CENTER


def fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def scales(full_range):
    """(sy, sc, oy)"""
    return (1.0, 1.0, 0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16)


def real_coeffs(matrix, full_range):
    """The exact (fp64) forward 3 x 3 and inverse (cy, crv, cbu, cgu, cgv)."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, _ = scales(full_range)
    db, dr = 2.0 * (1.0 - kb), 2.0 * (1.0 - kr)
    fwd = np.array([[sy * kr, sy * kg, sy * kb],
                    [sc * -kr / db, sc * -kg / db, sc * (1.0 - kb) / db],
                    [sc * (1.0 - kr) / dr, sc * -kg / dr, sc * -kb / dr]])
    crv, cbu = dr / sc, db / sc
    return fwd, (1.0 / sy, crv, cbu, -cbu * kb / kg, -crv * kr / kg)


def coeffs(matrix, full_range):
    """(fwd int64 [3, 3], inv int64 [5]) as isr_yuv_coeffs makes them."""
    f, v = real_coeffs(matrix, full_range)
    sy, _, _ = scales(full_range)
    fwd = np.zeros((3, 3), dtype=np.int64)
    for r in range(3):
        fwd[r, 0], fwd[r, 2] = fix(f[r, 0]), fix(f[r, 2])
        fwd[r, 1] = (fix(sy) if r == 0 else 0) - fwd[r, 0] - fwd[r, 2]
    return fwd, np.array([fix(c) for c in v], dtype=np.int64)


def frame_bytes(h, w):
    return 3 * h * w // 2


def check_size(h, w):
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"4:2:0 needs even h, w >= 2, got {h}x{w}")


# ------------------------------------------------------------------------------- frame layout
def pack(y, u, v, layout):
    """planes [n, h, w], [n, h/2, w/2] x 2 -> uint8 [n, 3 h w / 2]"""
    n = y.shape[0]
    if layout == "i420":
        return np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1).astype(np.uint8)
    uv = np.stack([u, v], axis=-1)
    return np.concatenate([y.reshape(n, -1), uv.reshape(n, -1)], axis=1).astype(np.uint8)


def unpack(frames, h, w, layout):
    """uint8 [n, 3 h w / 2] -> (y, u, v)"""
    check_size(h, w)
    f = np.asarray(frames).reshape(-1, frame_bytes(h, w))
    n = f.shape[0]
    y = f[:, :h * w].reshape(n, h, w)
    if layout == "i420":
        q = h * w // 4
        return y, f[:, h * w:h * w + q].reshape(n, h // 2, w // 2), f[:, h * w + q:].reshape(n, h // 2, w // 2)
    uv = f[:, h * w:].reshape(n, h // 2, w // 2, 2)
    return y, uv[..., 0], uv[..., 1]


# ------------------------------------------------------------------------------- the filters
def _shift(a, d, axis):
    """a[k + d] along `axis` with the edge replicated."""
    n = a.shape[axis]
    return np.take(a, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def chroma_sums(p, siting):
    """Footprint sums of planes [..., h, w] -> ([..., h/2, w/2], D); any numeric dtype."""
    rows = p[..., 0::2, :] + p[..., 1::2, :]
    if siting == "center":
        return rows[..., 0::2] + rows[..., 1::2], 4
    return _shift(rows, -1, -1)[..., 0::2] + 2 * rows[..., 0::2] + rows[..., 1::2], 8


def chroma_up(c, siting):
    """Chroma planes [..., h/2, w/2] -> numerators [..., h, w] and D."""
    hc, wc = c.shape[-2:]
    H = np.zeros(c.shape[:-1] + (2 * wc,), dtype=c.dtype)
    if siting == "left":
        H[..., 0::2] = 2 * c
        H[..., 1::2] = c + _shift(c, 1, -1)
    else:
        H[..., 0::2] = 3 * c + _shift(c, -1, -1)
        H[..., 1::2] = 3 * c + _shift(c, 1, -1)
    V = np.zeros(c.shape[:-2] + (2 * hc, 2 * wc), dtype=c.dtype)
    V[..., 0::2, :] = 3 * H + _shift(H, -1, -2)
    V[..., 1::2, :] = 3 * H + _shift(H, 1, -2)
    return V, (8 if siting == "left" else 16)


# ------------------------------------------------------------------------------- integer
def rgb_to_yuv420(rgb, matrix="bt709", full_range=False, siting="left", layout="i420"):
    """uint8 [n, 3, h, w] -> uint8 [n, 3 h w / 2]"""
    rgb = np.asarray(rgb).astype(np.int64)
    check_size(*rgb.shape[-2:])
    fwd, _ = coeffs(matrix, full_range)
    oy = scales(full_range)[2]
    y = np.clip((np.tensordot(fwd[0], rgb, ([0], [1])) + oy * ONE + ONE // 2) >> BITS, 0, 255)
    S, D = chroma_sums(rgb, siting)
    sh = BITS + int(math.log2(D))
    u = np.clip((np.tensordot(fwd[1], S, ([0], [1])) + 128 * ONE * D + (ONE // 2) * D) >> sh, 0, 255)
    v = np.clip((np.tensordot(fwd[2], S, ([0], [1])) + 128 * ONE * D + (ONE // 2) * D) >> sh, 0, 255)
    return pack(y, u, v, layout)


def yuv420_to_rgb(frames, h, w, matrix="bt709", full_range=False, siting="left", layout="i420"):
    """uint8 [n, 3 h w / 2] -> uint8 [n, 3, h, w]"""
    y, u, v = (p.astype(np.int64) for p in unpack(frames, h, w, layout))
    _, (cy, crv, cbu, cgu, cgv) = coeffs(matrix, full_range)
    oy = scales(full_range)[2]
    U, D = chroma_up(u, siting)
    V, _ = chroma_up(v, siting)
    sh = BITS + int(math.log2(D))
    base = cy * D * (y - oy) + (ONE // 2) * D
    U, V = U - 128 * D, V - 128 * D
    r = (base + crv * V) >> sh
    g = (base + cgu * U + cgv * V) >> sh
    b = (base + cbu * U) >> sh
    return np.clip(np.stack([r, g, b], axis=1), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------- exact (fp64)
def rgb_to_yuv420_exact(rgb, matrix="bt709", full_range=False, siting="left"):
    """fp64 planes (y [n, h, w], u, v [n, h/2, w/2]) before rounding and clamping."""
    rgb = np.asarray(rgb).astype(np.float64)
    fwd, _ = real_coeffs(matrix, full_range)
    oy = scales(full_range)[2]
    y = np.tensordot(fwd[0], rgb, ([0], [1])) + oy
    S, D = chroma_sums(rgb, siting)
    return y, np.tensordot(fwd[1], S / D, ([0], [1])) + 128.0, np.tensordot(fwd[2], S / D, ([0], [1])) + 128.0


def yuv420_to_rgb_exact(frames, h, w, matrix="bt709", full_range=False, siting="left", layout="i420"):
    """fp64 [n, 3, h, w] before rounding and clamping."""
    y, u, v = (p.astype(np.float64) for p in unpack(frames, h, w, layout))
    _, (cy, crv, cbu, cgu, cgv) = real_coeffs(matrix, full_range)
    oy = scales(full_range)[2]
    U, D = chroma_up(u, siting)
    V, _ = chroma_up(v, siting)
    U, V = U / D - 128.0, V / D - 128.0
    base = cy * (y - oy)
    return np.stack([base + crv * V, base + cgu * U + cgv * V, base + cbu * U], axis=1)


def round_clamp(x):
    return np.clip(np.floor(x + 0.5), 0, 255)
