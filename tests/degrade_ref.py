"""numpy restatements of the degradations of image_super_resolution_amd.degrade (csrc/degrade.hip),
written from libjpeg's documented algorithms and the published HLS formulas.  A helper of
test_degrade_cpu.py and test_gpu_degrade.py, not a test module.

JPEG round trip (baseline, 4:2:0, whole MCUs only), the decoded pixels without any entropy coding:
  encode  JFIF RGB -> YCbCr in 16-bit fixed point; h2v2 chroma downsample (4-pixel sum + bias
          1, 2, 1, 2, ... >> 2); level shift; 8x8 DCT-II; IJG tables scaled by the quality;
          quantise, rounding half away from zero
  decode  dequantise; IDCT; + 128, round, clamp; h2v2 "fancy" triangle upsample of the chroma
          planes; fixed-point YCbCr -> RGB.
The coefficients (u, v) in {0, 4}^2 only involve cos(k pi/4): they are integer sums over 8, sit
exactly on quantisation ties in flat regions, and are formed from integers on both transforms.
"""
import numpy as np

LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64).reshape(8, 8)

S4 = np.array([1, -1, -1, 1, 1, -1, -1, 1], dtype=np.int64)  # sign of cos((2x + 1) pi / 4)


def quant_table(base: np.ndarray, quality: int) -> np.ndarray:
    """jpeg_quality_scaling + jpeg_add_quant_table with force_baseline."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def dct_matrix(dtype=np.float64) -> np.ndarray:
    """M[u][x] = C(u)/2 cos((2x + 1) u pi / 16), the orthonormal 8-point DCT-II."""
    u = np.arange(8).reshape(8, 1)
    x = np.arange(8).reshape(1, 8)
    m = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    m[0] *= np.sqrt(0.5)
    return m.astype(dtype)


def _blocks(p: np.ndarray) -> np.ndarray:
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # [by][bx][y][x]


def _unblocks(b: np.ndarray) -> np.ndarray:
    by, bx = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _round_away(x: np.ndarray) -> np.ndarray:
    t = np.trunc(x)
    return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def codec_plane(plane_u8: np.ndarray, table: np.ndarray, dtype=np.float64) -> np.ndarray:
    """One component through DCT, quantisation, dequantisation and IDCT: uint8 in, uint8 out."""
    m = dct_matrix(dtype)
    f = _blocks(plane_u8.astype(np.int64) - 128)
    ff = f.astype(dtype)
    coef = np.einsum("vy,abyx,ux->abvu", m, ff, m).astype(dtype)
    # the four exact coefficients: integer sums / 8
    for v in (0, 4):
        for u in (0, 4):
            sy = S4 if v else np.ones(8, np.int64)
            sx = S4 if u else np.ones(8, np.int64)
            coef[..., v, u] = (np.einsum("y,abyx,x->ab", sy, f, sx).astype(dtype) / dtype(8))
    tq = table.astype(dtype)
    deq = _round_away(coef / tq).astype(np.int64) * table
    exact = np.zeros_like(deq)
    for v in (0, 4):
        for u in (0, 4):
            sy = S4 if v else np.ones(8, np.int64)
            sx = S4 if u else np.ones(8, np.int64)
            exact += deq[..., v, u][..., None, None] * sy.reshape(8, 1) * sx.reshape(1, 8)
    rest = deq.copy()
    rest[..., 0::4, 0::4] = 0
    out = np.einsum("vy,abvu,ux->abyx", m, rest.astype(dtype), m).astype(dtype) + exact.astype(dtype) / dtype(8)
    out = np.floor(out + dtype(128.5))
    return np.clip(_unblocks(out), 0, 255).astype(np.uint8)


def rgb_to_ycc(rgb: np.ndarray):
    """[3][h][w] uint8 -> (Y, Cb, Cr) uint8, libjpeg's jccolor tables (SCALEBITS 16)."""
    r, g, b = (rgb[c].astype(np.int64) for c in range(3))
    half = 1 << 15
    off = 128 << 16
    y = (19595 * r + 38470 * g + 7471 * b + half) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + off + half - 1) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + off + half - 1) >> 16
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def downsample_h2v2(p: np.ndarray) -> np.ndarray:
    q = p.astype(np.int64)
    s = q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2).reshape(1, -1)
    return ((s + bias) >> 2).astype(np.uint8)


def upsample_h2v2_fancy(c: np.ndarray) -> np.ndarray:
    """libjpeg's h2v2_fancy_upsample: 3:1 vertically, then 3:1 horizontally, edges replicated."""
    c = c.astype(np.int64)
    hc, wc = c.shape
    up = np.concatenate([c[:1], c[:-1]])      # the row above, replicated at the top
    dn = np.concatenate([c[1:], c[-1:]])      # the row below
    out = np.empty((2 * hc, 2 * wc), np.int64)
    for dy, far in ((0, up), (1, dn)):
        s = 3 * c + far                        # column sums of one output row
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[dy::2, 0::2] = (3 * s + left + 8) >> 4
        out[dy::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    y = y.astype(np.int64)
    cb = cb.astype(np.int64) - 128
    cr = cr.astype(np.int64) - 128
    half = 1 << 15
    r = y + ((91881 * cr + half) >> 16)
    g = y + ((-22554 * cb + half - 46802 * cr) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.clip(np.stack([r, g, b]), 0, 255).astype(np.uint8)


def jpeg_roundtrip(rgb: np.ndarray, quality: int, dtype=np.float64) -> np.ndarray:
    """[3][h][w] uint8 RGB, h and w multiples of 16; quality 0 returns the image."""
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[0] == 3
    assert rgb.shape[1] % 16 == 0 and rgb.shape[2] % 16 == 0
    if quality == 0:
        return rgb.copy()
    y, cb, cr = rgb_to_ycc(rgb)
    tl, tc = quant_table(LUMA_Q, quality), quant_table(CHROMA_Q, quality)
    y2 = codec_plane(y, tl, dtype)
    cb2 = codec_plane(downsample_h2v2(cb), tc, dtype)
    cr2 = codec_plane(downsample_h2v2(cr), tc, dtype)
    return ycc_to_rgb(y2, upsample_h2v2_fancy(cb2), upsample_h2v2_fancy(cr2))


def jpeg_roundtrip_batch(u8: np.ndarray, qualities, dtype=np.float64) -> np.ndarray:
    return np.stack([jpeg_roundtrip(u8[i], int(q), dtype) for i, q in enumerate(qualities)])


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


# ---- ISO noise ---------------------------------------------------------------------------------

def hls_l_moments(u8: np.ndarray):
    """[n][3][h][w] uint8 -> fp64 [n][2]: mean and population std of L = (max + min) / 510, from
    exact integer sums."""
    out = np.empty((u8.shape[0], 2))
    for i, im in enumerate(u8):
        s = im.max(0).astype(np.int64) + im.min(0).astype(np.int64)
        n = s.size
        s1, s2 = int(s.sum()), int((s * s).sum())
        out[i, 0] = s1 / (510 * n)
        out[i, 1] = np.sqrt((n * s2 - s1 * s1) / (n * n * 510 * 510))
    return out


def iso_noise(rgb: np.ndarray, lum: np.ndarray, hue: np.ndarray, dtype=np.float32) -> np.ndarray:
    """[3][h][w] uint8, lum [h][w] (Poisson counts), hue [h][w] (degrees) -> uint8 [3][h][w].
    Every operation is one rounding in `dtype`, in the order the kernel performs them."""
    f = dtype
    r, g, b = (rgb[c].astype(f) / f(255) for c in range(3))
    vmax = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    sm = vmax + vmin
    d = vmax - vmin
    l = sm * f(0.5)
    grey = d == 0
    dd = np.where(grey, f(1), d)
    s = np.where(l < f(0.5), d / np.where(grey, f(1), sm), d / np.where(grey, f(1), f(2) - sm))
    k = f(60) / dd
    h = np.where(vmax == r, (g - b) * k, np.where(vmax == g, (b - r) * k + f(120), (r - g) * k + f(240)))
    h = np.where(h < 0, h + f(360), h)
    h = np.where(grey, f(0), h)
    s = np.where(grey, f(0), s)

    h = h + hue.astype(f)
    h = np.where(h < 0, h + f(360), h)
    h = np.where(h > f(360), h - f(360), h)
    l = l + (lum.astype(f) / f(255)) * (f(1) - l)

    p2 = np.where(l <= f(0.5), l * (f(1) + s), (l + s) - l * s)
    p1 = f(2) * l - p2
    hh = h * (f(1) / f(60))
    hh = hh - f(6) * np.floor(hh * (f(1) / f(6)))
    sec = np.clip(np.floor(hh), 0, 5)
    fr = hh - sec
    dp = p2 - p1
    t2 = p1 + dp * (f(1) - fr)   # falling
    t3 = p1 + dp * fr            # rising
    sec = sec.astype(np.int64)
    # sector -> (b, g, r) from (p2, p1, falling, rising)
    tab = np.stack([p2, p1, t2, t3])
    bi = np.array([1, 1, 3, 0, 0, 2])[sec]
    gi = np.array([3, 0, 0, 2, 1, 1])[sec]
    ri = np.array([0, 2, 1, 1, 3, 0])[sec]
    pick = lambda idx: np.take_along_axis(tab, idx[None], 0)[0]
    rr, gg, bb = pick(ri), pick(gi), pick(bi)
    flat = s == 0
    rr, gg, bb = (np.where(flat, l, v) for v in (rr, gg, bb))
    out = np.stack([rr, gg, bb]) * f(255)
    return np.trunc(np.clip(out, f(0), f(255))).astype(np.uint8)
