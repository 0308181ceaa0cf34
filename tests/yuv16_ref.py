"""Numpy restatement of the 10-bit YUV 4:2:0 arithmetic of include/isr.h (not collected): what
isr_yuv_coeffs_depth / isr_rgb_to_yuv420_16 / isr_yuv420_to_rgb_16 are pinned to, bit for bit, in int64
and fp32, and an fp64 "exact" version of the same filters and matrices with no rounding before the end.
The filters are yuv_ref's; frames are byte arrays of little-endian 16-bit words, the sample at bit
`shift` of its word."""
import math

import numpy as np

import yuv_ref as Y

BITS, ONE = Y.BITS, Y.ONE
MATRICES, LAYOUTS, SITINGS = Y.MATRICES, Y.LAYOUTS, Y.SITINGS
fix = Y.fix


def top(depth):
    return (1 << depth) - 1


def scales(full_range, depth=10):
    """(sy, sc, oy)"""
    if full_range:
        return 1.0, 1.0, 0
    up = float(1 << (depth - 8))
    return 219.0 * up / top(depth), 224.0 * up / top(depth), 16 << (depth - 8)


def real_coeffs(matrix, full_range, depth=10):
    """The exact (fp64) forward 3 x 3 and inverse (cy, crv, cbu, cgu, cgv)."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, _ = scales(full_range, depth)
    db, dr = 2.0 * (1.0 - kb), 2.0 * (1.0 - kr)
    fwd = np.array([[sy * kr, sy * kg, sy * kb],
                    [sc * -kr / db, sc * -kg / db, sc * (1.0 - kb) / db],
                    [sc * (1.0 - kr) / dr, sc * -kg / dr, sc * -kb / dr]])
    crv, cbu = dr / sc, db / sc
    return fwd, (1.0 / sy, crv, cbu, -cbu * kb / kg, -crv * kr / kg)


def coeffs(matrix, full_range, depth=10):
    """(fwd int64 [3, 3], inv int64 [5]) as isr_yuv_coeffs_depth makes them."""
    f, v = real_coeffs(matrix, full_range, depth)
    sy = scales(full_range, depth)[0]
    fwd = np.zeros((3, 3), dtype=np.int64)
    for r in range(3):
        fwd[r, 0], fwd[r, 2] = fix(f[r, 0]), fix(f[r, 2])
        fwd[r, 1] = (fix(sy) if r == 0 else 0) - fwd[r, 0] - fwd[r, 2]
    return fwd, np.array([fix(c) for c in v], dtype=np.int64)


def frame_bytes(h, w):
    return 3 * h * w


# ------------------------------------------------------------------------------- frame layout
def pack(y, u, v, layout, shift=0, stray=None):
    """planes of samples [n, h, w], [n, h/2, w/2] x 2 -> uint8 [n, 3 h w]: words sample << shift, in the
    layout's order.  `stray`: a uint16 array of the frame's word count per frame whose bits outside the
    sample field are ORed in (what an input may carry and a kernel must ignore)."""
    n = y.shape[0]
    if layout == "i420":
        words = np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1)
    else:
        words = np.concatenate([y.reshape(n, -1), np.stack([u, v], axis=-1).reshape(n, -1)], axis=1)
    words = (words.astype(np.int64) << shift).astype("<u2")
    if stray is not None:
        field = np.uint16(top(10) << shift)
        words = words | (np.asarray(stray, dtype="<u2").reshape(words.shape) & ~field)
    return np.ascontiguousarray(words).view(np.uint8).reshape(n, -1)


def words_of(frames, h, w):
    """uint8 [n, 3 h w] (any shape of that many bytes) -> uint16 words [n, 3 h w / 2]"""
    Y.check_size(h, w)
    return np.ascontiguousarray(np.asarray(frames, dtype=np.uint8)).reshape(-1, frame_bytes(h, w)).view("<u2")


def unpack(frames, h, w, layout, shift=0, depth=10):
    """uint8 [n, 3 h w] -> sample planes (y, u, v) as int64: (word >> shift) & (2^depth - 1)"""
    f = (words_of(frames, h, w).astype(np.int64) >> shift) & top(depth)
    n = f.shape[0]
    y = f[:, :h * w].reshape(n, h, w)
    if layout == "i420":
        q = h * w // 4
        return y, f[:, h * w:h * w + q].reshape(n, h // 2, w // 2), f[:, h * w + q:].reshape(n, h // 2, w // 2)
    uv = f[:, h * w:].reshape(n, h // 2, w // 2, 2)
    return y, uv[..., 0], uv[..., 1]


# ------------------------------------------------------------------------------- the float kinds
def normalise(v, mean, inv_std, depth=10):
    """ISR_RGB_NORM_F32 of integer planes [n, 3, h, w]: fp32, one division, subtraction, multiplication."""
    q = np.asarray(v).astype(np.float32) / np.float32(top(depth))
    m = np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1)
    s = np.asarray(inv_std, dtype=np.float32).reshape(1, 3, 1, 1)
    out = (q - m) * s
    assert out.dtype == np.float32
    return out


def quantise(t, depth=10):
    """ISR_RGB_TANH_F32: fp32 t (any shape) -> int64 levels; NaN and t <= -1 give 0, t >= 1 the top."""
    t = np.asarray(t, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint((t + np.float32(1.0)) * np.float32(0.5) * np.float32(top(depth)))
        assert q.dtype == np.float32
        q = np.clip(np.nan_to_num(q, nan=0.0), 0, top(depth)).astype(np.int64)
        q = np.where(t > np.float32(-1.0), q, 0)
        return np.where(t >= np.float32(1.0), top(depth), q)


def rn32(x):
    """A positive Fraction rounded to the nearest fp32 (ties to even), as a Fraction; normal range only."""
    from fractions import Fraction
    e = 0
    while x / Fraction(2) ** e >= 1 << 24:
        e += 1
    while x / Fraction(2) ** e < 1 << 23:
        e -= 1
    return round(x / Fraction(2) ** e) * Fraction(2) ** e  # round(Fraction) is half-even


def quantise_exact(t, depth=10):
    """ISR_RGB_TANH_F32 of one fp32 value in rational arithmetic: each of the three operations exact, then
    rounded to fp32 once; rint half-even."""
    from fractions import Fraction
    t = np.float32(t)
    if not t > np.float32(-1.0):  # NaN too
        return 0
    if t >= np.float32(1.0):
        return top(depth)
    a = rn32(Fraction(float(t)) + 1)
    b = rn32(a * Fraction(1, 2))
    c = rn32(b * top(depth))
    return min(max(round(c), 0), top(depth))


def special_tanh_values(depth=10):
    """fp32 inputs of the quantiser's edges: every level's centre, the fp32 value nearest to every
    half-way point with both its neighbours, +-1 and their neighbours, +-0, beyond +-1, +-inf, NaN."""
    n = top(depth)
    centres = (2.0 * np.arange(n + 1) / n - 1.0).astype(np.float32)
    half = ((2.0 * np.arange(n) + 1.0) / n - 1.0).astype(np.float32)
    one = np.float32(1.0)
    edges = np.array([1.0, -1.0, 0.0, -0.0, 1.5, -1.5, 3e38, -3e38, np.inf, -np.inf, np.nan, 1e-30, -1e-30, -2.0 ** -24,
                      -2.0 ** -23, 2.0 ** -23],
                     dtype=np.float32)
    near = np.concatenate([np.nextafter(np.array([1, -1], np.float32), np.float32(0)),
                           np.nextafter(np.array([1, -1], np.float32), np.array([2, -2], np.float32))])
    return np.concatenate([centres, np.nextafter(half, -one - one), half, np.nextafter(half, one + one), edges, near])


# ------------------------------------------------------------------------------- integer
def rgb_to_yuv420(rgb, matrix="bt709", full_range=False, siting="left", layout="i420", shift=0, depth=10, peak=None):
    """integer RGB [n, 3, h, w] (the low `depth` bits of each value are read) -> uint8 [n, 3 h w].
    `peak`: a list that receives the largest absolute sum formed."""
    rgb = np.asarray(rgb).astype(np.int64) & top(depth)
    Y.check_size(*rgb.shape[-2:])
    fwd, _ = coeffs(matrix, full_range, depth)
    oy, mid = scales(full_range, depth)[2], 1 << (depth - 1)
    sums = [np.tensordot(fwd[0], rgb, ([0], [1])) + oy * ONE + ONE // 2]
    S, D = Y.chroma_sums(rgb, siting)
    sh = BITS + int(math.log2(D))
    sums += [np.tensordot(fwd[r], S, ([0], [1])) + mid * ONE * D + (ONE // 2) * D for r in (1, 2)]
    if peak is not None:
        peak.append(max(int(np.abs(s).max()) for s in sums))
    y, u, v = (np.clip(s >> k, 0, top(depth)) for s, k in zip(sums, (BITS, sh, sh)))
    return pack(y, u, v, layout, shift)


def yuv420_to_rgb(frames, h, w, matrix="bt709", full_range=False, siting="left", layout="i420", shift=0, depth=10,
                  peak=None):
    """uint8 [n, 3 h w] -> uint16 [n, 3, h, w] of 0 .. 2^depth - 1.  `peak`: a list that receives the
    largest absolute sum formed (the int32 question)."""
    y, u, v = unpack(frames, h, w, layout, shift, depth)
    _, (cy, crv, cbu, cgu, cgv) = coeffs(matrix, full_range, depth)
    oy, mid = scales(full_range, depth)[2], 1 << (depth - 1)
    U, D = Y.chroma_up(u, siting)
    V, _ = Y.chroma_up(v, siting)
    sh = BITS + int(math.log2(D))
    base = cy * D * (y - oy) + (ONE // 2) * D
    U, V = U - mid * D, V - mid * D
    sums = [base + crv * V, base + cgu * U + cgv * V, base + cbu * U]
    if peak is not None:
        peak.append(max(int(np.abs(s).max()) for s in sums))
    return np.clip(np.stack([s >> sh for s in sums], axis=1), 0, top(depth)).astype(np.uint16)


# ------------------------------------------------------------------------------- exact (fp64)
def rgb_to_yuv420_exact(rgb, matrix="bt709", full_range=False, siting="left", depth=10):
    """fp64 planes (y [n, h, w], u, v [n, h/2, w/2]) before rounding and clamping."""
    rgb = np.asarray(rgb).astype(np.float64)
    fwd, _ = real_coeffs(matrix, full_range, depth)
    oy, mid = scales(full_range, depth)[2], float(1 << (depth - 1))
    y = np.tensordot(fwd[0], rgb, ([0], [1])) + oy
    S, D = Y.chroma_sums(rgb, siting)
    return y, np.tensordot(fwd[1], S / D, ([0], [1])) + mid, np.tensordot(fwd[2], S / D, ([0], [1])) + mid


def yuv420_to_rgb_exact(frames, h, w, matrix="bt709", full_range=False, siting="left", layout="i420", shift=0, depth=10):
    """fp64 [n, 3, h, w] before rounding and clamping."""
    y, u, v = (p.astype(np.float64) for p in unpack(frames, h, w, layout, shift, depth))
    _, (cy, crv, cbu, cgu, cgv) = real_coeffs(matrix, full_range, depth)
    oy, mid = scales(full_range, depth)[2], float(1 << (depth - 1))
    U, D = Y.chroma_up(u, siting)
    V, _ = Y.chroma_up(v, siting)
    U, V = U / D - mid, V / D - mid
    base = cy * (y - oy)
    return np.stack([base + crv * V, base + cgu * U + cgv * V, base + cbu * U], axis=1)
