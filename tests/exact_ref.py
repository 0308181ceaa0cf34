"""Float64 CPU references for the exact-arithmetic tests of the MFMA conv, dgrad and wgrad kernels
(tests/test_gpu_exact.py), their integer input generators, and the table of cases both that file and
tests/test_exact_ref_cpu.py walk; at the end, the same for the 9x9 tail forward
(tests/test_gpu_tail_exact.py, tests/test_tail_exact_cpu.py).  No HIP, no GPU.

Why equality is a fair demand: activations, gradients and weights are small integers, the bias is
k/64 (k/1024 for the 9x9 head, whose sums are too small to round in fp16 otherwise) and every
epilogue scale is a power of two.  Every product and every partial sum of the kernel is then exactly
representable in fp32 whatever the MFMA order, the split-K partition or the FMA contraction, so the
only rounding in a kernel is its final store to bf16 / fp16 (none at all for the fp32 weight
gradients).  `assert_fp32_exact` is called on the accumulator and after every epilogue
stage: if it fails, the inputs are wrong, not the kernel.

The conv epilogue is restated in the documented order of include/isr.h / csrc/conv3x3.hip:
  1. v = conv + bias            2. v = v >= 0 ? v : v*slope
  3. v = v*s1 + r1 (r1 on channels < r1_cn when set)
  4. v = v*s2 + r2, or v *= s2 without r2
  5. v *= (m > 0 ? 1 : mslope) on channels >= m_c0     6. optional PixelShuffle(2)
  7. with shuffle, the mask is read on the shuffled grid (every channel).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

F64 = torch.float64


# ------------------------------------------------------------------ generators
def gen(seed) -> torch.Generator:
    """Seeded CPU generator; a string seeds by its CRC (stable across runs and machines)."""
    if isinstance(seed, str):
        seed = zlib.crc32(seed.encode())
    return torch.Generator(device="cpu").manual_seed(int(seed))


def _ints(shape, lo, hi, g) -> torch.Tensor:
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def acts(shape, g):
    """Activations, gradients and residuals: integers in [-3, 3]."""
    return _ints(shape, -3, 3, g)


def weights(shape, g):
    """Weights: integers in [-2, 2]."""
    return _ints(shape, -2, 2, g)


def even_weights(shape, g):
    """Weights in {-2, 0, 2}: the Winograd pack's (g0 +- g1 + g2) * 0.5 stays an integer."""
    return _ints(shape, -1, 1, g) * 2


def mask_src(shape, g):
    """Mask sources: integers in [-2, 2], about a fifth exactly 0."""
    return _ints(shape, -2, 2, g)


def bias(c, g, den=64):
    """k / 64, integer k in [-64, 64] (k / den, |k| <= den, for another power of two `den`)."""
    return _ints((c,), -den, den, g) / den


def u8_image(shape, g):
    """uint8 images holding only 0 and 255."""
    return (torch.randint(0, 2, tuple(shape), generator=g) * 255).to(torch.uint8)


# ------------------------------------------------------------------ exactness
def assert_fp32_exact(t: torch.Tensor, what: str = "value") -> None:
    assert torch.equal(t, t.float().double()), f"{what} is not exactly representable in fp32"


def granularity(*ts) -> float:
    """The largest power of two 2^-k (k >= 0) of which every element of every tensor is a multiple."""
    for k in range(40):
        if all(torch.equal(t * 2.0 ** k, (t * 2.0 ** k).round()) for t in ts if t is not None):
            return 2.0 ** -k
    raise AssertionError("inputs are not dyadic rationals")


def assert_sum_bound(x, W, b=None, padding=1, stride=1) -> None:
    """Worst case over every order of partial sums: (|W| conv |x|).max() + |bias|.max() must stay
    below 2^24 steps of the sums' granularity, so that no partial sum can round in fp32."""
    worst = F.conv2d(x.abs(), W.abs(), None, padding=padding, stride=stride).max().item()
    gran = granularity(x) * granularity(W)
    if b is not None:
        worst += b.abs().max().item()
        gran = min(gran, granularity(b))
    assert worst < 2.0 ** 24 * gran, (worst, gran)


def round_store(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> float32 (exact: asserted) -> dtype, round to nearest even; returned as float64."""
    assert_fp32_exact(v, "store operand")
    return v.float().to(dtype).double()


def rounding_is_exercised(v: torch.Tensor, dtype: torch.dtype) -> tuple[float, int]:
    """(share of elements of v not representable in dtype, number exactly halfway between two
    neighbours of dtype).  v is fp32-exact and inside dtype's normal range where non-zero."""
    assert_fp32_exact(v)
    mant = {torch.bfloat16: 7, torch.float16: 10}[dtype]
    a = v.abs()
    nz = a[a > 0]
    if nz.numel():
        lo, hi = (2.0 ** -14, 65504.0) if dtype == torch.float16 else (2.0 ** -126, 3.0e38)
        assert nz.min().item() >= lo and nz.max().item() <= hi
    inexact = (v.float().to(dtype).double() != v).double().mean().item()
    drop = 23 - mant  # fp32 mantissa bits the store drops
    bits = v.float().contiguous().view(torch.int32) & ((1 << drop) - 1)
    return inexact, int((bits == (1 << (drop - 1))).sum().item())


# ------------------------------------------------------------------ references
def lrelu(v, slope):
    return torch.where(v >= 0, v, v * slope)


def unshuffle_kernel_order(x2: torch.Tensor) -> torch.Tensor:
    """The x_sub2 view of a [n, cs, 2h, 2w] tensor: [n, 4cs, h, w] with channel s*cs + c
    (s = 2a + b) = x2[c] at (2y + a, 2x + b)."""
    return torch.cat([x2[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], dim=1)


def conv3x3_ref(x, W, b=None, *, slope=1.0, r1=None, s1=1.0, r1_cn=0, r2=None, s2=1.0, m=None, mslope=1.0,
                m_c0=0, shuffle=1, stride=1) -> torch.Tensor:
    """The unrounded float64 value the kernel stores (NCHW; on the 2h x 2w grid with shuffle=2)."""
    acc = F.conv2d(x, W, None, padding=1, stride=stride)
    assert_fp32_exact(acc, "accumulator")
    assert_sum_bound(x, W, b, stride=stride)
    v = acc if b is None else acc + b.view(1, -1, 1, 1)
    assert_fp32_exact(v, "conv + bias")
    v = lrelu(v, slope)
    assert_fp32_exact(v, "activation")
    if r1 is not None:
        v = v * s1
        assert_fp32_exact(v, "v * s1")
        cn = r1_cn if r1_cn else v.shape[1]
        v = torch.cat([v[:, :cn] + r1[:, :cn], v[:, cn:]], dim=1)
        assert_fp32_exact(v, "v * s1 + r1")
    v = v * s2
    assert_fp32_exact(v, "v * s2")
    if r2 is not None:
        v = v + r2
        assert_fp32_exact(v, "v * s2 + r2")
    if shuffle == 2:
        v = F.pixel_shuffle(v, 2)
        m_c0 = 0
    if m is not None:
        f = torch.where(m > 0, 1.0, mslope).to(F64)
        v = torch.cat([v[:, :m_c0], v[:, m_c0:] * f[:, m_c0:]], dim=1)
        assert_fp32_exact(v, "masked value")
    return v


def conv_input_grad(gy, W, padding=1, stride=1, in_hw=None) -> torch.Tensor:
    """d/dx of conv2d(x, W) for the upstream gradient gy, by float64 autograd."""
    n, _, ho, wo = gy.shape
    h, w = in_hw if in_hw is not None else (ho, wo)
    x = torch.zeros(n, W.shape[1], h, w, dtype=F64, requires_grad=True)
    F.conv2d(x, W, None, padding=padding, stride=stride).backward(gy)
    assert_fp32_exact(x.grad, "input gradient")
    return x.grad.detach()


def conv_weight_grad(x, g, k=3, scale=1.0, stride=1):
    """(dW, db) * scale of y = conv2d(x, W, b, padding=k//2) for the upstream gradient g, by float64
    autograd; exact (asserted), since the kernels' outputs are fp32 and take no rounding."""
    W = torch.zeros(g.shape[1], x.shape[1], k, k, dtype=F64, requires_grad=True)
    b = torch.zeros(g.shape[1], dtype=F64, requires_grad=True)
    F.conv2d(x, W, b, padding=k // 2, stride=stride).backward(g)
    dw, db = W.grad * scale, b.grad * scale
    assert_fp32_exact(dw, "dW")
    assert_fp32_exact(db, "db")
    # every partial sum of the reduction, in any order, is bounded by positions x the largest product
    worst = g.shape[0] * g.shape[2] * g.shape[3] * max(x.abs().max().item(), 1.0) * g.abs().max().item()
    assert worst < 2.0 ** 24 * granularity(x) * granularity(g) * granularity(torch.tensor(scale, dtype=F64))
    return dw.detach(), db.detach()


def head_input(x, mean=(0.0, 1.0, 0.0), std=(1.0, 0.5, 1.0)) -> torch.Tensor:
    """The head's input values: a uint8 image is normalised as (x/255 - mean) * inv_std."""
    if x.dtype != torch.uint8:
        return x.to(F64)
    mean_ = torch.tensor(mean, dtype=F64).view(1, 3, 1, 1)
    inv = (1.0 / torch.tensor(std, dtype=torch.float32)).double().view(1, 3, 1, 1)  # inv_std is an fp32 field
    v = (x.double() / 255.0 - mean_) * inv
    assert_fp32_exact(v, "normalised pixel")
    return v


def head9x9_ref(x, W, b=None, *, slope=1.0, m=None, mslope=1.0, mean=(0.0, 1.0, 0.0), std=(1.0, 0.5, 1.0)):
    xin = head_input(x, mean, std)
    assert torch.equal(xin, xin.to(torch.bfloat16).double()), "head input must survive the bf16 staging"
    acc = F.conv2d(xin, W, None, padding=4)
    assert_fp32_exact(acc, "accumulator")
    assert_sum_bound(xin, W, b, padding=4)
    v = acc if b is None else acc + b.view(1, -1, 1, 1)
    assert_fp32_exact(v, "conv + bias")
    v = lrelu(v, slope)
    assert_fp32_exact(v, "activation")
    if m is not None:
        v = torch.where(m > 0, v, v * mslope)
        assert_fp32_exact(v, "masked value")
    return v


# ------------------------------------------------------------------ the cases
G_IN, G_ONE, G_PAST = (1, 7, 5), (1, 16, 32), (2, 17, 33)  # inside a tile / one tile / past it, 2 images
BF, FP = torch.bfloat16, torch.float16
S1, S2, MSLOPE, SLOPE = 0.25, 0.5, 0.25, 0.25


@dataclass(frozen=True)
class Fwd:
    """One ops.conv3x3 launch: the shapes, the epilogue, and which storage types it runs in.
    `layout` names the buffer arrangement the GPU test builds (the values do not depend on it)."""
    name: str
    cin: int
    cout: int
    grid: tuple = G_PAST
    dtypes: tuple = (BF, FP)
    slope: float = 1.0
    r1: bool = False
    r1_is_x: bool = False   # r1 holds the values of x[:, :cout] (the residual fold's condition)
    r1_cn: int = 0
    s1: float = 1.0
    r2: bool = False
    s2: float = 1.0
    y2: bool = False
    mask: bool = False
    m_c0: int = 0
    mslope: float = 1.0
    shuffle: int = 1
    x_sub2: bool = False
    layout: str = "plain"


def _plain():
    out = []
    for cin, cout in [(16, 32), (96, 160), (192, 64), (96, 64)]:
        for grid in (G_IN, G_ONE, G_PAST):
            out.append(Fwd(f"plain-{cin}-{cout}-{grid[1]}x{grid[2]}", cin, cout, grid, slope=SLOPE))
    return out


PLAIN = _plain()
E = dict(s1=S1, s2=S2)
EPILOGUE = [
    Fwd("r1", 64, 64, r1=True, **E),
    Fwd("r2", 64, 64, r2=True, **E),
    Fwd("r1+r2-inplace", 192, 64, r1=True, r2=True, layout="y_is_r2", **E),
    Fwd("r1-32cout", 96, 32, r1=True, **E),
    Fwd("r1_cn64", 64, 192, r1=True, r1_cn=64, **E),
    Fwd("s2-only", 64, 64, slope=SLOPE, s2=S2),
    Fwd("y2", 64, 64, slope=SLOPE, y2=True),
    Fwd("y2+r1", 64, 64, y2=True, r1=True, **E),
    Fwd("y2+r2", 64, 64, y2=True, r2=True, **E),
    Fwd("y2+r1+r2", 64, 32, y2=True, r1=True, r2=True, **E),
    Fwd("mask-c0", 64, 192, dtypes=(BF,), mask=True, mslope=MSLOPE, s2=S2),
    Fwd("mask-c160", 64, 192, dtypes=(BF,), mask=True, m_c0=160, mslope=MSLOPE, s2=S2),
    Fwd("mask+r1", 64, 192, dtypes=(BF,), mask=True, m_c0=160, mslope=MSLOPE, r1=True, r1_cn=64, **E),
    Fwd("mask+r2", 64, 64, dtypes=(BF,), mask=True, mslope=MSLOPE, r2=True, **E),
    Fwd("mask+r1+r2", 64, 64, dtypes=(BF,), mask=True, mslope=MSLOPE, r1=True, r2=True, **E),
    Fwd("shuffle", 64, 256, slope=SLOPE, shuffle=2),
    Fwd("shuffle+mask", 64, 256, dtypes=(BF,), shuffle=2, mask=True, mslope=MSLOPE),
    Fwd("growth-slice", 96, 32, slope=SLOPE, layout="growth"),
    Fwd("dgrad-accumulate", 32, 160, dtypes=(BF,), r1=True, mask=True, m_c0=128, mslope=MSLOPE, layout="accumulate"),
]
# the residual fold (r1 is the conv's own input, slope 1, 1/s1 exact): the GPU test runs each case once
# with r1 = x's buffer (the fold triggers) and once with r1 in a buffer of its own (it does not)
FOLD = [
    Fwd("fold", 192, 64, r1=True, r1_is_x=True, s1=S1, layout="fold"),
    Fwd("fold+r2", 192, 64, r1=True, r1_is_x=True, s1=S1, r2=True, s2=S2, layout="fold"),
]
# x_sub2 needs cin % 128 == 0 (isr_conv3x3_fwd's descriptor check), so cin 192 (cs = 48) is refused and
# the compile-time-cin 192 tile never runs its x_sub2 form through the public entry
XSUB2 = [
    Fwd("xsub2-128-32", 128, 32, dtypes=(BF,), slope=SLOPE, x_sub2=True),
    Fwd("xsub2-256-64", 256, 64, dtypes=(BF,), slope=SLOPE, x_sub2=True),
    Fwd("xsub2-128-64-one-tile", 128, 64, G_ONE, dtypes=(BF,), slope=SLOPE, x_sub2=True),
]
FWD_CASES = PLAIN + EPILOGUE + FOLD + XSUB2


def fwd_inputs(c: Fwd) -> dict:
    """The case's inputs as float64 CPU tensors, from a generator seeded by its name."""
    g = gen(c.name)
    n, h, w = c.grid
    d = {}
    if c.x_sub2:  # the stored tensor: cin / 4 channels on the 2h x 2w grid
        d["x2"] = acts((n, c.cin // 4, 2 * h, 2 * w), g)
        d["x"] = unshuffle_kernel_order(d["x2"])
    else:
        d["x"] = acts((n, c.cin, h, w), g)
    d["W"] = weights((c.cout, c.cin, 3, 3), g)
    d["b"] = bias(c.cout, g)   # every case carries a bias, so its stores really round
    d["r1"] = (d["x"][:, :c.cout].clone() if c.r1_is_x else acts((n, c.cout, h, w), g)) if c.r1 else None
    d["r2"] = acts((n, c.cout, h, w), g) if c.r2 else None
    if c.mask:
        d["m"] = mask_src((n, c.cout // 4, 2 * h, 2 * w) if c.shuffle == 2 else (n, c.cout, h, w), g)
    else:
        d["m"] = None
    return d


def fwd_ref(c: Fwd, d: dict) -> torch.Tensor:
    return conv3x3_ref(d["x"], d["W"], d["b"], slope=c.slope, r1=d["r1"], s1=c.s1, r1_cn=c.r1_cn, r2=d["r2"],
                       s2=c.s2, m=d["m"], mslope=c.mslope, m_c0=c.m_c0, shuffle=c.shuffle)


# input gradient through the transposed pack: (cin, cout, sub2) of the layer, scale 0.5
DGRAD_PACK = [(64, 32, False), (32, 160, False), (192, 64, False), (64, 256, True)]
DGRAD_SCALE = 0.5
# stride-2 convs through the 2x2 phase decomposition: (cin, cout) of the layer; the output grid is 17 x 33
STRIDE2 = [(64, 64), (128, 256)]
HEAD_GRIDS = [G_IN, G_PAST]
WGRAD_SCALE = 0.5
WGRAD_SPLITS = [(64, 64, G_IN), (192, 64, G_PAST)]
WGRAD9_GRIDS = [G_PAST, (3, 7, 70)]
# the RDB's five weight gradients: (cin, cout, g_coff, scale) over D = [x | o0..o3], E = [g_out | g_3..g_0]
RDB_GROUP = [(192, 64, 0, 0.5), (160, 32, 64, 1.0), (128, 32, 96, 1.0), (96, 32, 128, 1.0), (64, 32, 160, 1.0)]


def dgrad_pack_inputs(cin, cout, sub2, grid=G_PAST):
    g = gen(f"dgrad-{cin}-{cout}-{sub2}")
    n, h, w = grid
    W = weights((cout, cin, 3, 3), g)
    if sub2:  # the gradient of the PixelShuffle output: cout / 4 channels at 2h x 2w
        ghr = acts((n, cout // 4, 2 * h, 2 * w), g)
        gy = F.pixel_unshuffle(ghr, 2)
    else:
        ghr, gy = None, acts((n, cout, h, w), g)
    ref = conv_input_grad(gy, W) * DGRAD_SCALE
    assert_fp32_exact(ref)
    return W, gy, ghr, ref


def stride2_inputs(cin, cout, grid=G_PAST):
    """x [n, cin, 2h, 2w], W, b, gy [n, cout, h, w], the forward and input-gradient references, the
    mask source on x's grid and the masked input gradient."""
    g = gen(f"stride2-{cin}-{cout}")
    n, h, w = grid
    x = acts((n, cin, 2 * h, 2 * w), g)
    W = weights((cout, cin, 3, 3), g)
    b = bias(cout, g)
    gy = acts((n, cout, h, w), g)
    y = conv3x3_ref(x, W, b, slope=SLOPE, stride=2)
    gx = conv_input_grad(gy, W, stride=2, in_hw=(2 * h, 2 * w))
    m = mask_src((n, cin, 2 * h, 2 * w), g)
    gxm = torch.where(m > 0, gx, gx * MSLOPE)
    assert_fp32_exact(gxm, "masked input gradient")
    return x, W, b, gy, y, gx, m, gxm


def wino_inputs():
    """The one Winograd case: 160 -> 32, n = 2, 33 x 65, weights in {-2, 0, 2}, bias, LeakyReLU 0.25."""
    g = gen("wino-gpu")
    x, W, b = acts((2, 160, 33, 65), g), even_weights((32, 160, 3, 3), g), bias(32, g)
    return x, W, b, conv3x3_ref(x, W, b, slope=SLOPE)


def head_inputs(grid, u8: bool):
    g = gen(f"head-{grid}-{u8}")
    n, h, w = grid
    x = u8_image((n, 3, h, w), g) if u8 else acts((n, 3, h, w), g)
    W = weights((64, 3, 9, 9), g)
    # k / 1024: a {0, 255} image normalises to {0, 1} / {-2, 0}, and on the 7 x 5 grid the sums stay so
    # small that with k / 64 only 1 % of the fp16 stores would round (bf16: 58 %)
    b = bias(64, g, den=1024)
    return x, W, b, head9x9_ref(x, W, b, slope=SLOPE)


def tail_dgrad_inputs(grid):
    """The 9x9 tail's input gradient through the head kernel: gp [n, 3, h, w], the tail's weights W2
    [3, 64, 9, 9], the mask source, and LeakyReLU'(mask) * dL/dU by float64 autograd."""
    g = gen(f"taildgrad-{grid}")
    n, h, w = grid
    W2 = weights((3, 64, 9, 9), g)
    gp = acts((n, 3, h, w), g)
    m = mask_src((n, 64, h, w), g)
    gu = conv_input_grad(gp, W2, padding=4)
    ref = torch.where(m > 0, gu, gu * MSLOPE)
    assert_fp32_exact(ref)
    return W2, gp, m, ref


# ------------------------------------------------------------------ the 9x9 tail forward (conv2 + tanh)
# Activations are integers in [-3, 3], weights k/256 with |k| <= 2, the bias k/256 with |k| <= 64: all
# exact in bf16 and fp16, every partial sum a multiple of 1/256 of magnitude <= 31168/256, so the
# pre-activation s is exact in fp32 in any summation order and lies on the grid of step 1/256.  tanhf is
# not correctly rounded, so the fp32 output is not pinned to a bit pattern but to a bracket: with
# hstep = 1/512 (half a grid step) the output must lie strictly inside
# (tanh64(s - hstep), tanh64(s + hstep)).  Any tanhf good to a few ulps passes (the narrower side is
# 43.85 fp32 ulps at |s| = 4, more below); an output computed from any other grid point fails, and a wrong
# tap, row, channel, ring slot or image moves s by whole grid steps.  Past |s| = 4 the bracket narrows
# below what a tanhf owes, so there only the sign and tanh64(4 - hstep) <= |out| <= 1 are demanded, and
# a case may have at most 0.1 % of such pixels.
TAIL_GRID = 256
TAIL_HSTEP = 1.0 / 512
TAIL_SMAX = 4.0
TAIL_FAR_SHARE = 1e-3
TAIL_SH = (8, 16, 32, 64, 128, 256, 512)


def tail_weights(g):
    """[3, 64, 9, 9] of k/256, integer k in [-2, 2]."""
    return weights((3, 64, 9, 9), g) / TAIL_GRID


def tail_bias(g):
    """[3] of k/256, integer |k| <= 64."""
    return _ints((3,), -64, 64, g) / TAIL_GRID


def tail_preact(xp, W, b=None) -> torch.Tensor:
    """s = conv9x9(x) + bias in float64.  xp [n, 64, h + 8, w + 8] carries its own zero halo of 4 (as the
    activation buffer does), so a column slice [x0 - 4, x0 + 36) of a wide image gives that strip alone."""
    # the generators' ranges, from which the sum bound follows for any data (|s| <= 31168/256 < 2^24/256:
    # assert_sum_bound on the all-extreme tensors, tests/test_tail_exact_cpu.py)
    for t, lim, gran in ((xp, 3, 1), (W, 2, TAIL_GRID), (b, 64, TAIL_GRID)):
        if t is not None:
            assert t.dtype == F64 and torch.equal(t * gran, (t * gran).round()) and (t * gran).abs().max().item() <= lim
    s = F.conv2d(xp, W, None)
    if b is not None:
        s = s + b.view(1, -1, 1, 1)
    assert_fp32_exact(s, "pre-activation")
    assert torch.equal(s * TAIL_GRID, (s * TAIL_GRID).round()), "pre-activation off the 1/256 grid"
    return s


def fp32_ulp(v: torch.Tensor) -> torch.Tensor:
    """The fp32 spacing at |v| (float64 in and out; the smallest normal's below it)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def tail_bracket_ulps(s: torch.Tensor) -> torch.Tensor:
    """Per element of s with |s| <= 4: the smaller distance from tanh64(s) to the bracket's ends, in
    fp32 ulps of tanh64(s)."""
    t = torch.tanh(s)
    room = torch.minimum(torch.tanh(s + TAIL_HSTEP) - t, t - torch.tanh(s - TAIL_HSTEP))
    return (room / fp32_ulp(t))[s.abs() <= TAIL_SMAX]


def check_tail_fp32(out: torch.Tensor, s: torch.Tensor, what: str = "tail") -> dict:
    """The fp32 bar of the tail: `out` (fp32, the kernel's) against the float64 pre-activation `s` of the
    same pixels.  Returns what it saw: pixels, share past |s| = 4, distinct s, exact zeros of s, and the
    largest |out - tanh64(s)| in fp32 ulps (informative: tanhf's own error)."""
    assert out.dtype == torch.float32 and out.shape == s.shape and s.dtype == F64, (out.dtype, out.shape, s.shape)
    o, s = out.double().flatten(), s.flatten()
    far = s.abs() > TAIL_SMAX
    share = far.double().mean().item()
    assert share <= TAIL_FAR_SHARE, f"{what}: {share:.4%} of the pixels have |s| > {TAIL_SMAX}"
    near = ~far
    lo, hi = torch.tanh(s - TAIL_HSTEP), torch.tanh(s + TAIL_HSTEP)
    bad = near & ~((o > lo) & (o < hi))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {s.numel()} outputs outside their bracket, first at flat "
                             f"index {i}: s = {s[i].item()!r}, got {o[i].item()!r}, bracket ({lo[i].item()!r}, "
                             f"{hi[i].item()!r})")
    floor = torch.tanh(torch.tensor(TAIL_SMAX - TAIL_HSTEP, dtype=F64)).item()
    ok_far = (torch.sign(o) == torch.sign(s)) & (o.abs() >= floor) & (o.abs() <= 1.0)
    assert bool(ok_far[far].all()), f"{what}: a saturated output has the wrong sign or magnitude"
    # the output is a function of s: equal s, equal bits
    key = (s * TAIL_GRID).round().to(torch.int64)
    bits = out.flatten().contiguous().view(torch.int32).to(torch.int64)
    order = torch.argsort(key, stable=True)
    k, v = key[order], bits[order]
    twin = k[1:] == k[:-1]
    assert bool((v[1:][twin] == v[:-1][twin]).all()), f"{what}: equal pre-activations gave different output bits"
    t = torch.tanh(s)
    return dict(pixels=s.numel(), far=share, distinct=int(torch.unique(key).numel()), zeros=int((key == 0).sum()),
                tanhf_ulps=((o - t).abs() / fp32_ulp(t))[near].max().item())


def tail_u8_expected(t: torch.Tensor) -> torch.Tensor:
    """The uint8 image of the kernel's own fp32 output t, in fp32 on the CPU with the kernel's operations:
    clamp(round_half_even(((t + 1) / 2) * 255), 0, 255)."""
    assert t.dtype == torch.float32 and t.device.type == "cpu"
    return torch.clamp(torch.round(((t + 1) / 2) * 255), 0, 255).to(torch.uint8)


def tail_segment_rule(n, h, w, u8, cus, ha=None, wa=None) -> int:
    """The tail dispatcher's rule, restated: 0 = the per-tile kernel (an image's output reaches 2 GiB),
    else the walk's segment height: 512 halved while it does not divide ha or leaves a CU without a block."""
    if 3 * h * w * (1 if u8 else 4) >= 2 ** 31:
        return 0
    ha = -(-h // 32) * 32 if ha is None else ha
    wa = -(-w // 32) * 32 if wa is None else wa
    sh = 512
    while sh > 8 and (ha % sh or n * (wa // 32) * (ha // sh) < cus):
        sh //= 2
    return sh


def tail_case(sh, m, cus, strips):
    """(n, h, w) on which a device of `cus` compute units walks segments of `sh` rows.  The computed height
    is ha = m * max(sh, 32), m in {1, 3} (computed regions are multiples of 32 rows): from 32 rows on no
    larger power of two divides ha, and the batch gives n * strips * (ha / sh) >= cus blocks; below 32 the
    block count alone decides, so the batch is the smallest that fills the CUs at sh (sh = 16), or a small
    one that cannot fill them at 16 (sh = 8).  h = ha - 5 (h % 16 = 11: a partial last tile and rows the
    walk computes but must not store), w = 32 * strips - 9 (a last strip of 23 columns)."""
    assert sh in TAIL_SH and m in (1, 3)
    ha = m * max(sh, 32)
    nseg = ha // sh
    need = -(-cus // nseg)                      # n * strips >= ceil(cus / nseg)
    n = 2 if sh == 8 else max(2, -(-need // strips))
    h, w = ha - 5, 32 * strips - 9
    for u8 in (False, True):
        assert tail_segment_rule(n, h, w, u8, cus) == sh, (sh, m, cus, strips, n)
    return n, h, w
