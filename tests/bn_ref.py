"""Float64 CPU restatement of the five train-mode BatchNorm stages of include/isr.h (isr_bn_stats,
isr_bn_finalize, isr_bn_apply, isr_bn_bwd_reduce, isr_bn_bwd_apply), the input builders of
tests/test_gpu_bn_exact.py and tests/test_bn_ref_cpu.py, the error bounds of the realistic-data
test, and numpy fp32 emulations of the kernels' arithmetic.  No HIP, no GPU.

Why equality is a fair demand on the exact cases.  The build contracts a*b + c to an FMA wherever it
likes, and the reduce kernels sum in an order of their own.  An equality is therefore asserted only
where every product and every partial sum is exactly representable in fp32 (then any order and any
contraction give the same bits), or where a single rounding is the last operation.  The builders make
it so: data are quarters a few units either side of zero, gamma / beta / the saved means quarters (gamma up
to 63/4: a product of fewer bits would fit bf16's eight and no store would round),
invstd in {1/4, 1/2, 1, 2}, slope in {1, 1/4}, s1 / s2 / gscale powers of two, momentum 1/4, running
statistics eighths, hand-set backward sums cnt * k/8.  tests/test_bn_ref_cpu.py checks the conditions
(`check_sum_conditions`, `check_apply_exact`, `check_bwd_apply_exact`) for every case the GPU file runs.  No stage inherits another's inexact output:
the tests write `save` and `acc` themselves.

The stages (all float64, nothing rounded unless said):
  stats       (sum z, sum z^2) per channel over the valid n x h x w
  finalize    mean = S/cnt, var = max(SS/cnt - mean^2, 0), save = (fl32(mean), fl32(1/sqrt(var + eps))),
              running_mean <- (1-m) rm + m fl32(mean), running_var <- (1-m) rv + m fl32(var cnt / max(cnt-1, 1)),
              both in fp32 (nn.BatchNorm2d: biased variance inside, unbiased in running_var).  The
              divisor 1 at cnt == 1 is the kernel's own convention; torch refuses that case.
  apply       a = gamma invstd, b = beta - mean a, y = ((lrelu_slope(a z + b)) s1 + r1) s2 + r2,
              rounded ONCE to bf16 by the caller
  bwd_reduce  (sum g, sum g (z - mean) invstd)
  bwd_apply   A = gscale gamma invstd, dz = A (g - acc0/cnt) - A invstd (acc1/cnt) (z - mean), rounded
              once to bf16; dgamma = acc1 gscale, dbeta = acc0 gscale

Bounds of the realistic-data test (random bf16 data, production eps): see the section "bounds"."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

import exact_ref as X

F64 = torch.float64
U = 2.0 ** -24          # fp32 unit roundoff
UD = 2.0 ** -53         # float64 unit roundoff
BN_ROWS, BN_COLS = 8, 128   # rows of a plane per reduce block, columns per pass of its 128 column threads
BN_MAX_C = 1024


def f32(v: float) -> float:
    """The value a C float field receives."""
    return ctypes.c_float(v).value


def fl32(t: torch.Tensor) -> torch.Tensor:
    """One rounding to fp32, kept in float64."""
    return t.float().double()


def _c(v: torch.Tensor) -> torch.Tensor:
    return v.view(1, -1, 1, 1)


# ------------------------------------------------------------------ the five stages
def stats(z):
    return z.sum((0, 2, 3)), (z * z).sum((0, 2, 3))


def finalize(s, ss, cnt, eps, momentum=None, rm=None, rv=None, fields32: bool = True) -> dict:
    """save as fp32 values, the unrounded float64 invstd, var, and (rm, rv given) the new running
    statistics as float64 values BEFORE their last fp32 rounding.  eps and momentum are C float fields
    and the running update takes fl32(mean), fl32(unbiased var); fields32=False keeps all of those in
    float64 (the comparison with torch's float64 batch_norm)."""
    rnd, fld = (fl32, f32) if fields32 else (lambda t: t, float)
    eps = fld(eps)
    mean = s / cnt
    var = (ss / cnt - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    out = dict(mean=fl32(mean), invstd=fl32(inv), mean64=mean, invstd64=inv, var=var)
    if rm is not None:
        m = fld(momentum)
        om = fld(1.0 - m)                                  # (1.f - momentum): one fp32 subtraction
        out["unbiased"] = rnd(var * cnt / max(cnt - 1, 1))
        out["rm"] = om * rm + m * rnd(mean)
        out["rv"] = om * rv + m * out["unbiased"]
    return out


def lrelu(t, slope):
    return torch.where(t >= 0, t, t * slope)


def apply(z, mean, invstd, gamma, beta, slope=1.0, s1=1.0, r1=None, s2=1.0, r2=None) -> dict:
    """Every value the kernel forms, unrounded: a, b, the product az, t = az + b, `pre` (the epilogue
    before its last addition) and y.  T is the sum of |terms| of each element's expanded formula."""
    a = gamma * invstd
    b = beta - mean * a
    az = _c(a) * z
    t = az + _c(b)
    v = lrelu(t, slope) * s1
    if r1 is not None:
        v = v + r1
    pre = v * s2
    y = pre if r2 is None else pre + r2
    T = abs(s1 * s2) * max(1.0, abs(slope)) * (az.abs() + _c(beta.abs() + (mean * a).abs()))
    if r1 is not None:
        T = T + abs(s2) * r1.abs()
    if r2 is not None:
        T = T + r2.abs()
    return dict(a=a, b=b, ma=mean * a, az=az, t=t, pre=pre, y=y, T=T)


def bwd_reduce(z, g, mean, invstd):
    return g.sum((0, 2, 3)), (g * (z - _c(mean)) * _c(invstd)).sum((0, 2, 3))


def bwd_apply(z, g, acc0, acc1, cnt, mean, invstd, gamma, gscale) -> dict:
    A = gscale * gamma * invstd
    mg, mgx = acc0 / cnt, acc1 / cnt
    K = A * invstd * mgx
    p1 = _c(A) * (g - _c(mg))
    p2 = _c(K) * (z - _c(mean))
    T = _c(A.abs()) * (g.abs() + _c(mg.abs())) + p2.abs()
    return dict(A=A, K=K, mg=mg, mgx=mgx, p1=p1, p2=p2, dz=p1 - p2, T=T, dgamma=acc1 * gscale, dbeta=acc0 * gscale)


def bf16r(v: torch.Tensor) -> torch.Tensor:
    """The one rounding of a store: float64 -> fp32 (exact, asserted) -> bf16, as float64."""
    return X.round_store(v, torch.bfloat16)


# ------------------------------------------------------------------ exact cases
@dataclass(frozen=True)
class Case:
    """(n, c, h, w) of one launch; c_total / coff: the channels are the slice at offset coff of
    c_total-channel buffers (0: buffers of their own)."""
    name: str
    n: int
    c: int
    h: int
    w: int
    c_total: int = 0
    coff: int = 0

    @property
    def cnt(self) -> int:
        return self.n * self.h * self.w


CASES = [
    Case("partial-block", 1, 32, 7, 45),        # one partial row block, odd width
    Case("two-pass", 2, 32, 9, 130),            # image stride, a one-row last row block, second column pass
    Case("one-block", 1, 16, 8, 128),           # exactly one block and one pass, a single plane
    Case("max-c", 1, BN_MAX_C, 2, 3),           # the per-channel tables and loops four times round 256 threads
    Case("slice", 1, 32, 9, 130, 96, 32),       # the channel slice at offset 32 of 96-channel buffers
]
SLOPES = (1.0, 0.25)
S1, S2, GSCALE, MOMENTUM = 0.25, 2.0, 0.5, 0.25
INVSTDS = (0.25, 0.5, 1.0, 2.0)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def exact_inputs(case: Case, amp: int = 4) -> dict:
    """The case's dyadic inputs as float64 CPU tensors, from a generator seeded by its name.  `amp`
    is the data's range in units (the tests use the default; a wider one breaks the sum condition)."""
    g = X.gen("bn-" + case.name)
    shape, c = (case.n, case.c, case.h, case.w), case.c
    d = {k: _ints(shape, -4 * amp, 4 * amp, g) / 4 for k in ("z", "g", "r1", "r2")}
    d["gamma"] = _ints((c,), -63, 63, g) / 4
    d["gamma"][0], d["gamma"][1], d["gamma"][2] = 0.0, -0.75, 1.25      # a zero, a negative, a positive
    d["beta"] = _ints((c,), -32, 32, g) / 4
    d["beta"][0] = 0.0                                                  # gamma = beta = 0: lrelu argument exactly 0
    d["mean"] = _ints((c,), -12, 12, g) / 4
    d["invstd"] = 2.0 ** _ints((c,), -2, 1, g)
    d["rm"] = _ints((c,), -16, 16, g) / 8
    d["rv"] = _ints((c,), 1, 32, g) / 8
    d["acc0"] = case.cnt * _ints((c,), -8, 8, g) / 8
    d["acc1"] = case.cnt * _ints((c,), -8, 8, g) / 8
    return d


def _units_below_2_24(x: torch.Tensor, what: str) -> None:
    """Per channel, sum |x| in units of x's smallest step stays below 2^24: then every partial sum,
    in any order and with any contraction, is an integer number of steps below 2^24, hence exact."""
    worst = (x.abs().sum((0, 2, 3)) / X.granularity(x)).max().item()
    assert worst < 2.0 ** 24, f"{what}: {worst:.0f} steps, fp32 partial sums could round"


def check_sum_conditions(d: dict) -> None:
    z, g = d["z"], d["g"]
    _units_below_2_24(z, "sum z")
    _units_below_2_24(z * z, "sum z^2")
    _units_below_2_24(g, "sum g")
    X.assert_fp32_exact(z - _c(d["mean"]), "z - mean")
    X.assert_fp32_exact(g * (z - _c(d["mean"])), "g (z - mean)")
    _units_below_2_24(g * (z - _c(d["mean"])) * _c(d["invstd"]), "sum g xhat")


def check_apply_exact(r: dict) -> None:
    """a z + b, its parts, and the epilogue before and after its last addition survive fp32."""
    for k in ("a", "ma", "b", "az", "t", "pre", "y"):
        X.assert_fp32_exact(r[k], "apply " + k)


def check_bwd_apply_exact(r: dict) -> None:
    for k in ("A", "K", "mg", "mgx", "p1", "p2", "dz", "dgamma", "dbeta"):
        X.assert_fp32_exact(r[k], "bwd_apply " + k)


# ------------------------------------------------------------------ the composed exact run
COMPOSED = Case("composed", 2, 32, 9, 136)     # cnt = 2448 = 16 * 153


def composed_inputs(case: Case = COMPOSED) -> dict:
    """Data with exactly representable statistics: per channel an integer mean mu and deviations
    +-1, +-3 in the ratio 5 : 3 with balanced signs, so var = (5 + 27) / 8 = 4 and, with eps = 0,
    invstd = 1/2 and xhat in {+-1/2, +-3/2}.  g holds integers in [-3, 3], nudged by +-1 at no more
    than a few hundred elements of a channel until sum g and sum g xhat are multiples of cnt / 16:
      sum g is first made even with one +1 at an xhat = +1/2 element (sum g xhat is an integer iff
      sum g is even, every xhat being an odd multiple of 1/2);
      d at an xhat = +1/2 and d at an xhat = -1/2 element moves sum g by 2d and sum g xhat not at all;
      +d at the first and -d at the second moves sum g xhat by d and sum g not at all."""
    cnt, c = case.cnt, case.c
    assert cnt % 16 == 0
    g_ = X.gen("bn-" + case.name)
    dev = torch.tensor([1.0, -1.0] * (5 * cnt // 16) + [3.0, -3.0] * (3 * cnt // 16), dtype=F64)
    assert dev.numel() == cnt
    mu = _ints((c,), -2, 2, g_)
    z = torch.stack([dev[torch.randperm(cnt, generator=g_)] + mu[k] for k in range(c)])       # [c, cnt]
    g = _ints((c, cnt), -3, 3, g_)
    step = cnt // 16
    for k in range(c):
        xh = (z[k] - mu[k]) / 2
        plus, minus = (xh == 0.5).nonzero().flatten().tolist(), (xh == -0.5).nonzero().flatten().tolist()
        if int(g[k].sum().item()) % 2:
            g[k, plus.pop()] += 1
        s0 = int(g[k].sum().item())
        m = round(s0 / (2 * step)) * (2 * step) - s0           # even, |m| <= step
        for _ in range(abs(m) // 2):
            g[k, plus.pop()] += math.copysign(1, m)
            g[k, minus.pop()] += math.copysign(1, m)
        s1 = (g[k] * xh).sum().item()
        assert s1 == round(s1)
        m = round(s1 / step) * step - int(s1)
        for _ in range(abs(m)):
            g[k, plus.pop()] += math.copysign(1, m)
            g[k, minus.pop()] -= math.copysign(1, m)

    def nchw(t):
        return t.view(c, case.n, case.h, case.w).transpose(0, 1).contiguous()

    d = dict(z=nchw(z), g=nchw(g), mu=mu)
    shape = (case.n, c, case.h, case.w)
    d["r1"], d["r2"] = _ints(shape, -12, 12, g_) / 4, _ints(shape, -12, 12, g_) / 4
    d["gamma"] = _ints((c,), -63, 63, g_) / 4
    d["gamma"][0], d["gamma"][1] = 0.0, -0.75
    d["beta"] = _ints((c,), -32, 32, g_) / 4
    d["beta"][0] = 0.0
    d["rm"], d["rv"] = _ints((c,), -16, 16, g_) / 8, _ints((c,), 1, 32, g_) / 8
    return d


# ------------------------------------------------------------------ realistic data
REAL = {"two-pass": Case("real-two-pass", 2, 32, 9, 130), "wide-batch": Case("real-wide-batch", 4, 64, 16, 32),
        "ill-conditioned": Case("real-ill-conditioned", 2, 32, 9, 130)}
REAL_EPS, REAL_MOMENTUM, REAL_S2, REAL_GSCALE = 1e-5, 0.1, 0.5, 0.25
REAL_SLOPE = REAL_S1 = f32(0.2)                # the value the descriptor's float field holds


def _bf(t):
    return t.to(torch.bfloat16).double()


def real_inputs(kind: str) -> dict:
    """Random normal data on the bf16 grid; `ill-conditioned`: channels of mean +-8 and std about 1/8
    (two steps of the bf16 grid at 8), where sum z^2 / cnt - mean^2 cancels 12 bits."""
    case = REAL[kind]
    g_ = X.gen("bn-" + case.name)
    shape, c = (case.n, case.c, case.h, case.w), case.c

    def rn(*s):
        return torch.randn(*s, generator=g_, dtype=F64)

    if kind == "ill-conditioned":
        sign = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0).to(F64)
        z = _bf(_c(8.0 * sign) + rn(*shape) / 8)
    else:
        z = _bf(rn(*shape) * 0.7 + _c(rn(c)))
    d = dict(z=z, g=_bf(rn(*shape)), r1=_bf(rn(*shape)), r2=_bf(rn(*shape)))
    d["gamma"] = fl32(torch.rand(c, generator=g_, dtype=F64) + 0.5) * torch.where(torch.arange(c) % 5 == 0, -1.0, 1.0)
    d["beta"] = fl32(rn(c) * 0.1)
    d["rm"] = fl32(rn(c) * 0.1)
    d["rv"] = fl32(torch.rand(c, generator=g_, dtype=F64) + 0.5)
    return d


# ------------------------------------------------------------------ bounds
# Every bound below is the standard forward error bound of a chain of k roundings, gamma_k times the
# sum of the magnitudes the roundings act on; k is counted from csrc/elementwise.hip for the
# UNcontracted code (contraction only removes roundings), nothing is tuned on a measured result.
#
# Reduce (bn_reduce_kernel): a thread adds at most BN_ROWS * ceil(w / 128) values in sequence (the
# first addition, to 0, is exact but is counted), five butterfly levels join the 32 lanes of a parity,
# three additions join the four waves: a value passes through at most D = 8 ceil(w/128) + 8 fp32
# additions, and each addition's error is at most u times the sum of the magnitudes under it.  The
# summand itself takes p roundings: 0 for z and g, 1 for z*z, 3 for g * (z - mean) * invstd.  So
# |block partial - exact| <= gamma_(D+p) sum |x|.  Blocks are joined in double by atomics: another
# nblocks * 2^-53 sum |x|.
#
# Apply (bn_apply_kernel), roundings on the path of each term of
# y = ((L(gamma invstd z + beta - mean gamma invstd)) s1 + r1) s2 + r2:
#   gamma invstd z:     a, z*a, + b, * slope, * s1, + r1, * s2, + r2            = 8
#   mean gamma invstd:  a, mean*a, beta - ., + b, * slope, * s1, + r1, * s2, + r2 = 9
#   beta: 7, r1: 3, r2: 1.   K_APPLY = 9.
# L is 1-Lipschitz for |slope| <= 1, so an argument whose sign the error flips costs no more than the
# error itself.
#
# Backward apply (bn_bwd_apply_kernel), v = ca (g - cc) - cb (z - cm) with ca = A = fl(fl(gscale gamma) istd),
# cb = fl(fl(A istd) mgx), cc = fl32(acc0/cnt), mgx = fl32(acc1/cnt), cm = the saved mean (an input):
#   A g:            A (2), g - cc, *, final -                = 5
#   A mg:           A (2), cc (1), g - cc, *, final -        = 6
#   K (z - mean):   A (2), * istd, mgx (1), * mgx, z - cm, *, final - = 8.   K_BWD = 8.
# dgamma / dbeta = fl(fl32(acc) * gscale): 2 roundings of the kernel's own double sum.
K_APPLY, K_BWD = 9, 8


def gamma_k(k: int) -> float:
    return k * U / (1.0 - k * U)


def reduce_depth(h: int, w: int) -> int:
    return min(h, BN_ROWS) * -(-w // BN_COLS) + 8


def reduce_blocks(case: Case) -> int:
    return case.n * -(-case.h // BN_ROWS)


def reduce_bound(x: torch.Tensor, case: Case, p: int) -> torch.Tensor:
    """Per channel: the most the kernel's double sum of the summands x (float64, [n, c, h, w]) may
    differ from their exact sum, p roundings going into each summand."""
    mag = x.abs().sum((0, 2, 3))
    return (gamma_k(reduce_depth(case.h, case.w) + p) + reduce_blocks(case) * UD) * mag


def save_brackets(s, ss, e0, e1, cnt, eps):
    """From |acc0 - s| <= e0, |acc1 - ss| <= e1: (mean_lo, mean_hi, invstd_lo, invstd_hi) that the
    kernel's fp32 save must lie in.  The double operations of the finalize add 4 * 2^-53 relative."""
    eps = f32(eps)
    mean, dm = s / cnt, e0 / cnt
    r = U + 4 * UD
    mlo, mhi = mean - dm - r * mean.abs(), mean + dm + r * mean.abs()
    var = (ss / cnt - mean * mean).clamp_min(0.0)
    dv = e1 / cnt + (2 * mean.abs() + dm) * dm + 4 * UD * (ss / cnt)
    ilo = 1.0 / torch.sqrt(var + dv + eps) * (1 - r)
    ihi = 1.0 / torch.sqrt((var - dv).clamp_min(0.0) + eps) * (1 + r)
    return mlo, mhi, ilo, ihi, dv


def bf16_bracket(ref: torch.Tensor, e: torch.Tensor):
    """The stored bf16 of any fp32 value within e of ref: fp32 and bf16 rounding are monotone, so it
    lies in [bf16(fl32(ref - e)), bf16(fl32(ref + e))].  That is half a bf16 ulp of ref plus e, made
    safe at a binade edge and where e exceeds the ulp."""
    lo = (ref - e).float().to(torch.bfloat16).double()
    hi = (ref + e).float().to(torch.bfloat16).double()
    return lo, hi


def assert_in_bracket(got: torch.Tensor, ref: torch.Tensor, e: torch.Tensor, what: str) -> float:
    """No element exempt.  Returns the largest |got - ref| in units of (half a bf16 ulp of ref + e)."""
    lo, hi = bf16_bracket(ref, e)
    bad = ~((got >= lo) & (got <= hi))
    if bool(bad.any()):
        k = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their bracket; first at {k}: "
                             f"got {got[k].item()!r}, ref {ref[k].item()!r}, bracket [{lo[k].item()!r}, {hi[k].item()!r}]")
    half_ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 8)
    return ((got - ref).abs() / (half_ulp + e)).max().item()


def assert_within(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    err = (got - ref).abs()
    assert bool((err <= bound).all()), (f"{what}: error {err.max().item():.3e} at channel {int((err - bound).argmax())} "
                                        f"exceeds its bound {bound[(err - bound).argmax()].item():.3e}")
    return (err / bound.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------ fp32 emulation (numpy)
# The kernels' arithmetic in numpy float32, in the kernels' order, without contraction and with the
# contraction hipcc may choose (an FMA is emulated as the float64 expression rounded once to fp32: the
# product of two fp32 values is exact in float64).  They show on the CPU that the bounds above are
# attainable by a correct fp32 implementation before the GPU sees them.
F = np.float32


def _np(t):
    return t.numpy().astype(np.float64)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def emu_reduce(z, g, mean, invstd, mode: int, contract: bool):
    """bn_reduce_kernel<mode> on [n, c, h, w] float64 tensors: per-thread sequential sums over the rows
    of a block and the column passes, the butterfly over 32 lanes, the four waves, blocks in double."""
    n, c, h, w = z.shape
    nrb, P = -(-h // BN_ROWS), -(-w // BN_COLS)
    pad = lambda t: np.pad(_np(t), ((0, 0), (0, 0), (0, nrb * BN_ROWS - h), (0, P * BN_COLS - w)))  # noqa: E731
    zz = pad(z).astype(F).reshape(n, c, nrb, BN_ROWS, P, BN_COLS)
    present = pad(torch.ones_like(z)).reshape(zz.shape) > 0
    if mode == 1:
        gg = pad(g).astype(F).reshape(zz.shape)
        mu = _np(mean).astype(F).reshape(1, c, 1, 1)
        istd = _np(invstd).astype(F).reshape(1, c, 1, 1)
    s1 = np.zeros((n, c, nrb, BN_COLS), F)
    s2 = np.zeros_like(s1)
    for y in range(BN_ROWS):
        for p in range(P):
            zv, ok = zz[:, :, :, y, p, :], present[:, :, :, y, p, :]
            if mode == 0:
                a1 = s1 + zv
                a2 = _fma(zv, zv, s2) if contract else s2 + zv * zv
            else:
                gv = gg[:, :, :, y, p, :]
                a1 = s1 + gv
                q = gv * (zv - mu)
                a2 = _fma(q, np.broadcast_to(istd, q.shape), s2) if contract else s2 + q * istd
            s1, s2 = np.where(ok, a1, s1).astype(F), np.where(ok, a2, s2).astype(F)
    out = []
    for s in (s1, s2):
        s = s.reshape(n, c, nrb, 4, 32)
        for _ in range(5):
            s = s[..., 0::2] + s[..., 1::2]
        s = s[..., 0]
        blk = ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]
        assert blk.dtype == F
        out.append(torch.from_numpy(blk.astype(np.float64).sum((0, 2))))
    return out


def emu_apply(z, mean, invstd, gamma, beta, slope, s1, r1, s2, r2, contract: bool) -> torch.Tensor:
    """bn_apply_kernel's value before the bf16 store (float64 holding fp32 values)."""
    c = z.shape[1]
    ch = lambda t: _np(t).astype(F).reshape(1, c, 1, 1)  # noqa: E731
    zv, a = _np(z).astype(F), ch(gamma) * ch(invstd)
    slope, s1, s2 = F(slope), F(s1), F(s2)
    if contract:
        b = _fma(-ch(mean), a, ch(beta))
        t = _fma(zv, np.broadcast_to(a, zv.shape), np.broadcast_to(b, zv.shape))
    else:
        b = ch(beta) - ch(mean) * a
        t = zv * a + b
    t = np.where(t >= 0, t, t * slope).astype(F)
    full = lambda x: np.broadcast_to(F(x), t.shape)  # noqa: E731
    if r1 is not None:
        v = _fma(t, full(s1), _np(r1).astype(F)) if contract else t * s1 + _np(r1).astype(F)
    else:
        v = t * s1
    if r2 is not None:
        v = _fma(v, full(s2), _np(r2).astype(F)) if contract else v * s2 + _np(r2).astype(F)
    else:
        v = v * s2
    assert v.dtype == F
    return torch.from_numpy(v.astype(np.float64))


def emu_bwd_apply(z, g, acc0, acc1, cnt, mean, invstd, gamma, gscale, contract: bool) -> torch.Tensor:
    c = z.shape[1]
    ch = lambda t: _np(t).astype(F).reshape(1, c, 1, 1)  # noqa: E731
    mg, mgx = (_np(acc0) / cnt).astype(F).reshape(1, c, 1, 1), (_np(acc1) / cnt).astype(F).reshape(1, c, 1, 1)
    istd = ch(invstd)
    A = F(gscale) * ch(gamma) * istd
    cb = A * istd * mgx
    d1, d2 = _np(g).astype(F) - mg, _np(z).astype(F) - ch(mean)
    p1 = A * d1
    v = _fma(-np.broadcast_to(cb, d2.shape), d2, p1) if contract else p1 - cb * d2
    assert v.dtype == F
    return torch.from_numpy(v.astype(np.float64))
