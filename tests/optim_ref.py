"""Plain numpy restatements of the optimiser kernels (csrc/optim.hip), the yardstick of
test_gpu_optim_exact.py and test_gpu_optim.py; proved on the CPU by test_optim_ref_cpu.py.

AdamOp is written in explicit fmaf, sqrtf, / and single fp32 operations, all of them correctly rounded
on the device, so `adam_step` repeats them in numpy float32 (whose * - / sqrt are correctly rounded)
with `fma32` for every fmaf, and the kernel's result can be compared bit for bit.  No GPU, no project
code."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24        # fp32 unit roundoff
ETA = 2.0 ** -150     # half the smallest fp32 denormal: the absolute rounding error where a result is denormal

AdamArgs = namedtuple("AdamArgs", "step beta1 beta2 eps weight_decay bc2_sqrt")


def fma32(a, b, c) -> np.ndarray:
    """Correctly rounded fp32 fused multiply-add round(a * b + c) on arrays.

    The product of two fp32 values is exact in float64 (48 bits).  TwoSum gives the float64 sum s of
    product and addend with its exact error e; where e != 0 and s has an even last bit, s moves one
    unit towards e, so that its last bit is odd (round to odd: the sticky bit is kept in the last
    place).  A 53-bit round-to-odd value rounds to 24 bits (or fewer, for a denormal result) exactly
    as the infinitely precise sum does, because 53 >= 24 + 2."""
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F32)


def adam_args(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, t: float) -> AdamArgs:
    """The six fp32 fields of isr_adam_args the way FusedAdam.step makes them for step count t: computed in
    Python doubles, then cast."""
    bc1 = 1.0 - beta1 ** t
    return AdamArgs(F32(-lr / bc1), F32(beta1), F32(beta2), F32(eps), F32(weight_decay),
                    F32(math.sqrt(1.0 - beta2 ** t)))


def adam_step(p, g, m, v, args: AdamArgs, scale=None):
    """AdamOp's operations in AdamOp's order in fp32; the new (p, m, v).  `scale` (an fp32 value or None):
    the device gradient multiplier; None multiplies by 1.0, which changes no bit."""
    a = AdamArgs(*(F32(x) for x in args))
    p, g, m, v = (np.asarray(x, dtype=F32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        g = g * F32(1.0 if scale is None else scale)
        if a.weight_decay != 0:
            g = fma32(a.weight_decay, p, g)
        m = fma32(F32(1) - a.beta1, g - m, m)
        v = fma32(F32(1) - a.beta2, g * g, v * a.beta2)
        denom = np.sqrt(v) / a.bc2_sqrt + a.eps
        p = fma32(a.step, m / denom, p)
    return p, m, v


def adam_step64(p, g, m, v, args: AdamArgs, scale=None, bound: bool = False):
    """The same update in float64 on the same fp32 inputs and fp32 args.  With bound=True also the
    elementwise bounds (ep, em, ev) on |adam_step - adam_step64|, a running error analysis in which
    every fp32 operation with exact result x contributes r(x) = U |x| + ETA (half an ulp, or half the
    smallest denormal) and earlier errors are carried through each operation's derivative:

        g1 = g s                     e_g  = r(g1)                           (0 without a scale)
        g2 = wd p + g1               e_g += r(g2)                           (only with weight decay)
        c1 = 1 - beta1               e_c1 = U c1     (the kernel rounds it to fp32; this function does not)
        d  = g2 - m                  e_d  = e_g + r(d)
        m' = c1 d + m                e_m  = c1 e_d + e_c1 |d| + r(m')
        q  = g2^2                    e_q  = 2 |g2| e_g + e_g^2 + r(q)
        w  = v beta2                 e_w  = r(w)
        c2 = 1 - beta2               e_c2 = U c2
        v' = c2 q + w                e_v  = c2 e_q + e_c2 q + e_w + r(v')
        r  = sqrt(v')                e_r  = min(e_v / r, sqrt(e_v)) + r(r)  (both hold for any e_v)
        h  = r / bc2_sqrt            e_h  = e_r / bc2_sqrt + r(h)
        n  = h + eps                 e_n  = e_h + r(n)
        t  = m' / n                  e_t  = (e_m + |t| e_n) / (n - e_n) + r(t)
        p' = step t + p              e_p  = |step| e_t + r(p')

    That is 13 roundings on the longest path from g to p' (11 operations and the two rounded
    constants).  r() is taken at the exact value where the kernel rounds its own, slightly different,
    value; the difference is second order, and the three bounds are widened by 2^-10 for it."""
    a = AdamArgs(*(np.float64(F32(x)) for x in args))
    p, g, m, v = (np.asarray(x, dtype=F32).astype(np.float64) for x in (p, g, m, v))

    def r(x):
        return U * np.abs(x) + ETA

    with np.errstate(all="ignore"):
        zero = np.zeros_like(g)
        g2 = g * (1.0 if scale is None else np.float64(F32(scale)))
        e_g = zero if scale is None else r(g2)
        if a.weight_decay != 0:
            g2 = a.weight_decay * p + g2
            e_g = e_g + r(g2)
        c1, c2 = 1.0 - a.beta1, 1.0 - a.beta2
        d = g2 - m
        m1 = c1 * d + m
        q = g2 * g2
        w = v * a.beta2
        v1 = c2 * q + w
        root = np.sqrt(v1)
        h = root / a.bc2_sqrt
        n = h + a.eps
        t = m1 / n
        p1 = a.step * t + p
        if not bound:
            return p1, m1, v1
        e_d = e_g + r(d)
        e_m = c1 * e_d + U * c1 * np.abs(d) + r(m1)
        e_q = 2 * np.abs(g2) * e_g + e_g * e_g + r(q)
        e_v = c2 * e_q + U * c2 * q + r(w) + r(v1)
        e_r = np.minimum(np.where(root > 0, e_v / np.where(root > 0, root, 1.0), np.inf), np.sqrt(e_v)) + r(root)
        e_n = e_r / a.bc2_sqrt + r(h) + r(n)
        e_t = (e_m + np.abs(t) * e_n) / (n - e_n) + r(t)
        e_p = np.abs(a.step) * e_t + r(p1)
    k = 1.0 + 2.0 ** -10
    return (p1, m1, v1), (k * e_p, k * e_m, k * e_v)


def clip_coef(partials, max_norm: float, norm=None):
    """(norm, coef) of isr_clip_coef: norm = fp32(sqrt(float64 sum of the partials)) unless given, and
    coef = fp32(max_norm) / (norm + fp32(1e-6)) in fp32, clamped to at most 1 with NaN kept (torch.clamp(max=1))."""
    with np.errstate(all="ignore"):
        if norm is None:
            norm = F32(np.sqrt(np.sum(np.asarray(partials, dtype=F32).astype(np.float64))))
        norm = F32(norm)
        coef = F32(max_norm) / (norm + F32(1e-6))
    return norm, (F32(1.0) if coef > 1 else F32(coef))


def ema(v, m, d: float) -> np.ndarray:
    """v d + m e in float64, rounded once to fp32; d is the fp32 value the kernel receives and e = 1 - d
    the fp32 difference it forms (exact for the d of the exact-product cases)."""
    d = F32(d)
    e = F32(1) - d
    v, m = (np.asarray(x, dtype=F32).astype(np.float64) for x in (v, m))
    return (v * np.float64(d) + m * np.float64(e)).astype(F32)
