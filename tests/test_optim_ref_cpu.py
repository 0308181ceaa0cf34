"""Proof on the CPU that tests/optim_ref.py, the yardstick of the optimiser kernels' exact tests, is
right: fma32 against rational arithmetic, adam_step against torch.optim.Adam and against its own
float64 form, clip_coef against torch's clamp."""
import math
from fractions import Fraction

import numpy as np
import torch

import optim_ref as R

F32 = np.float32


# ------------------------------------------------------------------ fma32
def _round_f32(x: Fraction) -> float:
    """Round-to-nearest-even of a rational to fp32 (24 bits, exponent floor -149, overflow to inf)."""
    if x == 0:
        return 0.0
    s, x = (-1.0, -x) if x < 0 else (1.0, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    q = max(e - 23, -149)  # exponent of the last place
    scaled = x / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    if n * Fraction(2) ** q >= Fraction(2) ** 128:
        return s * math.inf
    return s * math.ldexp(float(n), q)  # n < 2^25 and the result is an fp32 value: exact


def _exact_fma(a, b, c) -> np.ndarray:
    out = [_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)]
    return np.array(out, dtype=np.float64).astype(F32)


def _naive_fma(a, b, c) -> np.ndarray:
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    return (a * b + c).astype(F32)


def _same_bits(x, y) -> bool:
    return np.array_equal(np.asarray(x, dtype=F32).view(np.int32), np.asarray(y, dtype=F32).view(np.int32))


def test_round_f32_is_numpys_rounding():
    """The rational rounding itself, on doubles, where numpy's float64 -> float32 cast is the yardstick."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal(2000) * 10.0 ** rng.uniform(-44, 38, 2000)
    x = np.concatenate([x, [2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149, 2.0 ** -126, 3.4028235677973366e38,
                            3.5e38, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1 + 3 * 2.0 ** -24]])
    with np.errstate(over="ignore"):
        want = x.astype(F32)
    got = np.array([_round_f32(Fraction(float(v))) for v in x], dtype=np.float64).astype(F32)
    assert _same_bits(got, want)


def test_fma32_random_triples_over_mixed_magnitudes():
    rng = np.random.default_rng(1)
    n = 4000
    a, b, c = ((rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F32) for _ in range(3))
    # a third of the addends near -a*b (cancellation), a third far below the product's last place
    k = n // 3
    c[:k] = (-(a[:k].astype(np.float64) * b[:k]) * (1 + rng.standard_normal(k) * 1e-6)).astype(F32)
    c[k:2 * k] *= F32(1e-9)
    assert _same_bits(R.fma32(a, b, c), _exact_fma(a, b, c))


def test_fma32_denormal_results():
    rng = np.random.default_rng(2)
    n = 3000
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-24, -18, n)).astype(F32)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-24, -18, n)).astype(F32)
    c = (rng.standard_normal(n) * 10.0 ** rng.uniform(-46, -38, n)).astype(F32)
    got, want = R.fma32(a, b, c), _exact_fma(a, b, c)
    small = np.abs(want.astype(np.float64)) < 2.0 ** -126
    assert small.sum() > n // 2 and (want != 0).sum() > n // 2
    assert _same_bits(got, want)


def test_fma32_ties_and_near_ties_where_float64_rounds_twice():
    """a b = 2^24 + 1 is an fp32 tie; an addend below float64's last place decides it.  The float64
    route loses the addend, lands on the tie and rounds to even: it must differ here, or this test
    would not show that the emulation matters."""
    t = 2.0 ** -40
    a = np.array([24929, 24929, 24929, 24929, 24929, 4097, 4097], dtype=F32)
    b = np.array([673, 673, 673, 673, -673, 4097, 4097], dtype=F32)       # 4097^2 = 2^24 + 2^13 + 1: a tie too
    c = np.array([t, -t, 0, 2.0 ** -100, -t, t, -t], dtype=F32)
    assert 24929 * 673 == 2 ** 24 + 1
    want = np.array([2 ** 24 + 2, 2 ** 24, 2 ** 24, 2 ** 24 + 2, -(2 ** 24 + 2), 4097 ** 2 + 1, 4097 ** 2 - 1],
                    dtype=F32)
    assert _same_bits(_exact_fma(a, b, c), want)
    assert _same_bits(R.fma32(a, b, c), want)
    naive = _naive_fma(a, b, c)
    assert naive[0] == 2 ** 24 and want[0] == 2 ** 24 + 2
    assert (naive != want).sum() >= 3
    # ties at random: odd a, b with an odd product in [2^24, 2^25) (last place 2), times a power of two,
    # and an addend of either sign 2^-45 .. 2^-80 of the product, or zero
    rng = np.random.default_rng(3)
    n = 3000
    a = rng.integers(2 ** 11, 2 ** 12, n) * 2 + 1
    b = (2 ** 24 + rng.integers(0, 2 ** 24, n)) // a | 1
    keep = (a * b >= 2 ** 24) & (a * b < 2 ** 25)
    assert keep.sum() > n // 2
    sh = 2.0 ** rng.integers(-60, 40, n)
    a, b = (a * sh).astype(F32)[keep], b.astype(F32)[keep]
    prod = a.astype(np.float64) * b.astype(np.float64)
    c = (prod * rng.choice([-1, 0, 1], n)[keep] * 2.0 ** -rng.integers(45, 80, n)[keep]).astype(F32)
    got, want = R.fma32(a, b, c), _exact_fma(a, b, c)
    assert _same_bits(got, want)
    assert (_naive_fma(a, b, c) != want).sum() > len(a) // 8


def test_fma32_specials():
    inf, nan = F32(np.inf), F32(np.nan)
    assert R.fma32(F32(2), F32(3), inf) == inf
    assert np.isnan(R.fma32(inf, F32(0), F32(1)))
    assert np.isnan(R.fma32(nan, F32(1), F32(1)))
    assert R.fma32(F32(3e38), F32(3e38), F32(0)) == inf
    z = R.fma32(F32(-0.0), F32(5), F32(-0.0))
    assert z == 0 and np.signbit(z)
    z = R.fma32(F32(1.5), F32(2), F32(-3))
    assert z == 0 and not np.signbit(z)


# ------------------------------------------------------------------ adam_step
SHAPES = [(64, 3, 9, 9), (64,), (32, 64, 3, 3), (7,), (1, 1), (70001,), (256, 64, 3, 3), (8, 16, 3, 3)]


def _randn(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def test_adam_step_matches_torch_adam_over_five_steps():
    """test_gpu_optim.py's shapes, hyper-parameters, schedule and bar (rtol 2e-6, atol 2e-7), on the CPU."""
    for wd in (0.0, 1e-2):
        ps = [p.requires_grad_() for p in _randn(SHAPES, 0)]
        opt = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.999), weight_decay=wd, foreach=False)
        sched = torch.optim.lr_scheduler.LinearLR(opt, 1, 0.01, total_iters=5)
        mine = [(p.detach().numpy().copy(), np.zeros(p.shape, F32), np.zeros(p.shape, F32)) for p in ps]
        for step in range(5):
            grads = _randn(SHAPES, 100 + step)
            args = R.adam_args(opt.param_groups[0]["lr"], 0.9, 0.999, 1e-8, wd, float(step + 1))
            mine = [R.adam_step(p, g.numpy(), m, v, args) for (p, m, v), g in zip(mine, grads)]
            for p, g in zip(ps, grads):
                p.grad = g
            opt.step(), sched.step()
        for (p, m, v), q in zip(mine, ps):
            assert p.dtype == F32
            torch.testing.assert_close(torch.from_numpy(p), q.detach(), rtol=2e-6, atol=2e-7)
            torch.testing.assert_close(torch.from_numpy(m), opt.state[q]["exp_avg"], rtol=2e-6, atol=2e-7)
            # exp_avg_sq is no part of that bar (the GPU test compares parameters), and it is further from
            # torch's: AdamOp forms 1 - beta2 in fp32 from the fp32 beta2, torch in double from the double,
            # and every increment of v carries the ratio of the two (1.3e-5 at beta2 = 0.999)
            c2 = abs(float(F32(1) - F32(0.999)) / (1 - 0.999) - 1)
            assert 1.2e-5 < c2 < 1.4e-5
            torch.testing.assert_close(torch.from_numpy(v), opt.state[q]["exp_avg_sq"], rtol=2e-6 + c2, atol=2e-7)


def _adam_data(n, seed, gmag=(-3, 3)):
    rng = np.random.default_rng(seed)
    mk = lambda lo, hi: (rng.standard_normal(n) * 10.0 ** rng.uniform(lo, hi, n)).astype(F32)  # noqa: E731
    p, g, m = mk(-3, 3), mk(*gmag), mk(*gmag)
    v = np.square(mk(*gmag))
    return p, g, m, v


def test_adam_step_within_the_derived_bound_of_float64():
    """|adam_step - adam_step64| <= the running error bound of adam_step64's docstring (13 roundings on
    the longest path, each U |x| + ETA, carried through the derivatives), for m, v and p, at the bias
    corrections of step 1 and step 1000, with and without weight decay and a scale, on normal-range
    data and on gradients of 1e-18 .. 1e-20 whose squares are denormal.  On normal-range data the bound
    itself stays below 16 U of the magnitudes that enter each result, so it is no loose bar."""
    for gmag in ((-3, 3), (-20, -18)):
        for wd in (0.0, 1e-2):
            for t in (1.0, 1000.0):
                for scale in (None, 0.3):
                    p, g, m, v = _adam_data(20000, 5, gmag)
                    args = R.adam_args(1e-3, 0.9, 0.999, 1e-8, wd, t)
                    got = R.adam_step(p, g, m, v, args, scale)
                    ref, bounds = R.adam_step64(p, g, m, v, args, scale, bound=True)
                    for name, x, y, b in zip("pmv", got, ref, bounds):
                        err = np.abs(x.astype(np.float64) - y)
                        worst = float((err / b).max())
                        print(f"adam_step vs float64 gmag={gmag} wd={wd} t={t} scale={scale} {name}: "
                              f"err/bound {worst:.3f}")
                        assert worst <= 1.0
                    if gmag == (-3, 3) and wd == 0.0:
                        g1 = np.abs(g.astype(np.float64)) * (1.0 if scale is None else 0.3)
                        assert (bounds[1] <= 16 * R.U * (g1 + np.abs(m)) + 1e-44).all()
                        assert (bounds[2] <= 16 * R.U * (g1 * g1 + v) + 1e-44).all()


# ------------------------------------------------------------------ clip_coef, ema
def test_clip_coef_reproduces_torchs_clamp():
    def torch_coef(norm, max_norm):
        return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(norm) + 1e-6), max=1.0).numpy()

    norm, coef = R.clip_coef([1.0, np.nan, 4.0], 10.0)
    assert np.isnan(norm) and np.isnan(coef) and np.isnan(torch_coef(norm, 10.0))
    norm, coef = R.clip_coef([1.0, np.inf, 4.0], 10.0)
    assert norm == np.inf and coef == 0 and torch_coef(norm, 10.0) == 0
    norm, coef = R.clip_coef([9.0, 16.0], 10.0)
    assert norm == 5 and coef == 1 and coef.dtype == F32
    norm, coef = R.clip_coef([0.0], 10.0)
    assert norm == 0 and coef == 1
    norm, coef = R.clip_coef([3.0e4, 7.0], 10.0)
    assert _same_bits(coef, torch_coef(norm, 10.0)) and coef < 1
    assert _same_bits(R.clip_coef(None, 10.0, norm=F32(173.25))[1], torch_coef(F32(173.25), 10.0))
    # double accumulation: 1e6 and a thousand 1e-2 that an fp32 running sum would drop
    parts = np.array([1e6] + [1e-2] * 1000, dtype=F32)
    assert R.clip_coef(parts, 1.0)[0] == F32(math.sqrt(math.fsum(float(x) for x in parts)))


def test_ema_rounds_the_exact_sum_once():
    v = np.array([2047 * 2.0 ** 7, -3.0, 1.0], dtype=F32)
    m = np.array([-2047 * 2.0 ** -8, 5.0, 2.0 ** -30], dtype=F32)
    for d in (0.5, 0.75, 0.9375):
        want = [_round_f32(Fraction(float(x)) * Fraction(d) + Fraction(float(y)) * Fraction(1 - d))
                for x, y in zip(v, m)]
        assert _same_bits(R.ema(v, m, d), np.array(want, dtype=F32))
