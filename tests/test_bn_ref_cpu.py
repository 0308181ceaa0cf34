"""tests/bn_ref.py on the CPU: the float64 restatement of the BatchNorm stages against
F.batch_norm(training=True) + autograd in float64, the input conditions that the equalities of
tests/test_gpu_bn_exact.py rest on (for every exact case that file runs), the composed-run builder's
targets, and the attainability of the realistic-data bounds by an fp32 evaluation in the kernels'
order, with and without FMA contraction."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as B
import exact_ref as X

F64 = torch.float64
BF16 = torch.bfloat16


# ------------------------------------------------------------------ the restatement is nn.BatchNorm2d
@pytest.mark.parametrize("shape", [(2, 32, 9, 130), (3, 16, 5, 7)])
def test_restatement_is_batch_norm_in_float64(shape):
    n, c, h, w = shape
    cnt = n * h * w
    g_ = X.gen(f"bn-anchor-{shape}")
    rn = lambda *s: torch.randn(*s, generator=g_, dtype=F64)  # noqa: E731
    z, g = rn(*shape) * 0.7 + rn(1, c, 1, 1), rn(*shape)
    gamma, beta, rm, rv = rn(c), rn(c), rn(c), torch.rand(c, generator=g_, dtype=F64) + 0.5
    eps, mom, gscale = 1e-5, 0.1, 0.25
    zr, w_, b_ = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    trm, trv = rm.clone(), rv.clone()
    pre = F.batch_norm(zr, trm, trv, w_, b_, training=True, momentum=mom, eps=eps)
    pre.backward(g * gscale)

    s, ss = B.stats(z)
    fin = B.finalize(s, ss, cnt, eps, mom, rm, rv, fields32=False)
    mean, inv = fin["mean64"], fin["invstd64"]      # the unrounded statistics: the comparison is in float64
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)  # noqa: E731
    close(B.apply(z, mean, inv, gamma, beta)["y"], pre.detach())
    a0, a1 = B.bwd_reduce(z, g, mean, inv)
    bw = B.bwd_apply(z, g, a0, a1, cnt, mean, inv, gamma, gscale)
    close(bw["dz"], zr.grad)
    close(bw["dgamma"], w_.grad)
    close(bw["dbeta"], b_.grad)
    close(fin["rm"], trm)
    close(fin["rv"], trv)
    unb = ((z - B._c(mean)) ** 2).sum((0, 2, 3)) / (cnt - 1)
    close(fin["unbiased"], unb)                                        # unbiased in running_var ...
    close(inv, 1 / torch.sqrt(unb * (cnt - 1) / cnt + eps))            # ... biased inside
    # the fp32 fields (eps, momentum, mean and unbiased var rounded to fp32) move nothing past fp32's grain
    f32_ = B.finalize(s, ss, cnt, eps, mom, rm, rv)
    torch.testing.assert_close(f32_["rm"], trm, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(f32_["rv"], trv, rtol=1e-6, atol=1e-7)
    # the epilogue order, against a hand-written one
    r1, r2 = rn(*shape), rn(*shape)
    y = B.apply(z, mean, inv, gamma, beta, 0.2, 0.5, r1, 4.0, r2)["y"]
    t = pre.detach()
    close(y, (torch.where(t >= 0, t, t * 0.2) * 0.5 + r1) * 4.0 + r2)


def test_finalize_conventions():
    """var clamps at 0; cnt == 1 divides by 1 (the kernel's convention, torch refuses the case)."""
    one = torch.ones(1, dtype=F64)
    f = B.finalize(3 * one, 8 * one, 1, 0.0, 0.25, 0 * one, 0 * one)      # mean 3, SS/cnt - mean^2 = -1
    assert f["var"].item() == 0.0 and f["rv"].item() == 0.0 and f["mean"].item() == 3.0
    f = B.finalize(one, 5 * one, 1, 0.0, 0.25, 0 * one, 0 * one)          # var 4, unbiased 4 * 1 / 1
    assert f["invstd"].item() == 0.5 and f["rv"].item() == 1.0 and f["rm"].item() == 0.25


# ------------------------------------------------------------------ input conditions of the exact cases
@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.name)
def test_exact_case_conditions(case):
    d = B.exact_inputs(case)
    B.check_sum_conditions(d)
    for k in ("z", "g", "r1", "r2"):
        assert torch.equal(d[k], d[k].to(BF16).double()), f"{k} does not survive bf16 storage"
    assert (d["gamma"] == 0).any() and (d["gamma"] < 0).any() and set(d["invstd"].tolist()) <= set(B.INVSTDS)
    # sums themselves, and the hand-set backward sums over cnt
    for v in (*B.stats(d["z"]), *B.bwd_reduce(d["z"], d["g"], d["mean"], d["invstd"])):
        X.assert_fp32_exact(v, "a sum")
    neg_all, zero_all = [], 0
    for slope in B.SLOPES:
        for r1 in (None, d["r1"]):
            for r2 in (None, d["r2"]):
                r = B.apply(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], slope, B.S1, r1, B.S2, r2)
                B.check_apply_exact(r)
                share, ties = X.rounding_is_exercised(r["y"], BF16)
                assert share >= 0.10 and ties > 0, (slope, r1 is not None, r2 is not None, share, ties)
                neg_all.append((r["t"] < 0).double().mean().item())
                zero_all += int((r["t"] == 0).sum())
    assert all(0.2 <= s <= 0.8 for s in neg_all) and zero_all > 0, (neg_all, zero_all)
    bw = B.bwd_apply(d["z"], d["g"], d["acc0"], d["acc1"], case.cnt, d["mean"], d["invstd"], d["gamma"], B.GSCALE)
    B.check_bwd_apply_exact(bw)
    share, ties = X.rounding_is_exercised(bw["dz"], BF16)
    assert share >= 0.10 and ties > 0, (share, ties)


def test_a_wider_builder_breaks_the_sum_condition():
    """The 2^24 condition bites: the same builder at 12 times the data range is refused."""
    case = next(c for c in B.CASES if c.name == "two-pass")
    with pytest.raises(AssertionError, match="partial sums could round"):
        B.check_sum_conditions(B.exact_inputs(case, amp=48))


def test_finalize_exact_values():
    """The hand-written finalize sums of the GPU file: everything up to the last rounding is exact."""
    c, cnt = 32, 2340
    d = B.exact_inputs(B.CASES[1])
    for eps, var in ((0.0, 4.0), (3.0, 1.0)):
        s, ss = cnt * d["mean"], cnt * (var + d["mean"] ** 2)
        f = B.finalize(s, ss, cnt, eps, B.MOMENTUM, d["rm"], d["rv"])
        assert torch.equal(f["mean"], d["mean"]) and torch.equal(f["var"], torch.full((c,), var, dtype=F64))
        assert torch.equal(f["invstd"], torch.full((c,), 0.5, dtype=F64))
        X.assert_fp32_exact(f["rm"], "running_mean")
        assert not torch.equal(f["rv"], B.fl32(f["rv"]))    # running_var's one rounding really happens


# ------------------------------------------------------------------ the composed exact run
def test_composed_builder_lands_on_its_targets():
    case, d = B.COMPOSED, B.composed_inputs()
    cnt, c = case.cnt, case.c
    s, ss = B.stats(d["z"])
    assert torch.equal(s, cnt * d["mu"]) and torch.equal(ss, cnt * (4 + d["mu"] ** 2))
    f = B.finalize(s, ss, cnt, 0.0, B.MOMENTUM, d["rm"], d["rv"])
    assert torch.equal(f["mean"], d["mu"]) and torch.equal(f["invstd"], torch.full((c,), 0.5, dtype=F64))
    dev = (d["z"] - B._c(d["mu"])).abs()
    assert set(dev.unique().tolist()) == {1.0, 3.0} and (dev == 1).sum().item() * 3 == (dev == 3).sum().item() * 5
    assert d["g"].abs().max().item() <= 4
    nudged = (d["g"].abs() == 4).sum((0, 2, 3)).max().item()
    a0, a1 = B.bwd_reduce(d["z"], d["g"], f["mean"], f["invstd"])
    step = cnt // 16
    assert torch.equal(a0 % step, torch.zeros(c, dtype=F64)) and torch.equal(a1 % step, torch.zeros(c, dtype=F64))
    assert nudged <= 400
    B.check_sum_conditions(dict(z=d["z"], g=d["g"], mean=f["mean"], invstd=f["invstd"]))
    r = B.apply(d["z"], f["mean"], f["invstd"], d["gamma"], d["beta"], B.SLOPES[1], B.S1, d["r1"], B.S2, d["r2"])
    B.check_apply_exact(r)
    share, ties = X.rounding_is_exercised(r["y"], BF16)
    assert share >= 0.10 and ties > 0, (share, ties)
    assert 0.2 <= (r["t"] < 0).double().mean().item() <= 0.8 and bool((r["t"] == 0).any())
    bw = B.bwd_apply(d["z"], d["g"], a0, a1, cnt, f["mean"], f["invstd"], d["gamma"], B.GSCALE)
    B.check_bwd_apply_exact(bw)
    share, _ = X.rounding_is_exercised(bw["dz"], BF16)
    assert share >= 0.10


# ------------------------------------------------------------------ the realistic bounds are attainable
@pytest.mark.parametrize("contract", [False, True], ids=["plain", "fma"])
@pytest.mark.parametrize("kind", list(B.REAL))
def test_fp32_evaluation_stays_inside_the_bounds(kind, contract):
    """The kernels' arithmetic in numpy fp32 passes the very checks the GPU test applies."""
    case, d = B.REAL[kind], B.real_inputs(kind)
    cnt, z, g = case.cnt, d["z"], d["g"]
    for k in ("z", "g", "r1", "r2"):
        assert torch.equal(d[k], d[k].to(BF16).double())
    if kind == "ill-conditioned":
        s, ss = B.stats(z)
        mean = s / cnt
        std = torch.sqrt(ss / cnt - mean * mean)
        assert bool(((mean.abs() - 8).abs() < 0.05).all()) and bool(((std - 0.125).abs() < 0.02).all())
    # forward
    s, ss = B.stats(z)
    acc = B.emu_reduce(z, None, None, None, 0, contract)
    e0, e1 = B.reduce_bound(z, case, 0), B.reduce_bound(z * z, case, 1)
    B.assert_within(acc[0], s, e0, "sum z")
    B.assert_within(acc[1], ss, e1, "sum z^2")
    fin = B.finalize(acc[0], acc[1], cnt, B.REAL_EPS)              # the finalize is double in the kernel too
    mlo, mhi, ilo, ihi, _ = B.save_brackets(s, ss, e0, e1, cnt, B.REAL_EPS)
    mean, inv = fin["mean"], fin["invstd"]
    assert bool(((mean >= mlo) & (mean <= mhi) & (inv >= ilo) & (inv <= ihi)).all())
    ref = B.apply(z, mean, inv, d["gamma"], d["beta"], B.REAL_SLOPE, B.REAL_S1, d["r1"], B.REAL_S2, d["r2"])
    y = B.emu_apply(z, mean, inv, d["gamma"], d["beta"], B.REAL_SLOPE, B.REAL_S1, d["r1"], B.REAL_S2, d["r2"], contract)
    B.assert_in_bracket(y.to(BF16).double(), ref["y"], B.gamma_k(B.K_APPLY) * ref["T"], "y")
    # backward
    r0, r1 = B.bwd_reduce(z, g, mean, inv)
    acc = B.emu_reduce(z, g, mean, inv, 1, contract)
    B.assert_within(acc[0], r0, B.reduce_bound(g, case, 0), "sum g")
    B.assert_within(acc[1], r1, B.reduce_bound(g * (z - B._c(mean)) * B._c(inv), case, 3), "sum g xhat")
    bw = B.bwd_apply(z, g, acc[0], acc[1], cnt, mean, inv, d["gamma"], B.REAL_GSCALE)
    dz = B.emu_bwd_apply(z, g, acc[0], acc[1], cnt, mean, inv, d["gamma"], B.REAL_GSCALE, contract)
    B.assert_in_bracket(dz.to(BF16).double(), bw["dz"], B.gamma_k(B.K_BWD) * bw["T"], "dz")


def test_brackets_refuse_a_wrong_value():
    ref = torch.tensor([1.0, 1 + 2.0 ** -9, -3.0], dtype=F64)
    e = torch.full((3,), 1e-6, dtype=F64)
    B.assert_in_bracket(ref.to(BF16).double(), ref, e, "ok")
    with pytest.raises(AssertionError, match="outside their bracket"):
        B.assert_in_bracket(ref.to(BF16).double() + torch.tensor([0.0, 2.0 ** -7, 0.0], dtype=F64), ref, e, "off by one")
    with pytest.raises(AssertionError, match="exceeds its bound"):
        B.assert_within(torch.tensor([1.1], dtype=F64), torch.tensor([1.0], dtype=F64), torch.tensor([0.05], dtype=F64), "s")
