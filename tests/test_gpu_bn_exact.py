"""The train-mode BatchNorm kernels of csrc/elementwise.hip (bn_reduce_kernel<0/1>, bn_finalize_kernel,
bn_apply_kernel, bn_bwd_apply_kernel), stage by stage through isr_bn_stats / isr_bn_finalize /
isr_bn_apply / isr_bn_bwd_reduce / isr_bn_bwd_apply, against the float64 restatement of tests/bn_ref.py.

Every assertion is an equality (torch.equal on values), except:
  the invstd of a finalize at the production eps on arbitrary sums, which must be one of the two fp32
  neighbours of the float64 value (a double 1/sqrt accurate to a few double ulps, then one conversion);
  the realistic-data test at the end, whose bounds are derived in bn_ref.py ("bounds").

No stage inherits another's inexact output: the tests write BNState.save and BNState.acc themselves, with
dyadic values (bn_ref.py's builders; tests/test_bn_ref_cpu.py checks the conditions under which any
summation order and any FMA contraction give the same bits).  One composed run of ops.bn_forward and
ops.bn_backward on data with exactly representable statistics pins the hand-off between the stages.

Discipline of every case, as in test_gpu_glue.py: input buffers hold JUNK outside the values set (border,
ha x wa slack, neighbouring channels), output buffers SENTINEL; afterwards the valid interior of the
written slice equals the reference, its computed-but-invalid part is exactly zero, everything else still
holds the sentinel, and no input was written.

Not covered: the 64-bit index instantiation of the two apply kernels (2^31 or more element groups) needs
tens of GB per operand."""
import ctypes

import numpy as np
import pytest
import torch

import bn_ref as B
import exact_ref as X
import glue_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL, JUNK = 7.0, 3.0
F64 = torch.float64
ISR_ERR_BAD_DESC = -1
CASE_IDS = dict(ids=lambda c: c.name)


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


# ------------------------------------------------------------------ helpers
def _buf(case, x=None, fill=JUNK):
    """A buffer of the case's c_total channels filled with `fill`, x (float64 NCHW) at its slice."""
    from image_super_resolution_amd import ops
    b = ops.ActBuffer.alloc(case.n, case.h, case.w, case.c_total or case.c, 1, DEV)
    b.t.fill_(fill)
    if x is not None:
        b.set_nchw(x.float().to(DEV), case.coff)
    return b


def _bn(c, gamma=None, beta=None, rm=None, rv=None, eps=1e-5, momentum=B.MOMENTUM):
    bn = torch.nn.BatchNorm2d(c, eps=eps, momentum=momentum).to(DEV)
    with torch.no_grad():
        for dst, src in ((bn.weight, gamma), (bn.bias, beta), (bn.running_mean, rm), (bn.running_var, rv)):
            if src is not None:
                dst.copy_(src.float())
    return bn


def _state(c, save=None, acc=None):
    from image_super_resolution_amd import ops
    st = ops.BNState(c, DEV)
    st.save.fill_(SENTINEL)
    if save is not None:
        st.save.copy_(torch.cat(save).float())
    if acc is not None:
        st.acc.copy_(torch.cat(acc))
    return st


def _desc(case, zb, yb, st, bn, **kw):
    from image_super_resolution_amd import ops
    for k in ("r1", "r2", "dz"):
        if kw.get(k) is not None:
            kw[k + "_coff"] = case.coff
    return ops.bn_desc(zb, yb, case.c, st, bn, z_coff=case.coff, y_coff=case.coff, **kw)


def _run(stage: str, d, expect=0):
    from image_super_resolution_amd import _lib, ops
    rc = getattr(_lib.load(), "isr_bn_" + stage)(ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, f"isr_bn_{stage} returned {rc}: {_lib.load().isr_last_error().decode(errors='replace')}"


def _check_written(y, case, ref):
    """The three regions of an output buffer after a launch into the case's channel slice."""
    i, ii, iii = G.regions(y, case.coff, case.c)
    got = y.interior(case.coff, case.coff + case.c).double().cpu()
    assert got.shape == ref.shape
    if not torch.equal(got, ref):
        bad = got != ref
        k = bad.nonzero()[0].tolist()
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} interior elements differ; first at {k}: "
                             f"got {got[tuple(k)].item()!r}, want {ref[tuple(k)].item()!r}")
    assert bool((y.t[ii] == 0).all()), "computed-but-invalid positions are not exactly zero"
    assert bool((y.t[iii] == SENTINEL).all()), "a write outside the computed region of the channel slice"


def _snap(*bufs):
    return [(b, b.t.clone()) for b in bufs]


def _unchanged(pairs):
    for buf, before in pairs:
        assert torch.equal(buf.t, before), "an input buffer was written"


def _eq(got: torch.Tensor, want: torch.Tensor, what: str):
    got = got.detach().double().cpu()
    if not torch.equal(got, want):
        k = int((got != want).nonzero()[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {want.numel()} differ; first at {k}: "
                             f"got {got[k].item()!r}, want {want[k].item()!r}")


# ------------------------------------------------------------------ stats
@pytest.mark.parametrize("case", B.CASES, **CASE_IDS)
def test_stats_are_the_integer_sums_and_accumulate(case):
    """acc equals (sum z, sum z^2) of the valid region of the slice alone (the junk in the ha x wa slack,
    the border and the neighbouring channels is not seen); a second call without zeroing acc gives
    exactly twice the sums (isr.h: acc +=)."""
    d = B.exact_inputs(case)
    zb = _buf(case, d["z"])
    st, bn = _state(case.c), _bn(case.c)
    before = _snap(zb)
    desc = _desc(case, zb, zb, st, bn)
    want = torch.cat(B.stats(d["z"]))
    _run("stats", desc)
    _eq(st.acc, want, "acc")
    _run("stats", desc)
    _eq(st.acc, 2 * want, "acc after a second call")
    _unchanged(before)
    _eq(st.save, torch.full((2 * case.c,), SENTINEL, dtype=F64), "save")


# ------------------------------------------------------------------ finalize
FIN_CASES = [B.CASES[1], B.CASES[3]]      # cnt = 2340 at 32 channels; cnt = 6 at BN_MAX_C channels


def _finalize_setup(case, s, ss, eps, d, momentum=B.MOMENTUM, update_running=True):
    from image_super_resolution_amd import ops
    zb = ops.ActBuffer.alloc(case.n, case.h, case.w, case.c, 1, DEV)
    bn = _bn(case.c, rm=d["rm"], rv=d["rv"], eps=eps, momentum=momentum)
    st = _state(case.c, acc=(s, ss))
    return st, bn, ops.bn_desc(zb, zb, case.c, st, bn, update_running=update_running), zb


@pytest.mark.parametrize("eps,var", [(0.0, 4.0), (3.0, 1.0)], ids=["eps0-var4", "eps3-var1"])
@pytest.mark.parametrize("case", FIN_CASES, **CASE_IDS)
def test_finalize_where_var_plus_eps_is_a_power_of_four(case, eps, var):
    """save = (mean, 1/2) bit for bit from hand-written sums (eps = 3 with var = 1 proves that eps is
    added under the root); the running statistics with momentum 1/4 and dyadic old values; acc kept."""
    d, cnt = B.exact_inputs(case), case.cnt
    s, ss = cnt * d["mean"], cnt * (var + d["mean"] ** 2)
    ref = B.finalize(s, ss, cnt, eps, B.MOMENTUM, d["rm"], d["rv"])
    st, bn, desc, _ = _finalize_setup(case, s, ss, eps, d)
    _run("finalize", desc)
    _eq(st.save, torch.cat([d["mean"], torch.full((case.c,), 0.5, dtype=F64)]), "save")
    _eq(bn.running_mean, B.fl32(ref["rm"]), "running_mean")
    _eq(bn.running_var, B.fl32(ref["rv"]), "running_var")
    _eq(st.acc, torch.cat([s, ss]), "acc")


def _fp32_neighbours(v: torch.Tensor):
    """The largest fp32 <= v and the smallest fp32 >= v (float64 in and out)."""
    r = v.numpy().astype(np.float32)
    dn = np.where(r.astype(np.float64) <= v.numpy(), r, np.nextafter(r, np.float32(-np.inf)))
    up = np.where(r.astype(np.float64) >= v.numpy(), r, np.nextafter(r, np.float32(np.inf)))
    return torch.from_numpy(dn.astype(np.float64)), torch.from_numpy(up.astype(np.float64))


@pytest.mark.parametrize("case", FIN_CASES, **CASE_IDS)
def test_finalize_at_the_production_eps_on_arbitrary_sums(case):
    """save[0:c] = fl32(acc0 / cnt) bit for bit (one IEEE double division, one conversion); save[c:2c] one
    of the two fp32 neighbours of the float64 1/sqrt(var + eps); running_mean, whose one rounding is its
    last operation, bit for bit."""
    d, cnt = B.exact_inputs(case), case.cnt
    g_ = X.gen("bn-finalize-arbitrary-" + case.name)
    mean = torch.randn(case.c, generator=g_, dtype=F64) * 0.7
    s, ss = cnt * mean, cnt * (mean * mean + torch.rand(case.c, generator=g_, dtype=F64) + 0.05)
    ref = B.finalize(s, ss, cnt, 1e-5, B.MOMENTUM, d["rm"], d["rv"])
    st, bn, desc, _ = _finalize_setup(case, s, ss, 1e-5, d)
    _run("finalize", desc)
    save = st.save.double().cpu()
    _eq(save[:case.c], ref["mean"], "save mean")
    lo, hi = _fp32_neighbours(ref["invstd64"])
    got = save[case.c:]
    assert bool(((got == lo) | (got == hi)).all()), "invstd is not an fp32 neighbour of the float64 value"
    _eq(bn.running_mean, B.fl32(ref["rm"]), "running_mean")
    # running_var takes the double var, which a contracted acc1/cnt - mean*mean moves by a double ulp of
    # mean^2: fl32(unbiased var) may then be the other fp32 neighbour (2^-23 of it, a quarter of which
    # enters), and the sum rounds once more (2^-24 of the result): 2^-22 of the result bounds both
    rv = bn.running_var.double().cpu()
    assert bool(((rv - ref["rv"]).abs() <= 2.0 ** -22 * ref["rv"].abs()).all())


def test_finalize_clamps_a_negative_variance_and_divides_by_one_at_cnt_1():
    case = B.CASES[1]
    d, cnt, c = B.exact_inputs(case), case.cnt, case.c
    three = torch.full((c,), 3.0, dtype=F64)
    s, ss = cnt * three, cnt * (three * three - 1)                 # sum z^2 / cnt < mean^2, set by hand
    st, bn, desc, _ = _finalize_setup(case, s, ss, 1e-5, d)
    _run("finalize", desc)
    inv = np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5))))
    _eq(st.save, torch.cat([three, torch.full((c,), float(inv), dtype=F64)]), "save")
    _eq(bn.running_var, 0.75 * d["rv"], "running_var")             # unbiased var 0
    _eq(bn.running_mean, 0.75 * d["rm"] + 0.25 * three, "running_mean")
    # cnt = 1: var = 5 - 1 = 4, unbiased var = 4 * 1 / 1 (a divisor cnt - 1 would give inf)
    one = B.Case("cnt1", 1, 16, 1, 1)
    d = B.exact_inputs(one)
    s, ss = d["mean"], 4 + d["mean"] ** 2
    st, bn, desc, _ = _finalize_setup(one, s, ss, 0.0, d)
    _run("finalize", desc)
    _eq(st.save, torch.cat([d["mean"], torch.full((16,), 0.5, dtype=F64)]), "save at cnt 1")
    _eq(bn.running_var, 0.75 * d["rv"] + 1.0, "running_var at cnt 1")


def test_finalize_without_running_pointers_and_with_only_one():
    case = B.CASES[1]
    d, cnt, c = B.exact_inputs(case), case.cnt, case.c
    s, ss = cnt * d["mean"], cnt * (4 + d["mean"] ** 2)
    want = torch.cat([d["mean"], torch.full((c,), 0.5, dtype=F64)])
    st, bn, desc, _ = _finalize_setup(case, s, ss, 0.0, d, update_running=False)
    assert not desc.running_mean and not desc.running_var
    _run("finalize", desc)
    _eq(st.save, want, "save")
    _eq(bn.running_mean, d["rm"], "running_mean")
    _eq(bn.running_var, d["rv"], "running_var")
    for drop in ("running_mean", "running_var"):
        st, bn, desc, _ = _finalize_setup(case, s, ss, 0.0, d)
        setattr(desc, drop, None)
        _run("finalize", desc, expect=ISR_ERR_BAD_DESC)
        _eq(st.save, torch.full((2 * c,), SENTINEL, dtype=F64), "save after a refusal")
        _eq(bn.running_mean, d["rm"], "running_mean after a refusal")
        _eq(bn.running_var, d["rv"], "running_var after a refusal")


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("slope", B.SLOPES)
@pytest.mark.parametrize("r2", [False, True], ids=["", "r2"])
@pytest.mark.parametrize("r1", [False, True], ids=["", "r1"])
@pytest.mark.parametrize("case", B.CASES, **CASE_IDS)
def test_apply_from_a_dyadic_save(case, r1, r2, slope):
    """y = ((lrelu(a z + b)) s1 + r1) s2 + r2 rounded once to bf16, every product exact in fp32."""
    d = B.exact_inputs(case)
    zb = _buf(case, d["z"])
    r1b, r2b = (_buf(case, d["r1"]) if r1 else None), (_buf(case, d["r2"]) if r2 else None)
    yb = _buf(case, None, SENTINEL)
    st = _state(case.c, save=(d["mean"], d["invstd"]))
    bn = _bn(case.c, d["gamma"], d["beta"])
    before = _snap(*(b for b in (zb, r1b, r2b) if b is not None))
    _run("apply", _desc(case, zb, yb, st, bn, slope=slope, r1=r1b, s1=B.S1, r2=r2b, s2=B.S2))
    ref = B.apply(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], slope, B.S1, d["r1"] if r1 else None, B.S2,
                  d["r2"] if r2 else None)
    _check_written(yb, case, B.bf16r(ref["y"]))
    _unchanged(before)
    _eq(st.save, torch.cat([d["mean"], d["invstd"]]), "save")


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("case", B.CASES, **CASE_IDS)
def test_bwd_reduce_from_a_dyadic_save(case):
    d = B.exact_inputs(case)
    zb, gb = _buf(case, d["z"]), _buf(case, d["g"])
    st = _state(case.c, save=(d["mean"], d["invstd"]))
    before = _snap(zb, gb)
    _run("bwd_reduce", _desc(case, zb, gb, st, _bn(case.c, d["gamma"], d["beta"])))
    _eq(st.acc, torch.cat(B.bwd_reduce(d["z"], d["g"], d["mean"], d["invstd"])), "acc")
    _unchanged(before)


@pytest.mark.parametrize("in_place", [False, True], ids=["own-buffer", "in-place"])
@pytest.mark.parametrize("case", B.CASES, **CASE_IDS)
def test_bwd_apply_from_hand_written_sums(case, in_place):
    """dz rounded once, into a buffer of its own (g unchanged) or over g (dz.data == NULL); dgamma and
    dbeta = acc * gscale exactly."""
    d, c = B.exact_inputs(case), case.c
    zb = _buf(case, d["z"])
    gb = _buf(case, d["g"], SENTINEL if in_place else JUNK)
    dzb = None if in_place else _buf(case, None, SENTINEL)
    st = _state(c, save=(d["mean"], d["invstd"]), acc=(d["acc0"], d["acc1"]))
    bn = _bn(c, d["gamma"], d["beta"])
    dgam, dbet = torch.full((c,), SENTINEL, device=DEV), torch.full((c,), SENTINEL, device=DEV)
    before = _snap(zb) if in_place else _snap(zb, gb)
    _run("bwd_apply", _desc(case, zb, gb, st, bn, dz=dzb, dgamma=dgam, dbeta=dbet, gscale=B.GSCALE))
    ref = B.bwd_apply(d["z"], d["g"], d["acc0"], d["acc1"], case.cnt, d["mean"], d["invstd"], d["gamma"], B.GSCALE)
    _check_written(gb if in_place else dzb, case, B.bf16r(ref["dz"]))
    _unchanged(before)
    _eq(dgam, ref["dgamma"], "dgamma")
    _eq(dbet, ref["dbeta"], "dbeta")
    _eq(st.acc, torch.cat([d["acc0"], d["acc1"]]), "acc")


@pytest.mark.parametrize("given", ["dgamma", "dbeta"])
def test_bwd_apply_accepts_a_null_dgamma_or_dbeta(given):
    case = B.CASES[0]
    d, c = B.exact_inputs(case), case.c
    zb, gb, dzb = _buf(case, d["z"]), _buf(case, d["g"]), _buf(case, None, SENTINEL)
    st = _state(c, save=(d["mean"], d["invstd"]), acc=(d["acc0"], d["acc1"]))
    out = torch.full((3, c), SENTINEL, device=DEV)         # the given output between two guard rows
    desc = _desc(case, zb, gb, st, _bn(c, d["gamma"], d["beta"]), dz=dzb, gscale=B.GSCALE, **{given: out[1]})
    assert bool(desc.dgamma) != bool(desc.dbeta)
    _run("bwd_apply", desc)
    ref = B.bwd_apply(d["z"], d["g"], d["acc0"], d["acc1"], case.cnt, d["mean"], d["invstd"], d["gamma"], B.GSCALE)
    _check_written(dzb, case, B.bf16r(ref["dz"]))
    _eq(out[1], ref[given], given)
    assert bool((out[0] == SENTINEL).all()) and bool((out[2] == SENTINEL).all())


# ------------------------------------------------------------------ the composed exact run
def test_composed_forward_and_backward_on_exactly_representable_statistics():
    """ops.bn_forward then ops.bn_backward at (2, 32, 9, 136), eps = 0, on bn_ref.composed_inputs: var = 4
    exactly, so the kernels' own sums, save, running statistics, y, dz, dgamma and dbeta are all pinned."""
    from image_super_resolution_amd import ops
    case, d = B.COMPOSED, B.composed_inputs()
    cnt, c, slope = case.cnt, case.c, B.SLOPES[1]
    zb, r1b, r2b, gb = (_buf(case, d[k]) for k in ("z", "r1", "r2", "g"))
    yb, dzb = _buf(case, None, SENTINEL), _buf(case, None, SENTINEL)
    bn = _bn(c, d["gamma"], d["beta"], d["rm"], d["rv"], eps=0.0)
    st = _state(c)
    before = _snap(zb, r1b, r2b, gb)
    ops.bn_forward(_desc(case, zb, yb, st, bn, slope=slope, r1=r1b, s1=B.S1, r2=r2b, s2=B.S2), st)
    torch.cuda.synchronize()
    s, ss = B.stats(d["z"])
    fin = B.finalize(s, ss, cnt, 0.0, B.MOMENTUM, d["rm"], d["rv"])
    _eq(st.acc, torch.cat([s, ss]), "forward acc")
    _eq(st.save, torch.cat([fin["mean"], fin["invstd"]]), "save")
    _eq(bn.running_mean, B.fl32(fin["rm"]), "running_mean")
    _eq(bn.running_var, B.fl32(fin["rv"]), "running_var")
    ref = B.apply(d["z"], fin["mean"], fin["invstd"], d["gamma"], d["beta"], slope, B.S1, d["r1"], B.S2, d["r2"])
    _check_written(yb, case, B.bf16r(ref["y"]))
    dgam, dbet = torch.full((c,), SENTINEL, device=DEV), torch.full((c,), SENTINEL, device=DEV)
    ops.bn_backward(_desc(case, zb, gb, st, bn, dz=dzb, dgamma=dgam, dbeta=dbet, gscale=B.GSCALE), st)
    torch.cuda.synchronize()
    a0, a1 = B.bwd_reduce(d["z"], d["g"], fin["mean"], fin["invstd"])
    _eq(st.acc, torch.cat([a0, a1]), "backward acc")
    bw = B.bwd_apply(d["z"], d["g"], a0, a1, cnt, fin["mean"], fin["invstd"], d["gamma"], B.GSCALE)
    _check_written(dzb, case, B.bf16r(bw["dz"]))
    _eq(dgam, bw["dgamma"], "dgamma")
    _eq(dbet, bw["dbeta"], "dbeta")
    _unchanged(before)


# ------------------------------------------------------------------ realistic data, derived bounds
@pytest.mark.parametrize("kind", list(B.REAL))
def test_realistic_data_within_the_derived_bounds(kind):
    """Random normal bf16 data, eps 1e-5, momentum 0.1, through ops.bn_forward and ops.bn_backward; the
    reference of each stage is the float64 restatement on that stage's own inputs (the data, and the save /
    acc the kernels produced), its bound the one derived in bn_ref.py from the count of fp32 roundings:
    the sums against gamma_(D+p) sum |summand|, save and the running statistics against what those sum
    bounds allow, y and dz inside [bf16(ref - e), bf16(ref + e)] with e = gamma_k sum |terms|, dgamma and
    dbeta against the sum bound plus their two roundings.  No element is exempt.  `ill-conditioned`
    (|mean| = 8, std 1/8) is the case the explicit z - mean of bn_bwd_apply_kernel is there for."""
    from image_super_resolution_amd import ops
    case, d = B.REAL[kind], B.real_inputs(kind)
    cnt, c, z, g = case.cnt, case.c, d["z"], d["g"]
    zb, r1b, r2b, gb = (_buf(case, d[k]) for k in ("z", "r1", "r2", "g"))
    yb, dzb = _buf(case, None, SENTINEL), _buf(case, None, SENTINEL)
    bn = _bn(c, d["gamma"], d["beta"], d["rm"], d["rv"], eps=B.REAL_EPS, momentum=B.REAL_MOMENTUM)
    st = _state(c)
    ops.bn_forward(_desc(case, zb, yb, st, bn, slope=B.REAL_SLOPE, r1=r1b, s1=B.REAL_S1, r2=r2b, s2=B.REAL_S2), st)
    torch.cuda.synchronize()
    fig = {}
    acc, save = st.acc.cpu(), st.save.double().cpu()
    s, ss = B.stats(z)
    e0, e1 = B.reduce_bound(z, case, 0), B.reduce_bound(z * z, case, 1)
    fig["sum z"] = B.assert_within(acc[:c], s, e0, "sum z")
    fig["sum z^2"] = B.assert_within(acc[c:], ss, e1, "sum z^2")
    mlo, mhi, ilo, ihi, dv = B.save_brackets(s, ss, e0, e1, cnt, B.REAL_EPS)
    mean, inv = save[:c], save[c:]
    assert bool(((mean >= mlo) & (mean <= mhi)).all()), "saved mean outside its bracket"
    assert bool(((inv >= ilo) & (inv <= ihi)).all()), "saved invstd outside its bracket"
    fin = B.finalize(s, ss, cnt, B.REAL_EPS, B.REAL_MOMENTUM, d["rm"], d["rv"])
    fig["invstd rel"] = ((inv - fin["invstd64"]).abs() / fin["invstd64"]).max().item()
    m, om = B.f32(B.REAL_MOMENTUM), B.f32(1.0 - B.f32(B.REAL_MOMENTUM))
    r = B.U + 4 * B.UD
    ub = fin["var"] * cnt / (cnt - 1)
    brm = m * ((mhi - mlo) / 2) + B.gamma_k(2) * ((om * d["rm"]).abs() + (m * fin["mean64"]).abs())
    brv = m * (dv * cnt / (cnt - 1) + r * ub) + B.gamma_k(2) * ((om * d["rv"]).abs() + m * ub)
    fig["running_mean"] = B.assert_within(bn.running_mean.double().cpu(), om * d["rm"] + m * fin["mean64"], brm, "rm")
    fig["running_var"] = B.assert_within(bn.running_var.double().cpu(), om * d["rv"] + m * ub, brv, "rv")
    ref = B.apply(z, mean, inv, d["gamma"], d["beta"], B.REAL_SLOPE, B.REAL_S1, d["r1"], B.REAL_S2, d["r2"])
    _, ii, iii = G.regions(yb, 0, c)
    assert bool((yb.t[ii] == 0).all()) and bool((yb.t[iii] == SENTINEL).all())
    fig["y"] = B.assert_in_bracket(yb.interior().double().cpu(), ref["y"], B.gamma_k(B.K_APPLY) * ref["T"], "y")
    # backward, from the kernels' own save
    dgam, dbet = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    ops.bn_backward(_desc(case, zb, gb, st, bn, dz=dzb, dgamma=dgam, dbeta=dbet, gscale=B.REAL_GSCALE), st)
    torch.cuda.synchronize()
    acc = st.acc.cpu()
    r0, r1 = B.bwd_reduce(z, g, mean, inv)
    f0, f1 = B.reduce_bound(g, case, 0), B.reduce_bound(g * (z - B._c(mean)) * B._c(inv), case, 3)
    fig["sum g"] = B.assert_within(acc[:c], r0, f0, "sum g")
    fig["sum g xhat"] = B.assert_within(acc[c:], r1, f1, "sum g xhat")
    gs = B.f32(B.REAL_GSCALE)
    fig["dbeta"] = B.assert_within(dbet.double().cpu(), r0 * gs, gs * (f0 + B.gamma_k(2) * (r0.abs() + f0)), "dbeta")
    fig["dgamma"] = B.assert_within(dgam.double().cpu(), r1 * gs, gs * (f1 + B.gamma_k(2) * (r1.abs() + f1)), "dgamma")
    bw = B.bwd_apply(z, g, acc[:c], acc[c:], cnt, mean, inv, d["gamma"], gs)
    _, ii, iii = G.regions(dzb, 0, c)
    assert bool((dzb.t[ii] == 0).all()) and bool((dzb.t[iii] == SENTINEL).all())
    fig["dz"] = B.assert_in_bracket(dzb.interior().double().cpu(), bw["dz"], B.gamma_k(B.K_BWD) * bw["T"], "dz")
    print(f"\n{kind}: share of each bound used: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
