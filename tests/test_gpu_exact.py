"""The MFMA conv, dgrad and wgrad kernels against float64 CPU references (tests/exact_ref.py) on
integer data with power-of-two scales — every assertion is equality.

With activations / gradients in [-3, 3], weights in [-2, 2], a bias of k/64 and slopes and scales that
are powers of two, every product and partial sum is exact in fp32 in any order, so a kernel's output
must EQUAL the float64 result rounded once to its storage type (bf16 / fp16), and an fp32 weight
gradient must equal the integer result with no rounding at all.  A wrong tap, channel, border, tile
edge, image stride, epilogue order, mask rule (m == 0 occurs in a fifth of the mask sources) or
rounding mode shows as a mismatch; nothing hides under a tolerance.  The input conditions (fp32
exactness at every stage, >= 10 % of the stores really rounding, exact ties present) are checked on
the CPU in tests/test_exact_ref_cpu.py.  The sign of zero is not pinned (torch.equal compares values).

Grids: 7x5 (inside one 16 x 32 tile), 16x32 (one tile), 17x33 with n = 2 (one row and one column
past a tile, plus the image stride).  The 9x9 tail forward (tanh) has its own file,
test_gpu_tail_exact.py: exact pre-activations, a derived bracket for tanhf; so have the train-mode BatchNorm kernels,
test_gpu_bn_exact.py (each stage from hand-set dyadic statistics), and the optimiser kernels,
test_gpu_optim_exact.py.  Out of scope: the persistent trunk (its slopes are no powers of two; it is pinned bitwise to the
per-conv launches in test_gpu_chain.py)."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
from exact_ref import BF, FP
from test_gpu_kernels import WGRAD_FORMS  # every production form of the weight gradient

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def dev(t):
    return None if t is None else t.float().to(DEV)


def abuf(x, dt=BF, pad=1):
    from image_super_resolution_amd import ops
    return ops.ActBuffer.from_nchw(dev(x), pad=pad, dtype=dt)


def same(got, ref, what=""):
    """Equality on values, naming the first differing element."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} differ, first at {i}: "
                             f"got {got[i].item()!r}, want {ref[i].item()!r}")


def clean(b):
    assert int((b.outside_valid() != 0).sum()) == 0, "non-zero outside the valid region"


def junk(b, c0=0, c1=None):
    """Fill the computed ha x wa region of channels [c0, c1) with 7: the launch has to write every
    valid element and to zero the alignment slack itself, not inherit zeros from the allocation."""
    p = b.pad
    b.t[:, c0 // 16:None if c1 is None else c1 // 16, p:p + b.ha, p:p + b.wa, :] = 7.0
    return b


def ids(c):
    return c.name if isinstance(c, X.Fwd) else str(c).replace("torch.", "")


# ------------------------------------------------------------------ 3x3 forward and epilogue
def run_fwd(c: X.Fwd, dt, fold_separate=False):
    """Launch case c in storage type dt with the buffer arrangement c.layout names; returns
    (values read back from y, float64 reference rounded once to dt)."""
    from image_super_resolution_amd import ops
    d = X.fwd_inputs(c)
    ref = X.round_store(X.fwd_ref(c, d), dt)
    n, h, w = c.grid
    wp = ops.pack_conv3x3(dev(d["W"]), f16=dt == FP)
    b = dev(d["b"])
    kw = dict(slope=c.slope, s1=c.s1, s2=c.s2, r1_cn=c.r1_cn, shuffle=c.shuffle, x_sub2=c.x_sub2)
    if c.mask:
        kw.update(mslope=c.mslope, m_c0=c.m_c0)

    if c.layout == "growth":  # x = channels [0, cin) of a 192-channel buffer, y its slice [96, 128)
        full = X.acts((n, 192, h, w), X.gen(c.name + "-rest"))
        full[:, :c.cin] = d["x"]
        buf = abuf(full, dt)
        before = buf.t.clone()
        ops.conv3x3(buf, c.cin, wp, b, c.cout, buf, y_coff=96, **kw)
        torch.cuda.synchronize()
        assert torch.equal(buf.t[:, :6], before[:, :6]) and torch.equal(buf.t[:, 8:], before[:, 8:])
        clean(buf)
        return buf.to_nchw(96, 96 + c.cout), ref

    if c.layout == "accumulate":  # G[0:160] = mask * (conv(G[160:192]) + b + G[0:160]) in place
        gb = abuf(torch.cat([d["r1"], d["x"]], dim=1), dt)
        mb = abuf(d["m"], dt)
        ops.conv3x3(gb, c.cin, wp, b, c.cout, gb, x_coff=160, r1=gb, m=mb, **kw)
        torch.cuda.synchronize()
        same(gb.to_nchw(160, 192), d["x"], "the conv's own input slice")
        clean(gb)
        return gb.to_nchw(0, c.cout), ref

    if c.x_sub2:  # cin / 4 channels on the 2h x 2w grid, read as PixelShuffle(2) transposed
        yb = junk(ops.ActBuffer.alloc(n, h, w, c.cout, 1, DEV, dtype=dt))
        xb = ops.ActBuffer.alloc(n, 2 * h, 2 * w, c.cin // 4, 2, DEV, ha=2 * yb.ha, wa=2 * yb.wa, dtype=dt)
        xb.set_nchw(dev(d["x2"]), 0)
    else:
        xb = abuf(d["x"], dt)
        if c.shuffle == 2:
            yb = junk(ops.ActBuffer.alloc(n, 2 * h, 2 * w, c.cout // 4, 2, DEV, ha=2 * xb.ha, wa=2 * xb.wa, dtype=dt))
        else:
            yb = junk(ops.ActBuffer.alloc(n, h, w, c.cout, 1, DEV, dtype=dt))
    if c.r1:
        kw["r1"] = xb if (c.layout == "fold" and not fold_separate) else abuf(d["r1"], dt)
    if c.r2:
        kw["r2"] = abuf(d["r2"], dt)
        if c.layout == "y_is_r2":
            yb = kw["r2"]
    if c.mask:
        if c.shuffle == 2:
            kw["m"] = ops.ActBuffer.alloc(n, 2 * h, 2 * w, c.cout // 4, 1, DEV, ha=2 * xb.ha, wa=2 * xb.wa, dtype=dt)
            kw["m"].set_nchw(dev(d["m"]), 0)
        else:
            kw["m"] = abuf(d["m"], dt)
    y2 = None
    if c.y2:  # the second output: channels [32, 32 + cout) of a 192-channel buffer
        y2 = junk(ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=dt), 32, 32 + c.cout)
        kw.update(y2=y2, y2_coff=32)
    ops.conv3x3(xb, c.cin, wp, b, c.cout, yb, **kw)
    torch.cuda.synchronize()
    clean(yb)
    if y2 is not None:
        same(y2.to_nchw(32, 32 + c.cout), ref, c.name + " y2")
        assert int((y2.to_nchw(0, 32) != 0).sum()) == 0 and int((y2.to_nchw(32 + c.cout, 192) != 0).sum()) == 0
        clean(y2)
    return yb.to_nchw(0, c.cout if c.shuffle == 1 else c.cout // 4), ref


def _with_dtypes(cases):
    return [pytest.param(c, dt, id=f"{c.name}-{ids(dt)}") for c in cases for dt in c.dtypes]


@pytest.mark.parametrize("c,dt", _with_dtypes(X.PLAIN))
def test_conv3x3_plain(c, dt):
    """Bias + LeakyReLU 0.25 on every production tile: 16 -> 32 (one K-step, V_G0), 96 -> 160 (odd
    chunk count, five 32-cout tiles), 192 -> 64 (compile-time cin, V_F0), 96 -> 64 (V_W0)."""
    got, ref = run_fwd(c, dt)
    same(got, ref, c.name)


@pytest.mark.parametrize("c,dt", _with_dtypes(X.EPILOGUE))
def test_conv3x3_epilogue(c, dt):
    """Every epilogue MODE of conv3x3.hip (r1, r2, y2, mask, shuffle and their shipped
    combinations) with s1 = 0.25, s2 = 0.5, mslope = 0.25; the fp16 dispatch takes no mask."""
    got, ref = run_fwd(c, dt)
    same(got, ref, c.name)


@pytest.mark.parametrize("separate", [False, True], ids=["fold", "separate-r1"])
@pytest.mark.parametrize("c,dt", _with_dtypes(X.FOLD))
def test_conv3x3_residual_fold(c, dt, separate):
    """192 -> 64, slope 1, s1 = 0.25: with r1 the conv's own input buffer the residual rides the
    MFMAs (+ x / s1 on the centre tap); with the same values in a buffer of its own it is added in
    the epilogue.  Both equal the reference, hence each other."""
    got, ref = run_fwd(c, dt, fold_separate=separate)
    same(got, ref, c.name)


@pytest.mark.parametrize("c,dt", _with_dtypes(X.XSUB2))
def test_conv3x3_x_sub2(c, dt):
    """The PixelShuffle-transposed input read on the 32-cout and 64-cout tiles.  The descriptor check
    wants cin % 128 == 0, so cin 192 (cs = 48) is refused and V_F0's x_sub2 form is unreachable."""
    from image_super_resolution_amd import _lib, ops
    got, ref = run_fwd(c, dt)
    same(got, ref, c.name)
    y = ops.ActBuffer.alloc(1, 16, 32, 64, 1, DEV)
    x = ops.ActBuffer.alloc(1, 32, 64, 48, 2, DEV)
    with pytest.raises(_lib.IsrError, match="128"):
        ops.conv3x3(x, 192, torch.zeros(192 * 64 * 9, dtype=BF, device=DEV), None, 64, y, x_sub2=True)


@pytest.mark.parametrize("cin,cout", X.STRIDE2)
def test_stride2_phase_forms(cin, cout):
    """Stride-2 conv forward (x_sub2, taps=1, expand_fwd) and input gradient (shuffle=2, taps=2,
    expand_dgrad; also with the LeakyReLU' mask) against F.conv2d(stride=2) and its autograd."""
    from image_super_resolution_amd import ops
    from image_super_resolution_amd.train_layers import expand_dgrad, expand_fwd
    x, W, b, gy, y, gx, m, gxm = X.stride2_inputs(cin, cout)
    n, _, h, w = x.shape
    xb = ops.ActBuffer.alloc(n, h, w, cin, 2, DEV, min_hp=2 * ops.round_up(h // 2, 32) + 4,
                             min_wp=2 * ops.round_up(w // 2, 32) + 4)
    xb.set_nchw(dev(x), 0)
    yb = junk(ops.ActBuffer.alloc(n, h // 2, w // 2, cout, 1, DEV))
    ops.conv3x3(xb, 4 * cin, ops.pack_conv3x3(expand_fwd(dev(W))), dev(b), cout, yb, slope=X.SLOPE, x_sub2=True,
                taps=1)
    torch.cuda.synchronize()
    same(yb.to_nchw(), X.round_store(y, BF), "stride-2 forward")
    clean(yb)
    gyb = abuf(gy)
    wd = ops.pack_conv3x3(expand_dgrad(dev(W)))
    gxb = ops.ActBuffer.alloc(n, h, w, cin, 1, DEV, min_hp=2 * gyb.ha + 2, min_wp=2 * gyb.wa + 2)
    ops.conv3x3(gyb, cout, wd, None, 4 * cin, gxb, shuffle=2, taps=2)
    torch.cuda.synchronize()
    same(gxb.to_nchw(), X.round_store(gx, BF), "stride-2 input gradient")
    clean(gxb)
    mb = ops.ActBuffer.alloc(n, h, w, cin, 0, DEV, min_hp=2 * gyb.ha, min_wp=2 * gyb.wa)
    mb.set_nchw(dev(m), 0)
    gmb = ops.ActBuffer.alloc(n, h, w, cin, 1, DEV, min_hp=2 * gyb.ha + 2, min_wp=2 * gyb.wa + 2)
    ops.conv3x3(gyb, cout, wd, None, 4 * cin, gmb, shuffle=2, taps=2, m=mb, mslope=X.MSLOPE)
    torch.cuda.synchronize()
    same(gmb.to_nchw(), X.round_store(gxm, BF), "masked stride-2 input gradient")
    clean(gmb)


@pytest.mark.parametrize("cin,cout,sub2", X.DGRAD_PACK)
def test_dgrad_via_transposed_pack(cin, cout, sub2):
    """Input gradient = conv3x3 over the gradient with pack_conv3x3_dgrad's weights (rotated,
    transposed, times 0.5; the Scaler's PixelShuffle channel order with sub2) vs float64 autograd."""
    from image_super_resolution_amd import ops
    W, gy, ghr, ref = X.dgrad_pack_inputs(cin, cout, sub2)
    n, _, h, w = gy.shape
    wp = ops.pack_conv3x3_dgrad(dev(W), scale=X.DGRAD_SCALE, sub2=sub2)
    out = junk(ops.ActBuffer.alloc(n, h, w, cin, 1, DEV))
    if sub2:
        gb = ops.ActBuffer.alloc(n, 2 * h, 2 * w, cout // 4, 2, DEV, ha=2 * out.ha, wa=2 * out.wa)
        gb.set_nchw(dev(ghr), 0)
    else:
        gb = abuf(gy)
    ops.conv3x3(gb, cout, wp, None, cin, out, x_sub2=sub2)
    torch.cuda.synchronize()
    same(out.to_nchw(), X.round_store(ref, BF), f"dgrad {cin}<-{cout}")
    clean(out)


# ------------------------------------------------------------------ 9x9 head
@pytest.mark.parametrize("dt", [BF, FP], ids=ids)
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("grid", X.HEAD_GRIDS, ids=ids)
def test_head9x9(grid, u8, dt):
    """fp32 integer input, and uint8 input in {0, 255} with mean (0, 1, 0) / std (1, 0.5, 1) (the
    normalised values are 0, 1 and -2); bias, LeakyReLU 0.25, and the second output."""
    from image_super_resolution_amd import ops
    x, W, b, v = X.head_inputs(grid, u8)
    n, h, w = grid
    y = junk(ops.ActBuffer.alloc(n, h, w, 64, 1, DEV, dtype=dt))
    y2 = junk(ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=dt), 64, 128)
    xd = x.to(DEV) if u8 else dev(x)
    ops.head9x9(xd, ops.pack_head9x9(dev(W), f16=dt == FP), dev(b), y, slope=X.SLOPE, y2=y2, y2_coff=64,
                mean=(0.0, 1.0, 0.0), std=(1.0, 0.5, 1.0))
    torch.cuda.synchronize()
    ref = X.round_store(v, dt)
    same(y.to_nchw(), ref, "head y")
    same(y2.to_nchw(64, 128), ref, "head y2")
    assert int((y2.to_nchw(0, 64) != 0).sum()) == 0 and int((y2.to_nchw(128, 192) != 0).sum()) == 0
    clean(y)
    clean(y2)


@pytest.mark.parametrize("grid", X.HEAD_GRIDS, ids=ids)
def test_tail_dgrad_via_head_kernel_with_mask(grid):
    """The 9x9 tail's input gradient = the head kernel with flipped, transposed weights, times
    LeakyReLU'(mask source) with mslope 0.25 and m == 0 on the mslope side."""
    from image_super_resolution_amd import ops
    W2, gp, m, ref = X.tail_dgrad_inputs(grid)
    n, h, w = grid
    Wt = W2.flip(2, 3).transpose(0, 1).contiguous()
    out = junk(ops.ActBuffer.alloc(n, h, w, 64, 2, DEV))
    ops.head9x9(dev(gp), ops.pack_head9x9(dev(Wt)), None, out, slope=1.0, m=abuf(m), mslope=X.MSLOPE)
    torch.cuda.synchronize()
    same(out.to_nchw(), X.round_store(ref, BF), "tail dgrad")
    clean(out)


# ------------------------------------------------------------------ weight gradients (fp32, no rounding)
def _wgrad_form_inputs(cin, cout, kind, grid):
    """(x buffer, g buffer, keywords, float64 dW, float64 db, tap slice)."""
    from image_super_resolution_amd import ops
    g_ = X.gen(f"wgrad-{cin}-{cout}-{kind}-{grid}")
    n, h, w = grid
    if kind == "plain":
        x, gy = X.acts((n, cin, h, w), g_), X.acts((n, cout, h, w), g_)
        dw, db = X.conv_weight_grad(x, gy, scale=X.WGRAD_SCALE)
        return abuf(x), abuf(gy), {}, dw, db, slice(0, 3)
    if kind == "g_sub2":  # the gradient of the PixelShuffle output: cout / 4 channels at 2x
        x, ghr = X.acts((n, cin, h, w), g_), X.acts((n, cout // 4, 2 * h, 2 * w), g_)
        xb = abuf(x)
        gb = ops.ActBuffer.alloc(n, 2 * h, 2 * w, cout // 4, 2, DEV, ha=2 * xb.ha, wa=2 * xb.wa)
        gb.set_nchw(dev(ghr), 0)
        dw, db = X.conv_weight_grad(x, F.pixel_unshuffle(ghr, 2), scale=X.WGRAD_SCALE)
        return xb, gb, dict(g_sub2=True), dw, db, slice(0, 3)
    x2, gy = X.acts((n, cin // 4, 2 * h, 2 * w), g_), X.acts((n, cout, h, w), g_)  # x_sub2, taps {0,1}^2
    gb = abuf(gy)
    xb = ops.ActBuffer.alloc(n, 2 * h, 2 * w, cin // 4, 2, DEV, ha=2 * gb.ha, wa=2 * gb.wa)
    xb.set_nchw(dev(x2), 0)
    # db does not depend on the tap window; the training plans ask for it with this form too
    dw, db = X.conv_weight_grad(X.unshuffle_kernel_order(x2), gy, scale=X.WGRAD_SCALE)
    return xb, gb, dict(x_sub2=True, taps=1), dw, db, slice(0, 2)


def _run_wgrad(xb, cin, gb, cout, want_db, **kw):
    from image_super_resolution_amd import ops
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV) if want_db else None
    ops.wgrad3x3(xb, cin, gb, cout, dw, db, scale=X.WGRAD_SCALE, **kw)
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("cin,cout,kind", WGRAD_FORMS)
def test_wgrad3x3_forms(cin, cout, kind):
    """Every production form of the weight gradient (WGRAD_FORMS of test_gpu_kernels.py) at n = 2,
    17 x 33: dW and db equal the integer sums times 0.5.  With taps=1 only dW's taps {0,1}^2 are
    compared: include/isr.h leaves the other five undefined (the reduce sums workspace rows that the
    2 x 2 kernels never write), so there is nothing to hold them to."""
    xb, gb, kw, rw, rb, taps = _wgrad_form_inputs(cin, cout, kind, X.G_PAST)
    dw, db = _run_wgrad(xb, cin, gb, cout, True, **kw)
    same(dw[..., taps, taps], rw[..., taps, taps].contiguous(), f"dW {kind}")
    same(db, rb, f"db {kind}")


@functools.lru_cache(maxsize=None)
def _split_case(cin, cout, grid):
    return _wgrad_form_inputs(cin, cout, "plain", grid)


@pytest.mark.parametrize("splits", [0, 1, 3, 5])
@pytest.mark.parametrize("cin,cout,grid", X.WGRAD_SPLITS, ids=ids)
def test_wgrad3x3_splits(cin, cout, grid, splits):
    """Any split-K partition sums the same integers: the same bits."""
    xb, gb, _, rw, rb, _ = _split_case(cin, cout, grid)
    dw, db = _run_wgrad(xb, cin, gb, cout, True, splits=splits)
    same(dw, rw, f"dW splits={splits}")
    same(db, rb, f"db splits={splits}")


def test_wgrad3x3_dense_slices():
    """x and g read as channel slices of one dense 192-channel buffer (x_coff, g_coff)."""
    n, h, w = 2, 17, 33
    dense = X.acts((n, 192, h, w), X.gen("wgrad-dense"))
    b = abuf(dense)
    for x_coff, cin, g_coff, cout in [(0, 128, 160, 32), (32, 128, 160, 32), (64, 96, 0, 64)]:
        rw, rb = X.conv_weight_grad(dense[:, x_coff:x_coff + cin], dense[:, g_coff:g_coff + cout], scale=X.WGRAD_SCALE)
        dw, db = _run_wgrad(b, cin, b, cout, True, x_coff=x_coff, g_coff=g_coff)
        same(dw, rw, f"dW x_coff={x_coff} g_coff={g_coff}")
        same(db, rb, f"db x_coff={x_coff} g_coff={g_coff}")


def test_wgrad3x3_group_rdb():
    """isr_wgrad3x3_group on the five RDB members (D = [x | o0 | o1 | o2 | o3], E = [g_out | g_3 | g_2
    | g_1 | g_0]) under both values of ISR_WGRAD_GROUP_ORDER, the single launches, and partials +
    reduce: all equal the exact gradients, and therefore each other, bit for bit.  The variable picks
    the block order only in a tuning build (ISR_LIB), which reads it once per process; the production
    library always runs split-major, so there both passes run the same order."""
    from image_super_resolution_amd import _lib, ops
    lib = _lib.load()
    n, h, w = X.G_PAST
    g_ = X.gen("wgrad-group")
    D, E = X.acts((n, 192, h, w), g_), X.acts((n, 192, h, w), g_)
    Db, Eb = abuf(D), abuf(E)
    refs = [X.conv_weight_grad(D[:, :cin], E[:, gco:gco + cout], scale=sc) for cin, cout, gco, sc in X.RDB_GROUP]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fresh():
        outs = [(torch.full((cout, cin, 3, 3), float("nan"), device=DEV), torch.full((cout,), float("nan"), device=DEV))
                for cin, cout, _, _ in X.RDB_GROUP]
        descs = [ops.wgrad3x3_desc(Db, cin, Eb, cout, dw, db, g_coff=gco, scale=sc)
                 for (cin, cout, gco, sc), (dw, db) in zip(X.RDB_GROUP, outs)]
        return outs, descs

    def check(outs, what):
        for (cin, cout, _, _), (dw, db), (rw, rb) in zip(X.RDB_GROUP, outs, refs):
            same(dw, rw, f"{what}: dW {cin}->{cout}")
            same(db, rb, f"{what}: db {cin}->{cout}")

    old = os.environ.get("ISR_WGRAD_GROUP_ORDER")
    try:
        for order in ("0", "1"):
            os.environ["ISR_WGRAD_GROUP_ORDER"] = order
            outs, descs = fresh()
            arr = (_lib.IsrWgradDesc * 5)(*descs)
            nbytes = lib.isr_wgrad3x3_group_workspace_bytes(arr, 5)
            assert nbytes > 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            assert lib.isr_wgrad3x3_group(arr, 5, ws.data_ptr(), ws.numel(), st) == 0
            torch.cuda.synchronize()
            check(outs, f"group order {order}")
    finally:
        if old is None:
            os.environ.pop("ISR_WGRAD_GROUP_ORDER")
        else:
            os.environ["ISR_WGRAD_GROUP_ORDER"] = old
    outs, descs = fresh()
    for d in descs:
        ops.launch_wgrad3x3(d, DEV)
    torch.cuda.synchronize()
    check(outs, "single launches")
    outs, descs = fresh()
    for d in descs:
        nbytes = lib.isr_wgrad3x3_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
        assert lib.isr_wgrad3x3_partials(ctypes.byref(d), ws.data_ptr(), ws.numel(), st) == 0
        assert lib.isr_wgrad3x3_reduce(ctypes.byref(d), ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    check(outs, "partials + reduce")


@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("grid", X.WGRAD9_GRIDS, ids=ids)
def test_wgrad9x9_tail_and_head(grid, splits):
    from image_super_resolution_amd import ops
    n, h, w = grid
    g_ = X.gen(f"wgrad9-{grid}")
    # tail conv: 64 -> 3, p = the gradient at the output, q = the tail's input
    U, gp = X.acts((n, 64, h, w), g_), X.acts((n, 3, h, w), g_)
    dw, db = torch.full((3, 64, 9, 9), float("nan"), device=DEV), torch.full((3,), float("nan"), device=DEV)
    ops.wgrad9x9(dev(gp).contiguous(), abuf(U, pad=4), dw, db, head=False, scale=X.WGRAD_SCALE, splits=splits)
    torch.cuda.synchronize()
    rw, rb = X.conv_weight_grad(U, gp, k=9, scale=X.WGRAD_SCALE)
    same(dw, rw, "tail dW")
    same(db, rb, "tail db")
    # head conv: 3 -> 64, p = the image, q = the gradient at the head's output
    Xi, gq = X.acts((n, 3, h, w), g_), X.acts((n, 64, h, w), g_)
    dw, db = torch.full((64, 3, 9, 9), float("nan"), device=DEV), torch.full((64,), float("nan"), device=DEV)
    ops.wgrad9x9(dev(Xi).contiguous(), abuf(gq), dw, db, head=True, scale=X.WGRAD_SCALE, splits=splits)
    torch.cuda.synchronize()
    rw, rb = X.conv_weight_grad(Xi, gq, k=9, scale=X.WGRAD_SCALE)
    same(dw, rw, "head dW")
    same(db, rb, "head db")


# ------------------------------------------------------------------ Winograd, one case
def test_conv3x3_wino_equals_direct_on_integers():
    """Weights in {-2, 0, 2}: the pack's (g0 +- g1 + g2) * 0.5 are integers and the fp16 input
    transform of integers in [-3, 3] is exact, so on 160 -> 32, n = 2, 33 x 65 the Winograd form
    equals the float64 reference and the direct fp16 kernel on the same buffers."""
    from image_super_resolution_amd import ops
    x, W, b, v = X.wino_inputs()
    (n, cin, h, w), cout = x.shape, W.shape[0]
    ref = X.round_store(v, FP)
    xb = abuf(x, FP)
    yw = junk(ops.ActBuffer.alloc(n, h, w, cout, 1, DEV, dtype=FP))
    yd = junk(ops.ActBuffer.alloc(n, h, w, cout, 1, DEV, dtype=FP))
    ops.conv3x3_wino(xb, cin, ops.pack_conv3x3_wino(dev(W)), dev(b), cout, yw, slope=X.SLOPE)
    ops.conv3x3(xb, cin, ops.pack_conv3x3(dev(W), f16=True), dev(b), cout, yd, slope=X.SLOPE)
    torch.cuda.synchronize()
    same(yw.to_nchw(), ref, "winograd")
    same(yd.to_nchw(), ref, "direct")
    clean(yw)
    clean(yd)
