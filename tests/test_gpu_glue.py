"""The glue kernels around the convs, bit for bit against tests/glue_ref.py: isr_ew_combine,
isr_nchw_to_blocked / isr_blocked_to_nchw, isr_maxpool2_fwd / isr_maxpool2_bwd and
isr_pack_conv3x3_batch (its dgrad windows and packs written inside a larger pack).

Each of them is a single-rounding operation, so wherever the fp32 products are exact (no scale, or
scales that are powers of two) the yardstick is torch.equal.  The only tolerances are two derived
bounds for general scalars against an fp64 value (a bf16 half-ulp, 2^-8 |ref|, plus the fp32
roundings with or without FMA contraction, 2^-21 of the summed magnitudes; for the fp32 output of
isr_blocked_to_nchw 2^-22 (|v scale| + |ref|)) and test_gpu_kernels.py's `close` bar for the one
conv run on an assembled pack.

Discipline of every case: inputs go in with ActBuffer.set_nchw and outputs come out of ActBuffer.t
(plain torch, independent of the kernels under test).  Every input buffer is filled with JUNK
outside the values set (border, alignment slack, other channels), the whole output tensor with
SENTINEL before the launch; afterwards the valid interior of the written channel slice equals the
reference, the computed-but-invalid part of that slice is exactly zero, and everything else (border
ring, rows / columns past ha / wa, other channels) still holds the sentinel.  Mask sources hold a
block of +0.0 and of -0.0; pool inputs are drawn from {-3 .. 3} so that ties are the rule.

Not covered: the 64-bit index path of the elementwise launches (2^31 or more element groups) needs
tens of GB per operand."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import glue_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL, JUNK = 7.0, 3.0
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


# ------------------------------------------------------------------ helpers
def _randn(shape, seed, bf=True):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    return (G.bf16r(x) if bf else x).to(DEV)


def _mask_src(shape, seed):
    """bf16 randn with a block of exact +0.0 and one of -0.0 (both must take mslope)."""
    m = _randn(shape, seed)
    m[:, :, :2, :2] = 0.0
    m[:, :, 2:4, 1:3] = -0.0
    assert (m == 0).sum().item() >= 2 * shape[0] * shape[1]
    return m


def _quant(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).float().to(DEV)


def _f32(v: float) -> float:
    """The value a C float field receives."""
    return ctypes.c_float(v).value


def _filled(n, h, w, c, fill, **kw):
    from image_super_resolution_amd import ops
    b = ops.ActBuffer.alloc(n, h, w, c, 1, DEV, **kw)
    b.t.fill_(fill)
    return b


def _input(x, c_total=None, coff=0, **kw):
    """A JUNK-filled buffer holding x (NCHW, a multiple of 16 channels) at channel coff."""
    n, c, h, w = x.shape
    b = _filled(n, h, w, c_total or c, JUNK, **kw)
    b.set_nchw(x, coff)
    return b


def _check_written(y, coff, c, ref=None):
    """The three regions of an output buffer after a launch into channels [coff, coff + round16(c));
    ref (NCHW, round16(c) channels) None skips the interior."""
    i, ii, iii = G.regions(y, coff, c)
    if ref is not None:
        got = y.interior(coff, coff + G.round16(c)).float()
        assert got.shape == ref.shape
        if not torch.equal(got, ref):
            bad = got != ref
            k = bad.nonzero()[0].tolist()
            raise AssertionError(f"{int(bad.sum())} of {bad.numel()} interior elements differ; first at {k}: "
                                 f"got {got[tuple(k)].item()!r}, want {ref[tuple(k)].item()!r}")
    assert bool((y.t[ii] == 0).all()), "computed-but-invalid positions are not exactly zero"
    assert bool((y.t[iii] == SENTINEL).all()), "a write outside the computed region of the channel slice"


def _unchanged(*pairs):
    for buf, before in pairs:
        assert torch.equal(buf.t, before), "an input buffer was written"


def close(got, ref, tol=1.5e-2, mean_tol=2e-3):
    """test_gpu_kernels.py's conv bar."""
    err = (got - ref).abs()
    lim = tol * torch.clamp(ref.abs(), min=1.0)
    assert bool((err <= lim).all()), f"max err {err.max().item():.3e} (ref max {ref.abs().max().item():.3e})"
    assert err.mean().item() < mean_tol, f"mean err {err.mean().item():.3e}"


# ------------------------------------------------------------------ isr_ew_combine
SCALARS = [(1.0, 1.0), (0.5, -2.0), (-2.0, 0.5)]  # exact products: contraction cannot change a bit


@pytest.mark.parametrize("sa,sb", SCALARS)
def test_ew_combine_b_and_mask(sa, sb):
    """(2, 32, 7, 45): two images, two planes, odd sizes far from the 32 x 64 computed region."""
    from image_super_resolution_amd import ops
    shape = (2, 32, 7, 45)
    a, b, m = _randn(shape, 1), _randn(shape, 2), _mask_src(shape, 3)
    ab, bb, mb = _input(a), _input(b), _input(m)
    y = _filled(2, 7, 45, 32, SENTINEL)
    before = [(t, t.t.clone()) for t in (ab, bb, mb)]
    ops.ew_combine(y, ab, 32, sa=sa, b=bb, sb=sb, m=mb, mslope=0.2)
    torch.cuda.synchronize()
    _check_written(y, 0, 32, G.ew_combine(a, sa, b, sb, m, 0.2))
    _unchanged(*before)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("sa,sb", SCALARS)
def test_ew_combine_channel_slices(sa, sb, in_place):
    """(1, 64, 33, 65): a, b, m, y each another 64-channel slice (64, 128, 0, 64) of 192-channel
    buffers; in place, y is a's buffer and slice."""
    from image_super_resolution_amd import ops
    shape = (1, 64, 33, 65)
    a, b, m = _randn(shape, 4), _randn(shape, 5), _mask_src(shape, 6)
    ab = _input(a, 192, 64) if not in_place else None
    bb, mb = _input(b, 192, 128), _input(m, 192, 0)
    y = _filled(1, 33, 65, 192, SENTINEL)
    if in_place:
        y.set_nchw(a, 64)
        ab = y
    before = [(t, t.t.clone()) for t in (bb, mb) + (() if in_place else (ab,))]
    ops.ew_combine(y, ab, 64, sa=sa, b=bb, sb=sb, m=mb, mslope=0.2, y_coff=64, a_coff=64, b_coff=128, m_coff=0)
    torch.cuda.synchronize()
    _check_written(y, 64, 64, G.ew_combine(a, sa, b, sb, m, 0.2))
    _unchanged(*before)


@pytest.mark.parametrize("sa", [1.0, 0.5, -2.0])
def test_ew_combine_a_only(sa):
    """(1, 16, 5, 3): one plane, neither b nor m."""
    from image_super_resolution_amd import ops
    a = _randn((1, 16, 5, 3), 7)
    ab = _input(a)
    y = _filled(1, 5, 3, 16, SENTINEL)
    ops.ew_combine(y, ab, 16, sa=sa)
    torch.cuda.synchronize()
    _check_written(y, 0, 16, G.ew_combine(a, sa))


def test_ew_combine_grid_stride_loop():
    """(5, 64, 225, 250) with ha = wa = 256: 2.6 M threads against the 8192 x 256 grid cap, the one
    case whose threads run the grid-stride loop more than once."""
    from image_super_resolution_amd import ops
    n, c, h, w = 5, 64, 225, 250
    assert n * 256 * 256 * (c // 8) > 8192 * 256
    g = torch.Generator(device=DEV).manual_seed(8)
    a, b, m = (G.bf16r(torch.randn(n, c, h, w, device=DEV, generator=g)) for _ in range(3))
    m[:, :, 100:110, 200:250] = 0.0
    m[:, :, 220:225, :64] = -0.0
    kw = dict(ha=256, wa=256)
    ab, bb, mb = _input(a, **kw), _input(b, **kw), _input(m, **kw)
    y = _filled(n, h, w, c, SENTINEL, **kw)
    ops.ew_combine(y, ab, c, sa=0.5, b=bb, sb=-2.0, m=mb, mslope=0.2)
    torch.cuda.synchronize()
    _check_written(y, 0, c, G.ew_combine(a, 0.5, b, -2.0, m, 0.2))


def test_ew_combine_general_scalars_within_derived_bound():
    """sa = 0.3, sb = -1.7 against fp64: |err| <= 2^-8 |ref| + 2^-21 (|a sa| + |b sb|) — the bf16
    half-ulp plus the fp32 roundings of two products, a sum and the mask factor, with or without
    contraction (derived, not measured)."""
    from image_super_resolution_amd import ops
    shape = (2, 32, 7, 45)
    a, b, m = _randn(shape, 9), _randn(shape, 10), _mask_src(shape, 11)
    y = _filled(2, 7, 45, 32, SENTINEL)
    ops.ew_combine(y, _input(a), 32, sa=0.3, b=_input(b), sb=-1.7, m=_input(m), mslope=0.2)
    torch.cuda.synchronize()
    _check_written(y, 0, 32)
    pa, pb = a.double() * _f32(0.3), b.double() * _f32(-1.7)
    ref = (pa + pb) * torch.where(m > 0, 1.0, _f32(0.2)).double()
    err = (y.interior().double() - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + 2.0 ** -21 * (pa.abs() + pb.abs())
    print(f"ew general scalars: max err {err.max().item():.3e}, worst err/bound {(err / lim).max().item():.3f}")
    assert bool((err <= lim).all())


# ------------------------------------------------------------------ layout conversion
GRIDS = [(2, 20, 36), (1, 33, 65)]
# (c, channels of v's buffer, v_coff, mslope of the mask at m_coff = 64 of a 128-channel buffer or None)
TO_BLOCKED = [(3, 16, 0, None), (20, 64, 16, None), (64, 64, 0, 0.0), (64, 64, 0, 0.2)]


def _affine(c, kind, seed):
    if kind == "none":
        return None, None
    g = torch.Generator(device="cpu").manual_seed(seed)
    shift = torch.randn(c, generator=g)
    if kind == "pow2":
        scale = torch.tensor([2.0, 0.5, -4.0, 1.0, -0.25])[torch.randint(0, 5, (c,), generator=g)]
    else:
        scale = torch.randn(c, generator=g) + 1.5
    return scale.to(DEV), shift.to(DEV)


@pytest.mark.parametrize("affine", ["none", "pow2", "general"])
@pytest.mark.parametrize("n,h,w", GRIDS)
@pytest.mark.parametrize("c,cbuf,coff,mslope", TO_BLOCKED)
def test_nchw_to_blocked(c, cbuf, coff, mslope, n, h, w, affine):
    """c = 3 into a 16-channel buffer (the VGG input); c = 20 into channels [16, 48) of 64 (a partial
    last plane, planes 0 and 3 keep the sentinel); c = 64 with the LeakyReLU' / ReLU' mask of the VGG
    and discriminator backward entries.  Exact without an affine and with power-of-two scales; a
    general affine within 2^-8 |ref| + 2^-21 (|x scale| + |shift|) of the fp64 value."""
    from image_super_resolution_amd import ops
    x = _randn((n, c, h, w), 20 + c, bf=False)  # fp32 values: the kernel does the rounding
    scale, shift = _affine(c, affine, 30 + c)
    m = mb = None
    if mslope is not None:
        m = _mask_src((n, 64, h, w), 40)
        mb = _input(m, 128, 64)
    v = _filled(n, h, w, cbuf, SENTINEL)
    ops.nchw_to_blocked(x, v, v_coff=coff, scale=scale, shift=shift, m=mb, mslope=mslope or 0.0, m_coff=64)
    torch.cuda.synchronize()
    if affine != "general":
        _check_written(v, coff, c, G.nchw_to_blocked(x, scale, shift, m, mslope or 0.0))
        return
    _check_written(v, coff, c)
    got = v.interior(coff, coff + G.round16(c)).double()
    assert bool((got[:, c:] == 0).all())
    px, sh = x.double() * scale.double().view(1, c, 1, 1), shift.double().view(1, c, 1, 1)
    ref = px + sh
    if m is not None:
        ref = ref * torch.where(m > 0, 1.0, _f32(mslope)).double()
    err = (got[:, :c] - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + 2.0 ** -21 * (px.abs() + sh.abs())
    print(f"nchw_to_blocked general affine: worst err/bound {(err / lim).max().item():.3f}")
    assert bool((err <= lim).all())


@pytest.mark.parametrize("affine", ["none", "pow2", "general"])
@pytest.mark.parametrize("n,h,w", GRIDS)
@pytest.mark.parametrize("c,cbuf,coff", [(3, 32, 0), (20, 64, 16), (64, 64, 0)])
def test_blocked_to_nchw(c, cbuf, coff, n, h, w, affine):
    """c = 3 of a 32-channel buffer (the VGG input gradient), c = 20 from channel 16, c = 64, into a
    slice of a larger sentinel-filled fp32 tensor.  fp32 out: exact without an affine and with
    power-of-two scales; a general affine within 2^-22 (|v scale| + |ref|) of the fp64 value."""
    from image_super_resolution_amd import ops
    c16 = G.round16(c)
    vals = _randn((n, c16, h, w), 50 + c)
    vb = _input(vals, cbuf, coff)
    before = vb.t.clone()
    scale, shift = _affine(c, affine, 60 + c)
    guard, numel = 1024, n * c * h * w
    big = torch.full((numel + 2 * guard,), SENTINEL, device=DEV)
    out = big[guard:guard + numel].view(n, c, h, w)
    ops.blocked_to_nchw(vb, out, v_coff=coff, scale=scale, shift=shift)
    torch.cuda.synchronize()
    assert bool((big[:guard] == SENTINEL).all()) and bool((big[guard + numel:] == SENTINEL).all())
    _unchanged((vb, before))
    v = vals[:, :c]
    if affine != "general":
        assert torch.equal(out, G.blocked_to_nchw(v, scale, shift))
        return
    pv = v.double() * scale.double().view(1, c, 1, 1)
    ref = pv + shift.double().view(1, c, 1, 1)
    err = (out.double() - ref).abs()
    lim = 2.0 ** -22 * (pv.abs() + ref.abs())
    print(f"blocked_to_nchw general affine: worst err/bound {(err / lim.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= lim).all())


# ------------------------------------------------------------------ 2x2 max pool
# (n, c, h, w, channels of the buffers): aligned; valid smaller than computed; the output grid
# crosses one tile (in a buffer with a spare plane); odd: the last row and column are in no window
POOL = [(2, 32, 32, 64, 32), (1, 64, 20, 36, 64), (1, 16, 34, 70, 32), (1, 32, 33, 71, 32)]


def _pool_buffers(n, c, h, w, cbuf, x, gy=None):
    """x, y (and the input-gradient buffer g) allocated as VGGPlan does: ha = 2 * y.ha, wa = 2 * y.wa."""
    y = _filled(n, h // 2, w // 2, cbuf, JUNK if gy is not None else SENTINEL)
    kw = dict(ha=2 * y.ha, wa=2 * y.wa)
    xb = _filled(n, h, w, cbuf, JUNK, **kw)
    xb.set_nchw(x, 0)
    if gy is None:
        return xb, y, None
    y.set_nchw(gy, 0)
    return xb, y, _filled(n, h, w, cbuf, SENTINEL, **kw)


@pytest.mark.parametrize("n,c,h,w,cbuf", POOL)
def test_maxpool2_fwd(n, c, h, w, cbuf):
    from image_super_resolution_amd import ops
    x = _quant((n, c, h, w), 70)
    xb, y, _ = _pool_buffers(n, c, h, w, cbuf, x)
    before = xb.t.clone()
    ops.maxpool2_fwd(xb, y, c)
    torch.cuda.synchronize()
    _check_written(y, 0, c, G.maxpool2_fwd(x))
    _unchanged((xb, before))


@pytest.mark.parametrize("mslope", [0.0, 1.0, 0.2])
@pytest.mark.parametrize("n,c,h,w,cbuf", POOL)
def test_maxpool2_bwd(n, c, h, w, cbuf, mslope):
    """The gradient goes to the first maximum of each window, times mslope where not (x > 0) there;
    the output gradient's own alignment slack holds JUNK, which must not reach g (an odd last
    row / column and the computed-but-invalid windows get exact zeros)."""
    from image_super_resolution_amd import ops
    x = _quant((n, c, h, w), 71)
    gy = _randn((n, c, h // 2, w // 2), 72)
    xb, yb, g = _pool_buffers(n, c, h, w, cbuf, x, gy)
    before = [(xb, xb.t.clone()), (yb, yb.t.clone())]
    ops.maxpool2_bwd(xb, yb, g, c, mslope=mslope)
    torch.cuda.synchronize()
    ref = G.maxpool2_bwd(x, gy, mslope)
    assert (ref != 0).sum().item() > 0
    _check_written(g, 0, c, ref)
    _unchanged(*before)


def test_maxpool2_grid_stride_loop():
    """(3, 128, 390, 400), output region 224 x 224: 2.4 M threads against the 8192 x 256 grid cap, so
    the first 311 296 threads take a second window 2 097 152 / (2 * 224 * 224) = 20.9 planes on, at
    another pixel: valid and computed-but-invalid windows alternate within one thread."""
    from image_super_resolution_amd import ops
    n, c, h, w = 3, 128, 390, 400
    assert n * 224 * 224 * (c // 8) > 8192 * 256
    g = torch.Generator(device=DEV).manual_seed(73)
    x = torch.randint(-3, 4, (n, c, h, w), device=DEV, generator=g).float()
    gy = G.bf16r(torch.randn(n, c, h // 2, w // 2, device=DEV, generator=g))
    xb, y, _ = _pool_buffers(n, c, h, w, c, x)
    assert (y.ha, y.wa) == (224, 224)
    ops.maxpool2_fwd(xb, y, c)
    torch.cuda.synchronize()
    _check_written(y, 0, c, G.maxpool2_fwd(x))
    del y
    xb, yb, gb = _pool_buffers(n, c, h, w, c, x, gy)
    ops.maxpool2_bwd(xb, yb, gb, c, mslope=0.2)
    torch.cuda.synchronize()
    _check_written(gb, 0, c, G.maxpool2_bwd(x, gy, 0.2))


# ------------------------------------------------------------------ isr_pack_conv3x3_batch
def _w(cout, cin, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    s = (3.0 / (cin * 9)) ** 0.5
    return ((torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) * s).to(DEV)


def _packed_len(cout, cin):
    return cout * cin * 9


def _run_items(items):
    from image_super_resolution_amd import ops
    ops.pack_batch(ops.pack_batch_table(items, DEV))
    torch.cuda.synchronize()


def _words(t):
    return t.view(torch.int16)


def test_pack_batch_forward_and_dgrad_items():
    """One table: two forward items, a dgrad item with scale 0.25 and a sub2 dgrad item at cout 128.
    Each equals its single-pack entry point and the layout restated in glue_ref, word for word."""
    from image_super_resolution_amd import ops
    Wa, Wb, Wc, Wd = _w(32, 64, 1), _w(64, 192, 2), _w(32, 160, 3), _w(128, 64, 4)
    outs = [torch.full((_packed_len(*w.shape[:2]),), SENTINEL, dtype=BF16, device=DEV) for w in (Wa, Wb, Wc, Wd)]
    _run_items([(Wa, outs[0], 32, 64, False, False, 1.0), (Wb, outs[1], 64, 192, False, False, 1.0),
                (Wc, outs[2], 32, 160, True, False, 0.25), (Wd, outs[3], 128, 64, True, True, 0.25)])
    refs = [(ops.pack_conv3x3(Wa), G.pack_conv3x3(Wa)), (ops.pack_conv3x3(Wb), G.pack_conv3x3(Wb)),
            (ops.pack_conv3x3_dgrad(Wc, 0.25), G.pack_conv3x3(Wc, True, 0.25)),
            (ops.pack_conv3x3_dgrad(Wd, 0.25, sub2=True), G.pack_conv3x3(Wd, True, 0.25, True))]
    torch.cuda.synchronize()
    for out, (single, restated) in zip(outs, refs):
        assert torch.equal(_words(out), _words(single))
        assert torch.equal(_words(out), _words(restated))


@pytest.mark.parametrize("cout,src_cin,n0,cin", [(32, 160, 96, 32), (64, 192, 0, 64), (64, 192, 128, 32)])
def test_pack_batch_dgrad_window(cout, src_cin, n0, cin):
    """A window item packs input channels [n0, n0 + cin) of a layer with src_cin of them: the dgrad
    pack of that weight slice."""
    from image_super_resolution_amd import ops
    W = _w(cout, src_cin, 5)
    lead = 64
    big = torch.full((lead + _packed_len(cout, cin) + 64,), SENTINEL, dtype=BF16, device=DEV)
    _run_items([(W, big, cout, cin, True, False, 0.25, n0, src_cin, lead)])
    sl = W[:, n0:n0 + cin].contiguous()
    got = big[lead:lead + _packed_len(cout, cin)]
    assert torch.equal(_words(got), _words(ops.pack_conv3x3_dgrad(sl, 0.25)))
    assert torch.equal(_words(got), _words(G.pack_conv3x3(sl, True, 0.25)))
    assert bool((big[:lead] == SENTINEL).all()) and bool((big[lead + got.numel():] == SENTINEL).all())


def _gather_blocks(W5, W3, W2, out, scale5):
    """The items of train_engine._gather_items for the RDB dense-buffer block [96, 128) (its input is
    [g_f | g_3 | g_2], 128 channels): (weights, layer cout, input-channel offset of the block)."""
    n0, co = 96, 32
    blocks = [(W5, 64, 0, scale5), (W3, 32, 64, 1.0), (W2, 32, 96, 1.0)]
    return [(w, out, lc, co, True, False, sc, n0, w.shape[1], (off // 16) * 9 * co * 16)
            for w, lc, off, sc in blocks], blocks


def test_pack_batch_blocks_inside_one_pack_and_the_conv_over_it():
    """Three window items write at element offsets (off // 16) * 9 * co * 16 inside one buffer: each
    block equals its own single pack, a table without the middle item leaves that block's words
    alone, nothing before or after the pack is written, and isr_conv3x3_fwd over [g_f | g_3 | g_2]
    with the assembled pack is the sum of the three transposed convs."""
    from image_super_resolution_amd import ops
    W5, W3, W2 = _w(64, 192, 6), _w(32, 160, 7), _w(32, 128, 8)
    n0, co, lead, total = 96, 32, 64, _packed_len(32, 128)
    big = torch.full((lead + total + 64,), SENTINEL, dtype=BF16, device=DEV)
    items, blocks = _gather_blocks(W5, W3, W2, big[lead:], 0.25)
    singles = [ops.pack_conv3x3_dgrad(w[:, n0:n0 + co].contiguous(), sc) for w, _, _, sc in blocks]
    torch.cuda.synchronize()
    spans = [(it[9], it[9] + s.numel()) for it, s in zip(items, singles)]
    assert spans == [(0, 18432), (18432, 27648), (27648, total)]

    _run_items([items[0], items[2]])
    pack = big[lead:lead + total]
    assert torch.equal(_words(pack[0:18432]), _words(singles[0]))
    assert bool((pack[18432:27648] == SENTINEL).all())
    assert torch.equal(_words(pack[27648:]), _words(singles[2]))

    _run_items(items)
    for (lo, hi), s in zip(spans, singles):
        assert torch.equal(_words(pack[lo:hi]), _words(s))
    assert bool((big[:lead] == SENTINEL).all()) and bool((big[lead + total:] == SENTINEL).all())

    n, h, w = 1, 20, 36
    g = _randn((n, 128, h, w), 9)
    xb = ops.ActBuffer.from_nchw(g, pad=1)
    yb = ops.ActBuffer.alloc(n, h, w, 32, 1, DEV)
    ops.conv3x3(xb, 128, pack, None, 32, yb)
    torch.cuda.synchronize()
    gc = g.cpu()
    ref = sum(F.conv_transpose2d(gc[:, off:off + lc], G.bf16r(wt.cpu())[:, n0:n0 + co], padding=1) * sc
              for wt, lc, off, sc in blocks)
    close(yb.to_nchw().cpu(), ref)
    assert yb.outside_valid().float().abs().max().item() == 0.0
