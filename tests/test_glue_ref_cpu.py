"""The ruler of tests/test_gpu_glue.py checked without a GPU: tests/glue_ref.py against torch's own
max_pool2d / leaky_relu and their autograd on the CPU, on inputs where ties and exact zeros are the
rule, so the restatements' tie rule, mask rule and region bookkeeping are pinned independently of
any kernel."""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as G
from image_super_resolution_amd import ops


def _q(shape, seed):
    """Quantised values in {-3 .. 3}: most 2x2 windows hold a tie, many hold zeros."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).float()


def _randn_bf(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return G.bf16r(torch.randn(shape, generator=g))


POOL_SHAPES = [(2, 3, 8, 12), (1, 5, 9, 13), (2, 2, 7, 10), (1, 4, 6, 11), (1, 1, 2, 2), (1, 2, 3, 3)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool2_equals_torch_and_its_autograd(shape):
    x = _q(shape, 1)
    n, c, h, w = shape
    st = torch.stack(G._windows(x))
    tied = ((st == st.max(0).values).sum(0) > 1).sum().item()
    assert tied > 0 or st[0].numel() < 16  # the inputs do exercise the tie rule
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    assert torch.equal(G.maxpool2_fwd(x), y.detach())
    gy = _randn_bf(y.shape, 2)
    y.backward(gy)
    got = G.maxpool2_bwd(x, gy, 1.0)
    assert got.shape == x.shape and torch.equal(got, xr.grad)
    # an odd last row / column belongs to no window
    assert got[:, :, 2 * (h // 2):].abs().sum().item() == 0 and got[:, :, :, 2 * (w // 2):].abs().sum().item() == 0


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool2_bwd_relu_mask_equals_autograd_away_from_zero(shape):
    """mslope = 0 is the backward of max_pool2d(relu(z)) wherever z != 0: a window with a positive
    maximum has the same first maximum before and after the clamp, and a window without one gets no
    gradient either way (relu' = 0 at every position of it)."""
    z = _q(shape, 3)
    zr = z.clone().requires_grad_(True)
    y = F.max_pool2d(F.relu(zr), 2)
    gy = _randn_bf(y.shape, 4)
    y.backward(gy)
    got = G.maxpool2_bwd(z, gy, 0.0)
    keep = z != 0
    assert keep.any()
    assert torch.equal(got[keep], zr.grad[keep])


@pytest.mark.parametrize("mslope", [0.2, 0.0, 0.01])
def test_ew_combine_mask_is_leaky_relu_backward(mslope):
    m = _randn_bf((2, 16, 5, 7), 5)
    m[0, :, 1, :3] = 0.0
    m[1, :, 2, 2:6] = -0.0
    g = _randn_bf(m.shape, 6)
    mr = m.clone().requires_grad_(True)
    F.leaky_relu(mr, mslope).backward(g)
    got = G.ew_combine(g, 1.0, m=m, mslope=mslope)
    assert torch.equal(got, G.bf16r(mr.grad))
    # both zeros take mslope
    assert torch.equal(got[0, :, 1, :3], G.bf16r(g[0, :, 1, :3] * mslope))
    assert torch.equal(got[1, :, 2, 2:6], G.bf16r(g[1, :, 2, 2:6] * mslope))


def test_ew_combine_sum_and_order():
    a, b = _randn_bf((1, 16, 4, 6), 7), _randn_bf((1, 16, 4, 6), 8)
    m = _randn_bf(a.shape, 9)
    assert torch.equal(G.ew_combine(a, 1.0), a)
    assert torch.equal(G.ew_combine(a, -2.0, b, 0.5), G.bf16r(b * 0.5 - 2.0 * a))
    # general scalars: one bf16 rounding of the masked fp32 sum, so within a half-ulp of the fp64 value
    sa, sb, ms = 0.3, -1.7, 0.2
    exact = torch.where(m > 0, 1.0, ms).double() * (a.double() * float(torch.tensor(sa)) +
                                                     b.double() * float(torch.tensor(sb)))
    got = G.ew_combine(a, sa, b, sb, m, ms)
    assert bool(((got.double() - exact).abs() <= 2.0 ** -8 * exact.abs() + 1e-6).all())


@pytest.mark.parametrize("c,c_pad", [(3, 16), (20, 32), (64, 64)])
def test_layout_round_trip_is_bf16_rounding(c, c_pad):
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, c, 5, 9, generator=g)
    v = G.nchw_to_blocked(x, c_pad=c_pad)
    assert v.shape == (2, c_pad, 5, 9) and v[:, c:].abs().sum().item() == 0
    back = G.blocked_to_nchw(v[:, :c])
    assert back.dtype == torch.float32 and torch.equal(back, G.bf16r(x))
    # through a real buffer: set_nchw / interior are the same layout
    buf = ops.ActBuffer.alloc(2, 5, 9, c_pad, 1, "cpu")
    buf.set_nchw(v)
    assert torch.equal(buf.to_nchw(0, c), G.bf16r(x))


def test_layout_affine_and_mask():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 3, 4, 5, generator=g)
    scale, shift = torch.tensor([2.0, 0.5, -4.0]), torch.tensor([0.25, -1.0, 3.0])
    m = _randn_bf((1, 16, 4, 5), 12)
    m[0, :, 0, :2] = 0.0
    m[0, :, 1, :2] = -0.0
    got = G.nchw_to_blocked(x, scale, shift, m, 0.0)
    aff = x * scale.view(1, 3, 1, 1) + shift.view(1, 3, 1, 1)
    assert torch.equal(got[:, :3], G.bf16r(torch.where(m[:, :3] > 0, aff, torch.zeros(()))))
    assert got[0, :3, 0, :2].abs().sum().item() == 0 and got[0, :3, 1, :2].abs().sum().item() == 0
    v = G.bf16r(x)
    # powers of two: the product is exact, the sum rounds once
    want = (v.double() * scale.double().view(1, 3, 1, 1) + shift.double().view(1, 3, 1, 1)).float()
    assert torch.equal(G.blocked_to_nchw(v, scale, shift), want)


def test_pack_layout_restates_isr_h():
    """out[c16][tap][n][hpos][e] = W[n][c16*16 + (hpos ^ ((n >> 3) & 1))*8 + e][tap], element by element."""
    g = torch.Generator().manual_seed(13)
    cout, cin = 32, 48
    W = torch.randn(cout, cin, 3, 3, generator=g)
    fwd = G.pack_conv3x3(W).view(cin // 16, 9, cout, 2, 8)
    dg = G.pack_conv3x3(W, dgrad=True, scale=0.25).view(cout // 16, 9, cin, 2, 8)
    Wf = W.reshape(cout, cin, 9)
    for c16, tap, n, hpos, e in [(0, 0, 0, 0, 0), (2, 8, 9, 0, 3), (1, 4, 31, 1, 7), (2, 5, 16, 1, 0)]:
        ci = c16 * 16 + (hpos ^ ((n >> 3) & 1)) * 8 + e
        assert fwd[c16, tap, n, hpos, e] == Wf[n, ci, tap].to(torch.bfloat16)
    for c16, tap, n, hpos, e in [(0, 0, 0, 0, 0), (1, 8, 9, 0, 3), (1, 4, 47, 1, 7), (0, 5, 24, 1, 0)]:
        co = c16 * 16 + (hpos ^ ((n >> 3) & 1)) * 8 + e
        assert dg[c16, tap, n, hpos, e] == (Wf[co, n, 8 - tap] * 0.25).to(torch.bfloat16)
    # sub2: input channel ci = s*(cout/4) + c stands for layer output channel 4c + s
    W2 = torch.randn(128, 32, 3, 3, generator=g)
    s2 = G.pack_conv3x3(W2, dgrad=True, sub2=True).view(8, 9, 32, 2, 8)
    for c16, tap, n, hpos, e in [(0, 0, 0, 0, 0), (5, 2, 11, 1, 6), (7, 7, 31, 0, 7)]:
        ci = c16 * 16 + (hpos ^ ((n >> 3) & 1)) * 8 + e
        co = (ci % 32) * 4 + ci // 32
        assert s2[c16, tap, n, hpos, e] == W2.reshape(128, 32, 9)[co, n, 8 - tap].to(torch.bfloat16)


def test_regions_partition_a_buffer():
    buf = ops.ActBuffer.alloc(2, 20, 36, 64, 2, "cpu", ha=64, wa=96, min_hp=80, min_wp=70)
    assert tuple(buf.t.shape) == (2, 4, 80, 100, 16)
    for coff, c in ((16, 20), (0, 64), (48, 3)):
        i, ii, iii = G.regions(buf, coff, c)
        assert not (i & ii).any() and not (i & iii).any() and not (ii & iii).any()
        assert bool((i | ii | iii).all())
        planes = G.round16(c) // 16
        assert i.sum().item() == 2 * planes * 20 * 36 * 16
        assert ii.sum().item() == 2 * planes * (64 * 96 - 20 * 36) * 16
        # (i) is what interior() addresses; the border ring and the other planes are in (iii)
        buf.t.zero_()
        buf.t[i] = 1
        assert buf.interior(coff, coff + G.round16(c)).float().min().item() == 1
        assert buf.to_nchw().sum().item() == i.sum().item()
        assert bool(iii[:, :, :2].all()) and bool(iii[:, :, :, :2].all()) and bool(iii[:, :, 66:].all())
        assert bool(iii[:, :coff // 16].all()) and bool(iii[:, coff // 16 + planes:].all())
