"""The opt-in fp16 Winograd F(2,3) 3x3 conv (isr_conv3x3_wino_fwd, ops.conv3x3_wino, the engine's
`wino` option) on the GPU.

Yardstick of every kernel case: tests/wino_ref.py (U and V rounded to fp16, fp64 accumulation,
one final fp16 rounding).  Bar: elementwise |got - ref| <= 2^-9 * max(|ref|, 1) (two fp16 ulps),
at most 2 % of the elements different from ref at all, and exact zeros outside the valid region.
(fp32 accumulation in torch's order against fp64 differs on 0.05-0.14 % of the elements of these
shapes, each a single-ulp flip; the MFMA's summation order is a third order.)

The packed layout is undone on the host in test_pack_matches_ref_bitwise, so the pack case is kept."""
from pathlib import Path

import pytest
import torch

from wino_ref import wino_ref, wino_u

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16 = torch.float16
WEIGHTS_X2 = Path(__file__).parent / "golden" / "trained_resnet_x2.safetensors"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def _mk(n, c, h, w, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, c, h, w, generator=g).to(DEV)


def _w(cout, cin, k, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    s = (1.0 / (cin * k * k)) ** 0.5
    return (torch.rand(cout, cin, k, k, generator=g) * 2 - 1).mul(s * 3 ** 0.5).to(DEV)


def accept(got: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    lim = 2.0 ** -9 * torch.clamp(ref.abs(), min=1.0)
    share = (err > 0).double().mean().item()
    print(f"wino {what}: max err {err.max().item():.3e}, worst err/bound {(err / lim).max().item():.3f}, "
          f"differing {100 * share:.3f} %")
    assert bool((err <= lim).all()), f"max err {err.max().item():.3e} (worst err/bound {(err / lim).max().item():.3f})"
    assert share <= 0.02, f"{100 * share:.3f} % of the elements differ from the reference"


def zero_outside(*bufs) -> None:
    for b in bufs:
        assert b.outside_valid().float().abs().max().item() == 0.0


@pytest.mark.parametrize("n,cin,cout,h,w", [(1, 16, 32, 8, 6), (2, 160, 32, 33, 65), (2, 192, 64, 18, 40),
                                            (1, 64, 64, 7, 5)])
def test_wino_plain(n, cin, cout, h, w):
    """Bias + LeakyReLU 0.01.  (1,16,32,8,6): one chunk, wa = 32, the half-tile guard;
    (2,160,32,33,65): odd w, wa = 96 (a full and a half tile per row), ha = 64."""
    from image_super_resolution_amd import ops
    x = _mk(n, cin, h, w, 1)
    W = _w(cout, cin, 3, 2)
    b = torch.randn(cout, device=DEV) * 0.1
    xb = ops.ActBuffer.from_nchw(x, pad=1, dtype=F16)
    yb = ops.ActBuffer.alloc(n, h, w, cout, 1, DEV, dtype=F16)
    before = xb.t.clone()
    ops.conv3x3_wino(xb, cin, ops.pack_conv3x3_wino(W), b, cout, yb, slope=0.01)
    torch.cuda.synchronize()
    assert yb.t.dtype == F16 and torch.equal(xb.t, before)
    accept(yb.to_nchw(), wino_ref(xb.to_nchw(), W, b, slope=0.01), f"plain {n}x{cin}->{cout} {h}x{w}")
    zero_outside(yb)


def test_wino_growth_in_place():
    """A growth conv writes a higher channel slice of the buffer its input lives in."""
    from image_super_resolution_amd import ops
    n, h, w = 2, 18, 40
    buf = ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=F16)
    buf.set_nchw(_mk(n, 192, h, w, 3), 0)  # channels [96, 192) hold stale data the conv overwrites / skips
    W = _w(32, 96, 3, 4)
    b = torch.randn(32, device=DEV) * 0.1
    before = buf.t.clone()
    xin = buf.to_nchw(0, 96)
    ops.conv3x3_wino(buf, 96, ops.pack_conv3x3_wino(W), b, 32, buf, y_coff=96, slope=0.01)
    torch.cuda.synchronize()
    assert torch.equal(buf.t[:, :6], before[:, :6])  # channels [0, 96) bitwise unchanged
    assert torch.equal(buf.t[:, 8:], before[:, 8:])  # and [128, 192)
    accept(buf.to_nchw(96, 128), wino_ref(xin, W, b, slope=0.01), "growth in place")
    assert buf.t[:, 6:8].float().abs().sum().item() > 0
    p = buf.pad
    border = buf.t[:, 6:8].clone()
    border[:, :, p:p + h, p:p + w] = 0
    assert border.float().abs().max().item() == 0.0


@pytest.mark.parametrize("with_r2", [False, True])
def test_wino_rdb_final_with_residuals(with_r2):
    """192 -> 64, identity activation, r1 = the conv's own input, s1 = 0.2; with r2 / s2 = 0.2
    written in place over r2 (the RRDB residual) and duplicated to y2."""
    from image_super_resolution_amd import ops
    n, h, w = 2, 24, 40
    src = ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=F16)
    src.set_nchw(_mk(n, 192, h, w, 3), 0)
    W = _w(64, 192, 3, 5)
    b = torch.randn(64, device=DEV) * 0.1
    wp = ops.pack_conv3x3_wino(W)
    xin = src.to_nchw(0, 192)
    dst = ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=F16)
    if not with_r2:
        ops.conv3x3_wino(src, 192, wp, b, 64, dst, slope=1.0, r1=src, s1=0.2)
        torch.cuda.synchronize()
        accept(dst.to_nchw(0, 64), wino_ref(xin, W, b, r1=xin[:, :64], s1=0.2), "final r1")
        zero_outside(dst)
        return
    dst.set_nchw(_mk(n, 64, h, w, 6), 0)
    r2 = dst.to_nchw(0, 64)
    y2 = ops.ActBuffer.alloc(n, h, w, 64, 1, DEV, dtype=F16)
    ops.conv3x3_wino(src, 192, wp, b, 64, dst, slope=1.0, r1=src, s1=0.2, r2=dst, s2=0.2, y2=y2)
    torch.cuda.synchronize()
    accept(dst.to_nchw(0, 64), wino_ref(xin, W, b, r1=xin[:, :64], s1=0.2, r2=r2, s2=0.2), "final r1 r2 y2")
    assert torch.equal(dst.to_nchw(0, 64), y2.to_nchw())
    zero_outside(dst, y2)


def test_wino_two_images_and_determinism():
    """n = 2 with different content per image equals the two n = 1 launches bit for bit (the image
    stride), and the same launch twice is bitwise equal."""
    from image_super_resolution_amd import ops
    cin, cout, h, w = 64, 32, 20, 70
    x = _mk(2, cin, h, w, 8)
    assert not torch.equal(x[0], x[1])
    W = _w(cout, cin, 3, 9)
    b = torch.randn(cout, device=DEV) * 0.1
    wp = ops.pack_conv3x3_wino(W)

    def run(xs):
        xb = ops.ActBuffer.from_nchw(xs, pad=1, dtype=F16)
        yb = ops.ActBuffer.alloc(xs.shape[0], h, w, cout, 1, DEV, dtype=F16)
        ops.conv3x3_wino(xb, cin, wp, b, cout, yb, slope=0.01)
        torch.cuda.synchronize()
        return yb.to_nchw()

    both = run(x)
    assert torch.equal(both, run(x))
    assert torch.equal(both[0:1], run(x[0:1])) and torch.equal(both[1:2], run(x[1:2]))
    accept(both, wino_ref(x.half().float(), W, b, slope=0.01), "two images")


def test_pack_matches_ref_bitwise():
    """pack_conv3x3_wino, its layout (include/isr.h) undone on the host, is wino_ref's U bit for bit."""
    from image_super_resolution_amd import ops
    cout, cin = 64, 48
    W = _w(cout, cin, 3, 13)
    packed = ops.pack_conv3x3_wino(W).cpu().view(cin // 16, 3, 4, cout, 2, 8)  # [c16][ky][p][n][hpos][e]
    U = wino_u(W)  # [p][cout][cin][ky] fp16
    hpos = torch.arange(2).view(1, 2) ^ ((torch.arange(cout).view(cout, 1) >> 3) & 1)  # h of (n, hpos)
    # ref[c16][ky][p][n][hpos][e] = U[p][n][c16*16 + h*8 + e][ky]
    Ur = U.view(4, cout, cin // 16, 2, 8, 3)  # [p][n][c16][h][e][ky]
    idx = hpos.view(1, cout, 1, 2, 1, 1).expand(4, cout, cin // 16, 2, 8, 3)
    ref = torch.gather(Ur, 3, idx).permute(2, 5, 0, 1, 3, 4).contiguous()
    assert torch.equal(packed.view(torch.int16), ref.view(torch.int16))


def test_wino_refuses_bf16_and_mixed_storage():
    from image_super_resolution_amd import ops
    W = _w(64, 64, 3, 1)
    xb = ops.ActBuffer.alloc(1, 16, 32, 64, 1, DEV)  # bf16
    yb = ops.ActBuffer.alloc(1, 16, 32, 64, 1, DEV)
    yh = ops.ActBuffer.alloc(1, 16, 32, 64, 1, DEV, dtype=F16)
    with pytest.raises(TypeError):
        ops.conv3x3_wino(xb, 64, ops.pack_conv3x3_wino(W), None, 64, yb)
    with pytest.raises(TypeError):
        ops.conv3x3_wino(xb, 64, ops.pack_conv3x3_wino(W), None, 64, yh)
    with pytest.raises(TypeError):  # bf16 throughout (a direct-form pack): fp16 only
        ops.conv3x3_wino(xb, 64, ops.pack_conv3x3(W), None, 64, yb)


@torch.no_grad()
def test_plan_wino_runs_graphs_and_keys():
    """ResNet(1 block, x2), synthetic weights, 1 x 32 x 32: both options run per conv, the HIP-graph
    replay equals the eager run bitwise, and get_plan's cache tells the options apart."""
    from image_super_resolution_amd import engine, models
    from image_super_resolution_amd.weights import normalize, synth_lr_batch, synth_state_dict
    sd = {k: v.to(DEV) for k, v in synth_state_dict(models.ResNet(1, 0.2, scaleRate=2).state_dict(), 0).items()}
    x = normalize(synth_lr_batch(1, 32, 32, seed=1)[0]).to(DEV).contiguous()
    gw = engine.pack_generator(sd, enchant=False, device=DEV, wino="rdb")
    assert all(pc.ww is not None for blk in gw.rdb for rdb in blk for pc in rdb) and gw.conv1.ww is None
    lib = engine.ops._lib.load()
    outs = {}
    for wino, n_wino in ((None, 0), ("final", 3), ("rdb", 15)):
        plan = engine.GeneratorPlan(gw, 1, 32, 32, torch.device(DEV), False, False, MEAN, STD, chain=False, wino=wino)
        assert plan.chain is None and plan.wino == wino
        assert sum(fn is lib.isr_conv3x3_wino_fwd for fn, _, _, _ in plan.launches) == n_wino
        assert all(tag[0] == "conv3x3" for fn, _, tag, _ in plan.launches if fn is lib.isr_conv3x3_wino_fwd)
        y = torch.empty(plan.out_shape, device=DEV)
        plan.run(x, y)
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        outs[wino] = y.clone()
        if wino:
            gp = engine.GraphedPlan(plan, x, torch.empty_like(y))
            assert torch.equal(gp.run(), y)
            torch.cuda.synchronize()
            # chain=None resolves to per-conv launches under wino
            assert engine.GeneratorPlan(gw, 1, 32, 32, torch.device(DEV), False, False, MEAN, STD,
                                        wino=wino).chain is None
    assert not torch.equal(outs[None], outs["final"]) and not torch.equal(outs["final"], outs["rdb"])
    p0 = engine.get_plan(gw, x, False, MEAN, STD)
    p1 = engine.get_plan(gw, x, False, MEAN, STD, wino="final")
    assert p1 is not p0 and p1.wino == "final" and p0.wino is None
    assert engine.get_plan(gw, x, False, MEAN, STD, wino="final") is p1
    p2 = engine.get_plan(gw, x, False, MEAN, STD, wino="rdb")
    assert p2 is not p1 and p2.wino == "rdb"
    assert torch.equal(engine.run_generator(gw, x, wino="rdb"), outs["rdb"])
    with pytest.raises(ValueError, match="Winograd pack"):  # weights packed without the option
        engine.GeneratorPlan(engine.pack_generator(sd, enchant=False, device=DEV), 1, 32, 32, torch.device(DEV),
                             False, False, MEAN, STD, wino="final")


@torch.no_grad()
def test_trained_x2_generator_wino_vs_direct_vs_oracle():
    """The recipe of test_trained_x2_generator_fp16_vs_bf16_vs_oracle (96 x 128 held-out crop,
    trained x2 weights) per conv, for wino in (None, "final", "rdb"): each Winograd plan agrees with
    the fp32 oracle by >= 70 dB (the project's x2 bar), keeps |dPSNR| vs HR <= 0.002 and stays
    within 1 dB of the direct per-conv plan's agreement (the CPU emulation loses 0.08 / 0.28 dB)."""
    from image_super_resolution_amd import checkpoint, engine, models
    from image_super_resolution_amd.weights import heldout_still
    from oracle import ref_cpu as R
    sd = {k: v.float() for k, v in checkpoint.load_module_state(WEIGHTS_X2).items()}
    net = models.ResNet(16, 0.2, scaleRate=2)
    net.load_state_dict(sd)
    lr, hr = heldout_still(96, 128, 2, device="cpu")
    xin = R.normalize_u8(lr[None])
    ref = R.generator(R.fuse_state_dict(sd), xin, num_blocks=16, scale=2)
    hr1 = hr[None].float() / 127.5 - 1
    dsd = {k: v.to(DEV) for k, v in R.fuse_state_dict(sd).items()}
    x = xin.to(DEV).contiguous()
    gw = engine.pack_generator(dsd, enchant=False, add_rate=0.2, device=DEV, wino="rdb")
    res = {}
    for wino in (None, "final", "rdb"):
        plan = engine.GeneratorPlan(gw, 1, 96, 128, torch.device(DEV), False, False, MEAN, STD, chain=False, wino=wino)
        y = torch.empty(plan.out_shape, device=DEV)
        plan.run(x, y)
        torch.cuda.synchronize()
        y = y.cpu()
        res[wino] = (R.psnr(y, ref), abs(R.psnr(y, hr1) - R.psnr(ref, hr1)))
        del plan
    print("x2 trained, 96x128 crop, per conv: " + ", ".join(
        f"wino={k}: {v[0]:.2f} dB vs oracle (dPSNR {v[1]:.5f})" for k, v in res.items()))
    for wino in ("final", "rdb"):
        assert res[wino][0] >= 70.0, res
        assert res[wino][1] <= 0.002, res
        assert res[wino][0] >= res[None][0] - 1.0, res
