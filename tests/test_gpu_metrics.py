"""isr_image_metrics / metrics.image_metrics / trainer.validate / the CLIs on the GPU, against the fp64
restatement tests/metrics_ref.py.

Bars (set by the definitions, not by what the kernel gives):
* mse of two uint8 images is == the exact integer sum of squares divided once;
* every other mse and every mse_y: relative error <= 1e-5 (the luma difference is formed from the
  channel differences, so nothing cancels; fp32 partial sums over <= 16 values would give 1e-6);
* ssim_y: |delta| <= 1e-6 in every case, the flat image included, which a plain fp32 evaluation of
  E[x^2] - mu^2 at x ~ 200 misses by 5e-5 to 1e-4 (fp64 moments give about 1e-11).
"""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_ref as M
from image_super_resolution_amd import _lib, checkpoint, data, metrics, models, trainer
from image_super_resolution_amd.weights import heldout_tiles
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
WEIGHTS = Path(__file__).parent / "golden" / "trained_resnet_x4.safetensors"

# (n, h, w, border): one window; ragged, odd, unaligned uint8 rows; several tiles high, ragged both
# ways; window tiles exactly 32 x 64; one row and one column past a tile; the remaining ragged case
SHAPES = [(1, 19, 19, 4), (2, 37, 53, 4), (3, 75, 43, 4), (1, 42, 74, 0), (1, 43, 75, 0), (2, 51, 52, 4)]
KINDS = [("u8", "u8"), ("tanh", "u8"), ("tanh", "norm")]


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def content(kind: str, n: int, h: int, w: int, seed: int):
    """(estimate, truth) in [0, 1], float64, from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return (torch.rand(n, 3, h, w, generator=g, dtype=torch.float64),
                torch.rand(n, 3, h, w, generator=g, dtype=torch.float64))
    if kind == "smooth":
        base = torch.rand(n, 3, 5, 6, generator=g, dtype=torch.float64)
        b = F.interpolate(base, size=(h, w), mode="bicubic", align_corners=False).clamp(0, 1)
        return (b + 0.02 * torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)).clamp(0, 1), b
    if kind == "flat":  # every pixel 200 against the same plus Gaussian noise of sigma 4
        b = torch.full((n, 3, h, w), 200.0 / 255.0, dtype=torch.float64)
        return b + (4.0 / 255.0) * torch.randn(n, 3, h, w, generator=g, dtype=torch.float64), b
    raise ValueError(kind)


def encode(x01: torch.Tensor, space: str) -> torch.Tensor:
    if space == "u8":
        return (x01.clamp(0, 1) * 255).round().to(torch.uint8)
    if space == "tanh":
        return (x01 * 2 - 1).float()
    if space == "norm":
        return ((x01 - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)).float()
    return x01.float()


def check(got: metrics.Metrics, want: dict, what: str, exact_mse=None):
    mse, mse_y, ssim = got.mse.cpu(), got.mse_y.cpu(), got.ssim_y.cpu()
    rel = lambda a, b: ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()  # noqa: E731
    e_mse, e_y, e_s = rel(mse, want["mse"]), rel(mse_y, want["mse_y"]), (ssim - want["ssim_y"]).abs().max().item()
    print(f"{what}: mse rel {e_mse:.2e}, mse_y rel {e_y:.2e}, ssim abs {e_s:.2e}")
    if exact_mse is not None:
        assert mse.tolist() == exact_mse, (what, mse.tolist(), exact_mse)
    assert e_mse <= 1e-5, (what, e_mse)
    assert e_y <= 1e-5, (what, e_y)
    assert e_s <= 1e-6, (what, e_s)
    assert torch.allclose(got.psnr.cpu(), -10 * torch.log10(mse), rtol=0, atol=1e-9)  # inf where mse is 0
    assert torch.allclose(got.psnr_y.cpu(), -10 * torch.log10(mse_y), rtol=0, atol=1e-9)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_restatement(shape):
    n, h, w, border = shape
    for ci, kind in enumerate(("noise", "smooth", "flat")):
        a01, b01 = content(kind, n, h, w, seed=100 * ci + h)
        for sa, sb in KINDS:
            a, b = encode(a01, sa), encode(b01, sb)
            for quantize in (False, True):
                want = M.metrics(a, b, sa, sb, border=border, quantize=quantize, mean=MEAN, std=STD)
                got = metrics.image_metrics(a.to(DEV), b.to(DEV), sr_space=sa, hr_space=sb, border=border,
                                            quantize=quantize, mean=MEAN, std=STD)
                exact = M.mse_u8_exact(a, b, border) if (sa, sb) == ("u8", "u8") else None
                check(got, want, f"{shape} {kind} {sa}/{sb} q={int(quantize)}", exact)


def test_identical_inputs():
    a01, _ = content("smooth", 2, 37, 53, seed=7)
    for space in ("u8", "tanh"):
        a = encode(a01, space).to(DEV)
        m = metrics.image_metrics(a, a.clone(), sr_space=space, hr_space=space)
        assert m.mse.tolist() == [0.0, 0.0] and m.mse_y.tolist() == [0.0, 0.0]
        assert all(math.isinf(v) and v > 0 for v in m.psnr.tolist() + m.psnr_y.tolist())
        assert (m.ssim_y - 1).abs().max().item() <= 1e-12


def test_constant_black_against_white():
    """Both variances must come out as 0, not as a rounding residue that changes the result."""
    a = torch.zeros(1, 3, 43, 75, dtype=torch.uint8)
    b = torch.full((1, 3, 43, 75), 255, dtype=torch.uint8)
    got = metrics.image_metrics(a.to(DEV), b.to(DEV), sr_space="u8", hr_space="u8")
    check(got, M.metrics(a, b, "u8", "u8"), "black / white", M.mse_u8_exact(a, b))
    assert got.mse.item() == 1.0
    a1 = encode(torch.zeros(1, 3, 43, 75, dtype=torch.float64), "tanh")
    check(metrics.image_metrics(a1.to(DEV), b.to(DEV), sr_space="tanh", hr_space="u8"),
          M.metrics(a1, b, "tanh", "u8"), "black (tanh) / white")


def test_two_calls_give_the_same_bits():
    a01, b01 = content("noise", 3, 75, 43, seed=11)
    a, b = encode(a01, "tanh").to(DEV), encode(b01, "norm").to(DEV)
    m1 = metrics.image_metrics(a, b, sr_space="tanh", hr_space="norm")
    m2 = metrics.image_metrics(a, b, sr_space="tanh", hr_space="norm")
    for x, y in zip(m1, m2):
        assert torch.equal(x, y)


def test_evaluator_equals_one_call_on_the_concatenation():
    a01, b01 = content("smooth", 6, 37, 53, seed=13)
    a, b = encode(a01, "tanh").to(DEV), encode(b01, "u8").to(DEV)
    ev = metrics.Evaluator()
    for sl in (slice(0, 1), slice(1, 4), slice(4, 6)):
        ev.update(a[sl], b[sl], sr_space="tanh", hr_space="u8")
    got = ev.result()
    m = metrics.image_metrics(a, b, sr_space="tanh", hr_space="u8")
    assert got["images"] == 6
    for k, v in (("psnr", m.psnr), ("psnr_y", m.psnr_y), ("ssim_y", m.ssim_y)):
        want = v.mean().item()
        assert abs(got[k] - want) <= 1e-12 * abs(want), (k, got[k], want)
    # state / merge: two evaluators added
    e1, e2 = metrics.Evaluator(), metrics.Evaluator()
    e1.update(a[:2], b[:2], sr_space="tanh", hr_space="u8")
    e2.update(a[2:], b[2:], sr_space="tanh", hr_space="u8")
    assert e1.state().dtype == torch.float64 and e1.state().is_cuda
    e1.merge(e2.state())
    assert abs(e1.result()["psnr"] - m.psnr.mean().item()) <= 1e-12 * m.psnr.mean().item()


def test_refusals():
    a = torch.zeros(1, 3, 20, 30, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.IsrError, match="11-pixel SSIM window"):
        metrics.image_metrics(a, a, sr_space="u8", hr_space="u8", border=5)  # hc = 10
    c = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP"):
        metrics.image_metrics(c, c, sr_space="u8", hr_space="u8")
    with pytest.raises(ValueError, match="one shape"):
        metrics.image_metrics(a, torch.zeros(1, 3, 20, 31, dtype=torch.uint8, device=DEV), sr_space="u8", hr_space="u8")


def test_graph_capture():
    """The call is capturable like every other entry point: no allocation or sync inside the library."""
    a01, b01 = content("noise", 2, 51, 52, seed=17)
    a, b = encode(a01, "tanh").to(DEV), encode(b01, "u8").to(DEV)
    want = metrics.image_metrics(a, b, sr_space="tanh", hr_space="u8")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = metrics.image_metrics(a, b, sr_space="tanh", hr_space="u8")
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got.mse, want.mse) and torch.equal(got.ssim_y, want.ssim_y)


@torch.no_grad()
def test_validate_on_the_trained_weights():
    net = models.ResNet(16, 0.2, scaleRate=4)
    net.load_state_dict(checkpoint.load_module_state(WEIGHTS))
    net = net.eval().to(DEV)
    lr, hr = heldout_tiles(2, 32, scale=4)  # LR 32², HR 128², on the CPU
    hr_u8 = (hr * 255.0).round().to(torch.uint8)
    res = trainer.validate(net, [hr_u8], 4, mean=MEAN, std=STD)
    assert res["images"] == 2 and not net.training
    # the oracle's metrics, on the CPU, of the same HIP output (per tile, then the mean over tiles)
    _, lr_dev = data.GPUTransform(4, hr_norm=False, mean=MEAN, std=STD, device=DEV)(hr_u8.to(DEV))
    torch.testing.assert_close(lr_dev.cpu(), lr, rtol=0, atol=1e-5)  # validate's LR is heldout_tiles' LR
    y = net(lr_dev).float().cpu()
    hr1 = hr * 2 - 1
    c = lambda t: t[..., 4:-4, 4:-4]  # noqa: E731
    to01 = lambda t: (t.clamp(-1, 1) + 1) / 2  # noqa: E731
    p = np.mean([R.psnr(c(y[i:i + 1]), c(hr1[i:i + 1])) for i in range(2)])
    py = np.mean([R.psnr_y(to01(y[i:i + 1]), hr[i:i + 1]) for i in range(2)])
    print(f"validate {res}; oracle psnr {p:.5f} psnr_y {py:.5f}")
    assert abs(res["psnr"] - p) <= 1e-4 and abs(res["psnr_y"] - py) <= 1e-4
    assert 0 < res["ssim_y"] <= 1
    lr01 = lr * torch.tensor(STD).view(1, 3, 1, 1) + torch.tensor(MEAN).view(1, 3, 1, 1)
    bic = F.interpolate(lr01, scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 1) * 2 - 1
    p_bic = np.mean([R.psnr(c(bic[i:i + 1]), c(hr1[i:i + 1])) for i in range(2)])
    assert res["psnr"] > p_bic, (res["psnr"], p_bic)
    net.train()
    again = trainer.validate(net, [hr_u8[:1], hr_u8[1:]], 4, mean=MEAN, std=STD)
    assert net.training
    assert abs(again["psnr"] - res["psnr"]) <= 1e-9 and again["images"] == 2


COMMON = ["--resnet", "--synthetic", "--synthetic_kind", "leaves", "--rs_deep", "1", "--shape", "64", "--scale", "2",
          "--batch_size", "2", "--epochs", "2", "--steps", "2", "--save_name", "t"]
# what train.py's --resnet save_checkpoint call writes without validation
RES_KEYS = {"gen_net", "optimizer", "epoch", "mean", "std", "loss", "scaler", "ema", "updates"}


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    import train
    d = tmp_path_factory.mktemp("val")
    train.main(train.parse(COMMON + ["--val_synthetic", "2", "--val_shape", "64", "--work_dir", str(d)]))
    return d


def test_train_cli_with_validation(trained):
    lines = [json.loads(s) for s in (trained / "val_t.jsonl").read_text().splitlines()]
    assert [r["epoch"] for r in lines] == [0, 1]
    for r in lines:
        assert math.isfinite(r["psnr"]) and math.isfinite(r["psnr_y"]) and 0 < r["ssim_y"] <= 1
        assert r["images"] == 2 and r["seconds"] >= 0
    best = checkpoint.load_checkpoint(trained / "res_t_1_0.2.best.pt")
    ck = checkpoint.load_checkpoint(trained / "res_t_1_0.2.pt")
    assert set(ck) == RES_KEYS | {"val"} and set(best) == RES_KEYS | {"val"}
    assert ck["val"] == lines[1]
    assert best["val"]["psnr_y"] == max(r["psnr_y"] for r in lines)


def test_train_cli_without_validation_is_unchanged(tmp_path):
    import train
    train.main(train.parse(COMMON + ["--work_dir", str(tmp_path)]))
    assert not (tmp_path / "val_t.jsonl").exists() and not (tmp_path / "res_t_1_0.2.best.pt").exists()
    assert set(checkpoint.load_checkpoint(tmp_path / "res_t_1_0.2.pt")) == RES_KEYS


def test_train_denoise_refuses_validation(tmp_path):
    import train
    with pytest.raises(ValueError, match="--train_denoise"):
        train.main(train.parse(["--train_denoise", "--synthetic", "--val_synthetic", "2", "--work_dir", str(tmp_path)]))


def test_rs_ref(trained, tmp_path, capsys):
    import rs
    from PIL import Image
    g = torch.Generator().manual_seed(5)
    base = torch.rand(1, 3, 6, 8, generator=g)
    hr = (F.interpolate(base, size=(96, 128), mode="bicubic", align_corners=False).clamp(0, 1) * 255).round()
    lr = F.interpolate(hr, size=(48, 64), mode="bilinear", align_corners=False).round().clamp(0, 255)
    Image.fromarray(hr[0].permute(1, 2, 0).to(torch.uint8).numpy()).save(tmp_path / "hr.png")
    Image.fromarray(lr[0].permute(1, 2, 0).to(torch.uint8).numpy()).save(tmp_path / "lr.png")
    kw = dict(model=str(trained / "res_t_1_0.2.pt"), src=str(tmp_path / "lr.png"), save_dir=str(tmp_path / "out.png"),
              window_size=32, batch_size=2, worker=0, halo=0, add_rate=0.2, mean=MEAN, std=STD,
              ref=str(tmp_path / "hr.png"), ref_border=4)
    capsys.readouterr()
    rs.runer(**kw)
    out_lines = [s for s in capsys.readouterr().out.splitlines() if s.startswith("{")]
    assert len(out_lines) == 1
    rec = json.loads(out_lines[0])
    out = rs.read_image(tmp_path / "out.png")
    want = M.metrics(out[None], rs.read_image(tmp_path / "hr.png")[None], "u8", "u8", border=4, quantize=True)
    assert abs(rec["psnr"] - want["psnr"].item()) <= 1e-6
    assert abs(rec["psnr_y"] - want["psnr_y"].item()) <= 1e-6 and abs(rec["ssim_y"] - want["ssim_y"].item()) <= 1e-6
    # a reference of another size is refused, and the message names both sizes
    Image.fromarray(hr[0, :, :90].permute(1, 2, 0).to(torch.uint8).numpy()).save(tmp_path / "small.png")
    with pytest.raises(ValueError, match=r"128x90.*128x96"):
        rs.runer(**dict(kw, ref=str(tmp_path / "small.png")))
