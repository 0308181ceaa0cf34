"""isr_blur_u8 on the GPU (csrc/blur.hip; degrade.filter_u8 / median_u8 / blur_u8, data.LRDegrade,
GPUTransform's `degrade`, train.py --lr_degrade), pinned bit for bit to tests/blur_ref.py, the numpy
restatement that tests/test_blur_cpu.py holds against scipy and Pillow.  The shapes are the smallest
that reach every branch of the kernel: the smallest image (every border folds back inside one 32 x 32
tile), ragged tiles, one tile plus a pixel on both axes, two tiles on both axes with each w % 4 (the
byte stores; the dword loads that start off a dword), and 96 x 96 (the dword stores)."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import blur_ref as B
import resample_ref as R
from image_super_resolution_amd import data, degrade

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DEV = "cuda"
MEAN, STD = data.IMAGENET_MEAN, data.IMAGENET_STD
SHAPES = [(2, (7, 7)), (3, (9, 13)), (2, (33, 33)), (2, (40, 61)), (2, (33, 62)), (2, (64, 63)), (3, (96, 96))]
LINEAR = {"box": {3: {}, 5: {}, 7: {}},
          "gaussian": {3: dict(sigma_x=0.8, sigma_y=0.8), 5: dict(sigma_x=2.0, sigma_y=0.5, angle=0.4),
                       7: dict(sigma_x=3.0, sigma_y=0.6, angle=0.7)},
          "motion": {3: dict(x1=0, y1=0, x2=2, y2=1), 5: dict(x1=4, y1=0, x2=0, y2=3), 7: dict(x1=1, y1=6, x2=5, y2=0)}}
SHARPEN = np.zeros((7, 7), dtype=np.int32)  # 5 at the centre, -1 on its four neighbours: sum |tap| = 9 * 2^16
SHARPEN[3, 3] = 5 << 16
SHARPEN[2, 3] = SHARPEN[4, 3] = SHARPEN[3, 2] = SHARPEN[3, 4] = -(1 << 16)


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def dev(x):
    return torch.from_numpy(x).to(DEV)


def batch(n, h, w, seed=0):
    """uint8 [n, 3, h, w], test_gpu_resample.py's patterns: noise, then a 0/255 binary image, then
    step edges (the clip's cases)."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    x = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    if n > 1:
        x[1] = rng.integers(0, 2, (3, h, w)) * 255
    if n > 2:
        x[2] = 0
        x[2, 0, :, w // 2:] = 255
        x[2, 1, h // 2:, :] = 255
        x[2, 2, h // 3:, w // 3:] = 255
    return x


@pytest.mark.parametrize("kind", sorted(LINEAR))
def test_linear_bitwise_against_the_restatement(kind):
    for n, (h, w) in SHAPES:
        x = batch(n, h, w)
        xd = dev(x)
        for k, kw in LINEAR[kind].items():
            table = B.taps(kind, k, **kw)
            assert np.array_equal(degrade.blur_taps(kind, k, **kw), table)
            got = degrade.filter_u8(xd, table, k)
            assert got.dtype == torch.uint8 and got.shape == xd.shape
            bad = int((got.cpu().numpy() != B.filter_u8(x, table, k)).sum())
            assert bad == 0, f"{kind} k={k} {h}x{w}: {bad} values differ"
            # the whole 7 x 7 window (ksize left at its default) reads the zero taps too: same pixels
            assert torch.equal(degrade.filter_u8(xd, table), got), f"{kind} k={k} {h}x{w}: ksize 7 differs"


@pytest.mark.parametrize("k", [3, 5, 7])
def test_median_bitwise_against_the_restatement(k):
    for n, (h, w) in SHAPES:
        x = batch(n, h, w, seed=k)
        bad = int((degrade.median_u8(dev(x), k).cpu().numpy() != B.median_u8(x, k)).sum())
        assert bad == 0, f"median k={k} {h}x{w}: {bad} values differ"


def test_negative_taps_reach_both_clip_branches():
    for _, (h, w) in SHAPES:
        x = batch(3, h, w, seed=2)  # image 2: the step edges
        sums = B.filter_sums(x, SHARPEN, 3)
        assert sums.min() < 0 and sums.max() > 255 << 16
        for k in (3, 7):
            got = degrade.filter_u8(dev(x), SHARPEN, k).cpu().numpy()
            assert np.array_equal(got, B.filter_u8(x, SHARPEN, 3)), f"sharpen k={k} {h}x{w}"


def test_mixed_batch():
    cases = [("box", 3), ("gaussian", 5), ("motion", 7), ("median", 3), ("median", 7), ("median", 0), ("box", 9),
             ("motion", -1)]
    n, h, w = len(cases), 40, 50
    x = batch(n, h, w, seed=4)
    x[1], x[2] = batch(3, h, w, seed=5)[0], batch(3, h, w, seed=6)[0]  # noise where the linear kinds run
    xd = dev(x)
    ks = [k for _, k in cases]
    med = [int(kind == "median") for kind, _ in cases]
    tables = np.stack([np.zeros((7, 7), dtype=np.int32) if kind == "median" else
                       B.taps(kind, k if k in (3, 5, 7) else 7, **LINEAR[kind][k if k in (3, 5, 7) else 7])
                       for kind, k in cases])
    want = B.blur_u8(x, ks, med, tables)
    for i in (5, 6, 7):
        assert np.array_equal(want[i], x[i])
    forms = [(ks, med, tables), (torch.tensor(ks), torch.tensor(med), torch.from_numpy(tables)),
             (torch.tensor(ks, dtype=torch.int32, device=DEV), torch.tensor(med, device=DEV), dev(tables)),
             (np.array(ks), tuple(med), dev(tables).long())]
    for kf, mf, tf in forms:
        got = degrade.blur_u8(xd, kf, mf, tf)
        assert np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got[5:], xd[5:])  # copy-through: ksize 0, 9 and -1
    for i in range(n):  # every image equals its single-image launch
        single = degrade.blur_u8(xd[i:i + 1], ks[i], med[i], tables[i])
        assert np.array_equal(single.cpu().numpy()[0], want[i]), cases[i]
    assert torch.equal(degrade.median_u8(xd, 0), xd)
    assert np.array_equal(degrade.median_u8(xd, torch.tensor([3, 0, 5, 0, 7, 0, 9, 3])).cpu().numpy(),
                          B.blur_u8(x, [3, 0, 5, 0, 7, 0, 9, 3], [1] * n, tables))
    for bad in (lambda: degrade.blur_u8(xd, ks[:3], med, tables), lambda: degrade.blur_u8(xd, 3, 0, tables[:2]),
                lambda: degrade.blur_u8(xd, 3, 0, tables.astype(np.float32)), lambda: degrade.filter_u8(xd.float(), tables),
                lambda: degrade.blur_u8(xd, torch.tensor(ks).float(), med, tables)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(Exception, match="smaller than"):
        degrade.median_u8(xd[..., :6, :], 3)


def chain(seed, **kw):
    kw = dict(dict(iso_p=0.5, jpeg_p=0.5, blur_p=0.5, gauss_p=0.5), **kw)
    return data.LRDegrade(seed=seed, device=DEV, **kw)


@pytest.mark.parametrize("lr_filter", ["cv2", "bicubic"])
def test_chain_keeps_hr_and_is_reproducible(lr_filter):
    for scale in (2, 4):
        x = batch(8, 48, 48, seed=scale)
        x[1], x[2] = batch(3, 48, 48, seed=20)[0], batch(3, 48, 48, seed=21)[0]
        xd = dev(x)
        keep = xd.clone()
        plain_hr, plain_lr = data.GPUTransform(scale, device=DEV, lr_filter=lr_filter)(xd)
        hr, lr = data.GPUTransform(scale, device=DEV, lr_filter=lr_filter, degrade=chain(3))(xd)
        hr2, lr2 = data.GPUTransform(scale, device=DEV, lr_filter=lr_filter, degrade=chain(3))(xd)
        assert torch.equal(xd, keep), "the crops were written to"
        assert torch.equal(hr, hr2) and torch.equal(lr, lr2), f"{lr_filter} x{scale}: not reproducible"
        assert torch.equal(hr, plain_hr), f"{lr_filter} x{scale}: hr is not the clean crops'"
        assert lr.shape == plain_lr.shape and not torch.equal(lr, plain_lr) and bool(torch.isfinite(lr).all())
        _, lr3 = data.GPUTransform(scale, device=DEV, lr_filter=lr_filter, degrade=chain(4))(xd)
        assert not torch.equal(lr, lr3), "another seed gives the same degradation"
        off = chain(3, iso_p=0.0, jpeg_p=0.0, blur_p=0.0, gauss_p=0.0)
        hr0, lr0 = data.GPUTransform(scale, device=DEV, lr_filter=lr_filter, degrade=off)(xd)
        assert torch.equal(hr0, plain_hr) and torch.equal(lr0, plain_lr), f"{lr_filter} x{scale}: p = 0 changes lr"


def test_random_filter_draws_are_undisturbed():
    x = batch(16, 48, 48, seed=9)
    x[1], x[2] = batch(3, 48, 48, seed=10)[0], batch(3, 48, 48, seed=11)[0]
    xd = dev(x)
    plain = data.GPUTransform(4, device=DEV, lr_filter="random", seed=7)
    off = data.GPUTransform(4, device=DEV, lr_filter="random", seed=7,
                            degrade=chain(1, iso_p=0.0, jpeg_p=0.0, blur_p=0.0, gauss_p=0.0))
    on = data.GPUTransform(4, device=DEV, lr_filter="random", seed=7, degrade=chain(1))
    for _ in range(2):  # the second call continues the streams
        hr, lr = plain(xd)
        hr0, lr0 = off(xd)
        hr1, lr1 = on(xd)
        assert torch.equal(hr, hr0) and torch.equal(lr, lr0) and torch.equal(hr, hr1)
        assert not torch.equal(lr, lr1)


def test_box_chain_equals_restatement_then_resize():
    for k in (3, 7):
        for scale, name in ((4, "bicubic"), (2, "box")):
            x = batch(3, 48, 48, seed=k)
            deg = data.LRDegrade(blur_p=1.0, blur_kinds=("box",), blur_ksizes=(k,), seed=5, device=DEV)
            hr, lr = data.GPUTransform(scale, device=DEV, lr_filter=name, degrade=deg)(dev(x))
            blurred = B.filter_u8(x, B.taps("box", k), k)
            ref = R.normalize(R.resize(blurred, (48 // scale, 48 // scale), name), MEAN, STD)
            np.testing.assert_allclose(lr.cpu().numpy(), ref, rtol=0, atol=2e-6)
            assert np.array_equal(deg(dev(x)).cpu().numpy(), blurred)


def test_host_draws_follow_the_documented_order():
    seed, n, p = 12, 32, 0.6
    x = batch(n, 24, 40, seed=3)
    x[1], x[2] = batch(3, 24, 40, seed=30)[0], batch(3, 24, 40, seed=31)[0]
    xd = dev(x)
    deg = data.LRDegrade(blur_p=p, seed=seed, device=DEV)
    gen = torch.Generator().manual_seed(seed)
    kinds = set()
    for _ in range(2):  # the second call continues the generator's stream
        got = deg(xd).cpu().numpy()
        # the documented draws, spelled out
        a = torch.rand(n, generator=gen, dtype=torch.float64).tolist()
        b = torch.randint(0, 4, (n,), generator=gen).tolist()
        c = torch.randint(0, 3, (n,), generator=gen).tolist()
        g = torch.rand(n, 3, generator=gen, dtype=torch.float64).tolist()
        m = torch.rand(n, 4, generator=gen, dtype=torch.float64).tolist()
        for i in range(n):
            k, kind = (3, 5, 7)[c[i]], data.LRDegrade.BLUR_KINDS[b[i]]
            want = x[i]
            if a[i] < p:
                kinds.add(kind)
                if kind == "median":
                    want = B.median_u8(x[i], k)
                else:
                    kw = {}
                    if kind == "gaussian":
                        kw = dict(sigma_x=0.2 + 2.8 * g[i][0], sigma_y=0.2 + 2.8 * g[i][1], angle=math.pi * g[i][2])
                    elif kind == "motion":
                        x1, x2, y1 = (int(k * v) for v in m[i][:3])
                        y2 = int(k * m[i][3]) if x1 != x2 else (y1 + 1 + int((k - 1) * m[i][3])) % k
                        kw = dict(x1=x1, y1=y1, x2=x2, y2=y2)
                    try:
                        want = B.filter_u8(x[i], B.taps(kind, k, **kw), k)
                    except ValueError:  # the six-pixel line that misses the centre: left unblurred
                        assert kind == "motion" and k == 7
            assert np.array_equal(got[i], want), (i, kind, k, a[i] < p)
    assert kinds == set(data.LRDegrade.BLUR_KINDS)


def _train(tmp_path, *extra, timeout=240):
    cmd = [sys.executable, str(ROOT / "train.py"), "--resnet", "--scale", "4", "--synthetic", "--steps", "2", "--epochs",
           "1", "--shape", "96", "--work_dir", str(tmp_path), "--save_name", "t", *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=str(tmp_path))


def _loss(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [line.rsplit(" ", 1)[1] for line in r.stdout.splitlines() if line.startswith("epoch 0: loss")]
    assert len(losses) == 1 and math.isfinite(float(losses[0])), r.stdout[-2000:]
    return losses[0]


def test_train_cli_lr_degrade(tmp_path):
    """train.py --lr_degrade blind in a child process of its own trains to a finite loss and is refused
    together with --train_denoise; a run without the flag still prints the same loss as itself."""
    _loss(_train(tmp_path, "--lr_degrade", "blind"))
    r = _train(tmp_path, "--lr_degrade", "blind", "--train_denoise", timeout=120)
    assert r.returncode == 2 and "--lr_degrade" in r.stderr and "--train_denoise" in r.stderr, r.stderr[-2000:]
    assert _loss(_train(tmp_path)) == _loss(_train(tmp_path))
