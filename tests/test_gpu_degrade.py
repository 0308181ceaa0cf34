"""The training-data degradations on the GPU (csrc/degrade.hip, image_super_resolution_amd.degrade)
against their numpy restatements (tests/degrade_ref.py; test_degrade_cpu.py holds the restatement
against PIL's libjpeg), and the reference denoise pipeline they make (NoisyTransform.reference,
`ISR_DENOISE_DEGRADE=reference train.py --train_denoise`)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import degrade_ref as R
from image_super_resolution_amd import data, degrade

ROOT = Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu

JPEG_SHAPES = [(16, 16), (32, 48), (96, 96)]  # one MCU (every edge an image edge); interior MCU borders, not square
QUALITIES = [(50, 0, 75), (62, 75, 100)]

# Share of output values on which the ISO-noise restatement run in fp32 differs from itself run in
# fp64, over iso_cases() below: the truncation-flip rate of the formula (a value within an fp32
# rounding of an integer truncates either way).  Measured on the CPU: 4956 of 30900 values
# (with zero noise the round trip lands within a rounding of the source integer, so a third of those
# values truncate one down in one precision or the other).
ISO_FLIP_SHARE = 4956 / 30900


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def steps_image(h, w):
    """Flat regions and steps that put DC, (0,4), (4,0) and (4,4) on exact quantisation ties: blocks
    of constant grey whose level-shifted DC is an odd multiple of half a quantiser step, 4-pixel
    stripes and 4x4 checkers of amplitudes that do the same for the other three."""
    im = np.empty((3, h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    by, bx = yy // 8, xx // 8
    base = 128 + ((by * 5 + bx * 3) % 9 - 4)              # DC = 8 * (base - 128): ties at q | 16 etc.
    stripe_x = np.where((xx + 1) % 4 < 2, 1, -1)          # the sign pattern of cos((2x + 1) pi / 4)
    stripe_y = np.where((yy + 1) % 4 < 2, 1, -1)
    kind = (by + 2 * bx) % 4
    amp = 1 + (by + bx) % 6
    v = base + np.where(kind == 1, amp * stripe_x, 0) + np.where(kind == 2, amp * stripe_y, 0) + \
        np.where(kind == 3, amp * stripe_x * stripe_y, 0)
    # one pixel + 4 in every other block: all four exact coefficients move by +-1/2, a tie at step 1
    v = v + np.where(((by + bx) % 2 == 0) & (yy % 8 == 3) & (xx % 8 == 5), 4, 0)
    im[0] = im[1] = im[2] = np.clip(v, 0, 255)
    im[2, : h // 2] = np.clip(v[: h // 2] + 16, 0, 255)   # some chroma in the upper half
    return im


@pytest.fixture(scope="module")
def jpeg_inputs():
    """Per shape a batch of 3: two dead-leaves crops and the flat-plus-steps image."""
    leaves = data.leaves_hr_u8(2, 96, torch.Generator().manual_seed(21), device="cpu").numpy()
    return {(h, w): np.stack([leaves[0][:, :h, :w], leaves[1][:, 96 - h:, 96 - w:], steps_image(h, w)])
            for h, w in JPEG_SHAPES}


@pytest.mark.parametrize("shape", JPEG_SHAPES)
@pytest.mark.parametrize("quals", QUALITIES)
def test_jpeg_kernel_matches_restatement(jpeg_inputs, shape, quals):
    """Expected: zero differing pixels (the restatement in fp32 against fp64 gives zero).  The bar:
    at most 0.5 % of values differ at all and PSNR(kernel, restatement) >= 60 dB."""
    x = jpeg_inputs[shape]
    ref = R.jpeg_roundtrip_batch(x, quals)
    q = torch.tensor(quals, dtype=torch.int32, device="cuda")
    out = degrade.jpeg_roundtrip(torch.from_numpy(x).cuda(), q).cpu().numpy()
    differ = int((out != ref).sum())
    print(f"jpeg {shape} q={quals}: {differ} of {ref.size} values differ, PSNR {R.psnr(out, ref):.1f} dB")
    for i, qi in enumerate(quals):
        if qi == 0:
            assert np.array_equal(out[i], x[i])
    assert differ <= 0.005 * ref.size
    assert R.psnr(out, ref) >= 60.0


def test_jpeg_quality_zero_and_batching(jpeg_inputs):
    x = torch.from_numpy(jpeg_inputs[(32, 48)]).cuda()
    assert torch.equal(degrade.jpeg_roundtrip(x, 0), x)
    mixed = degrade.jpeg_roundtrip(x, torch.tensor([70, 0, 55], device="cuda"))
    assert torch.equal(mixed[1], x[1]) and not torch.equal(mixed[0], x[0])
    for i, q in enumerate((70, 0, 55)):
        assert torch.equal(degrade.jpeg_roundtrip(x[i:i + 1], q)[0], mixed[i])
    # the destination of an image does not depend on the batch around it
    big = degrade.jpeg_roundtrip(torch.cat([x, x.flip(0), x]), torch.tensor([55] * 9, device="cuda"))
    small = degrade.jpeg_roundtrip(x, 55)
    assert torch.equal(big[:3], small) and torch.equal(big[6:], small) and torch.equal(big[3:6], small.flip(0))
    with pytest.raises(Exception, match="16"):
        degrade.jpeg_roundtrip(x[:, :, :24], 60)


@pytest.mark.parametrize("shape", [(16, 16), (33, 47)])
def test_hls_l_moments(shape):
    h, w = shape
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (4, 3, h, w), dtype=np.uint8)
    x[1] = 77                                   # flat: std exactly 0
    x[2] = (x[2] // 64) * 64                    # few levels
    x[3, :, : h // 2] = 255                     # bright half
    ref = R.hls_l_moments(x)
    out = degrade.hls_l_moments(torch.from_numpy(x).cuda()).cpu().numpy()
    assert out.shape == (4, 2) and out.dtype == np.float64
    assert out[1, 1] == 0.0 and out[1, 0] == ref[1, 0]
    rel = np.abs(out - ref) / np.maximum(np.abs(ref), 1e-300)
    rel[1, 1] = 0.0
    print(f"hls_l_moments {shape}: max relative error {rel.max():.3e}")
    assert rel.max() <= 1e-12
    assert np.array_equal(out, degrade.hls_l_moments(torch.from_numpy(x).cuda()).cpu().numpy())


def iso_cases():
    """(rgb uint8 [n][3][h][w], lum fp32 [n][h][w], hue fp32 [n][h][w]) at 32x32 (four pixels per
    thread) and 33x47 (one): greys, saturated primaries and secondaries, random pixels, under zero
    noise, hue offsets of +-400 degrees (both wraps), a luminance ramp, and random noise."""
    rng = np.random.default_rng(9)
    cases = []
    for h, w in ((32, 32), (33, 47)):
        im = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        im[:, 0:4] = np.linspace(0, 255, 4 * w).astype(np.uint8).reshape(4, w)  # greys
        prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                         [0, 0, 0], [255, 255, 255]], np.uint8)
        im[:, 4:8] = prim[np.arange(4 * w) % 8].T.reshape(3, 4, w)
        zero = np.zeros((h, w), np.float32)
        hue400 = np.where(np.arange(h * w).reshape(h, w) % 2 == 0, 400.0, -400.0).astype(np.float32)
        ramp = (np.arange(h * w, dtype=np.float32).reshape(h, w) % 97)
        lum_r = rng.poisson(12.0, (h, w)).astype(np.float32)
        hue_r = (rng.standard_normal((h, w)) * 9.0).astype(np.float32)
        rgb = np.stack([im] * 4)
        cases.append((rgb, np.stack([zero, zero, ramp, lum_r]), np.stack([zero, hue400, zero, hue_r])))
    return cases


def test_iso_noise_kernel_matches_restatement():
    """max |diff| <= 1 LSB, and the share of differing values at most 3 x ISO_FLIP_SHARE."""
    differ = total = 0
    for rgb, lum, hue in iso_cases():
        ref = np.stack([R.iso_noise(rgb[i], lum[i], hue[i], np.float32) for i in range(len(rgb))])
        out = degrade.iso_noise_planes(torch.from_numpy(rgb).cuda(), torch.from_numpy(lum).cuda(),
                                       torch.from_numpy(hue).cuda()).cpu().numpy()
        d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
        assert d.max() <= 1, d.max()
        differ += int((d != 0).sum())
        total += d.size
    print(f"iso_noise: {differ} of {total} values differ from the fp32 restatement "
          f"(allowed {3 * ISO_FLIP_SHARE * total:.0f})")
    assert differ <= 3 * ISO_FLIP_SHARE * total


def test_iso_flip_share_is_the_recorded_one():
    """ISO_FLIP_SHARE is the restatement's own fp32-against-fp64 flip rate on iso_cases()."""
    differ = total = 0
    for rgb, lum, hue in iso_cases():
        for i in range(len(rgb)):
            a, b = R.iso_noise(rgb[i], lum[i], hue[i], np.float32), R.iso_noise(rgb[i], lum[i], hue[i], np.float64)
            assert np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 1
            differ += int((a != b).sum())
            total += a.size
    assert abs(differ / total - ISO_FLIP_SHARE) < 1e-9, (differ, total)


def test_iso_apply_zero_copies_through():
    rgb, lum, hue = iso_cases()[0]
    x = torch.from_numpy(rgb).cuda()
    ap = torch.tensor([1, 0, 1, 0], device="cuda")
    out = degrade.iso_noise_planes(x, torch.from_numpy(lum).cuda() + 20, torch.from_numpy(hue).cuda(), ap)
    full = degrade.iso_noise_planes(x, torch.from_numpy(lum).cuda() + 20, torch.from_numpy(hue).cuda())
    assert torch.equal(out[1], x[1]) and torch.equal(out[3], x[3])
    assert torch.equal(out[0], full[0]) and torch.equal(out[2], full[2]) and not torch.equal(full[1], x[1])


def test_iso_noise_end_to_end():
    g = lambda: torch.Generator(device="cuda").manual_seed(17)
    # a flat grey image: std(L) = 0 -> Poisson rate 0 -> no luminance change; grey has S = 0, so the
    # hue noise changes nothing either (255 * (k / 255) truncates back to k for every k)
    flat = torch.full((2, 3, 32, 32), 93, dtype=torch.uint8, device="cuda")
    assert torch.equal(degrade.iso_noise(flat, 0.05, 0.5, g()), flat)
    # a flat coloured image: still no luminance change; only the hue moves, so L = (max + min) / 2 stays
    col = torch.tensor([200, 120, 40], dtype=torch.uint8, device="cuda").view(1, 3, 1, 1).expand(2, 3, 32, 32).contiguous()
    out = degrade.iso_noise(col, 0.05, 0.5, g())
    assert not torch.equal(out, col)
    l_in = degrade.hls_l_moments(col)[:, 0]
    l_out = degrade.hls_l_moments(out)[:, 0]
    assert float((l_out - l_in).abs().max()) <= 1.0 / 255.0  # truncation only
    # a textured image: Poisson counts are >= 0 and scaled into the headroom, so mean L rises
    tex = data.leaves_hr_u8(2, 32, torch.Generator(device="cuda").manual_seed(2), device="cuda")
    a = degrade.iso_noise(tex, 0.03, 0.5, g())
    b = degrade.iso_noise(tex, 0.03, 0.5, g())
    assert torch.equal(a, b) and not torch.equal(a, tex)
    assert bool((degrade.hls_l_moments(a)[:, 0] > degrade.hls_l_moments(tex)[:, 0]).all())
    c = degrade.iso_noise(tex, 0.03, 0.5, torch.Generator(device="cuda").manual_seed(18))
    assert not torch.equal(a, c)


def test_graph_capture(jpeg_inputs):
    """The entry points are capturable: no allocation or synchronisation inside the library, and the
    per-image quality / apply arrays are read on the device at replay."""
    x = torch.from_numpy(jpeg_inputs[(32, 48)]).cuda()
    rgb, lum, hue = iso_cases()[0]
    xi, lum, hue = torch.from_numpy(rgb).cuda(), torch.from_numpy(lum).cuda(), torch.from_numpy(hue).cuda()
    q = torch.tensor([60, 0, 75], dtype=torch.int32, device="cuda")
    want_j, want_i, want_m = degrade.jpeg_roundtrip(x, q), degrade.iso_noise_planes(xi, lum, hue), degrade.hls_l_moments(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got_j, got_i, got_m = degrade.jpeg_roundtrip(x, q), degrade.iso_noise_planes(xi, lum, hue), degrade.hls_l_moments(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_j, want_j) and torch.equal(got_i, want_i) and torch.equal(got_m, want_m)
    q.copy_(torch.tensor([0, 90, 75], dtype=torch.int32, device="cuda"))  # the same graph, other qualities
    want_j = degrade.jpeg_roundtrip(x, q)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_j, want_j) and torch.equal(got_j[0], x[0])


def _denorm255(lr):
    mean = torch.tensor(data.IMAGENET_MEAN, device=lr.device).view(1, 3, 1, 1)
    std = torch.tensor(data.IMAGENET_STD, device=lr.device).view(1, 3, 1, 1)
    return (lr * std + mean) * 255.0


def test_noisy_transform_reference_pipeline():
    crops = data.leaves_hr_u8(64, 32, torch.Generator(device="cuda").manual_seed(4), device="cuda")
    hr, lr = data.NoisyTransform.reference(device="cuda", seed=6)(crops)
    hr2, lr2 = data.NoisyTransform.reference(device="cuda", seed=6)(crops)
    assert torch.equal(hr, hr2) and torch.equal(lr, lr2)
    assert hr.shape == lr.shape == (64, 3, 32, 32)
    px = _denorm255(lr)
    assert float(px.min()) >= -1e-3 and float(px.max()) <= 255 + 1e-3
    assert float((px - px.round()).abs().max()) < 1e-3  # the stages exchange uint8
    # each stage alone (the others off) touches a binomial(64, 0.5) number of images
    for kw in (dict(p=0.0, iso_p=0.5), dict(p=0.0, jpeg_p=0.5), dict(p=0.5)):
        _, one = data.NoisyTransform(device="cuda", seed=8, **kw)(crops)
        touched = int(((_denorm255(one) - crops.float()).abs().flatten(1).amax(1) > 0.5).sum())
        print(f"NoisyTransform {kw}: {touched} of 64 images touched")
        assert 10 <= touched <= 54, (kw, touched)


def test_noisy_transform_default_is_the_old_formula_on_the_gpu():
    from test_degrade_cpu import old_noisy_formula
    crops = torch.randint(0, 256, (8, 3, 32, 32), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    t = data.NoisyTransform(device="cuda", seed=12)
    hr, lr = t(crops)
    hr0, lr0, g = old_noisy_formula(crops, 12, "cuda")
    assert torch.equal(hr, hr0) and torch.equal(lr, lr0)
    assert torch.equal(torch.rand(4, device="cuda", generator=t.gen), torch.rand(4, device="cuda", generator=g))


def test_train_denoise_cli_with_reference_degradations(tmp_path):
    """ISR_DENOISE_DEGRADE=reference train.py --train_denoise, in a fresh child process."""
    env = dict(os.environ, ISR_DENOISE_DEGRADE="reference")
    cmd = [sys.executable, str(ROOT / "train.py"), "--train_denoise", "--synthetic", "--steps", "4", "--batch_size", "2",
           "--shape", "48", "--rs_deep", "2", "--epochs", "1", "--work_dir", str(tmp_path), "--save_name", "d"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("epoch 0: loss")]
    assert line, r.stdout[-2000:]
    assert np.isfinite(float(line[0].split()[-1]))
    assert (tmp_path / "denoise_d_2_0.2.pt").is_file()
