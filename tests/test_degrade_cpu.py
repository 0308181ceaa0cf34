"""Host-side checks of the training-data degradations (no GPU): the numpy restatement of the JPEG
round trip (tests/degrade_ref.py, the reference of tests/test_gpu_degrade.py) against PIL's
libjpeg, the quantisation tables, the C ABI's symbols and struct layouts (its refusals are rows of
tests/test_capi_refusals.py), and NoisyTransform's unchanged default path."""
import ctypes
import io

import numpy as np
import pytest
import torch

import degrade_ref as R
from image_super_resolution_amd import _lib, data, degrade

NEW_SYMBOLS = ("isr_jpeg_roundtrip_workspace_bytes", "isr_jpeg_roundtrip", "isr_hls_l_moments", "isr_iso_noise")


def pil_roundtrip(rgb: np.ndarray, q: int) -> np.ndarray:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb.transpose(1, 2, 0))).save(buf, format="JPEG", quality=q)
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB")).transpose(2, 0, 1)


@pytest.fixture(scope="module")
def crops():
    """Per shape: two dead-leaves crops and two uniform-noise crops."""
    leaves = data.leaves_hr_u8(2, 96, torch.Generator().manual_seed(11), device="cpu").numpy()
    rng = np.random.default_rng(0)
    out = {}
    for h, w in ((16, 16), (32, 48), (96, 96)):
        out[(h, w)] = [leaves[0][:, :h, :w].copy(), leaves[1][:, :h, :w].copy(),
                       rng.integers(0, 256, (3, h, w), dtype=np.uint8),
                       rng.integers(0, 256, (3, h, w), dtype=np.uint8)]
    return out


@pytest.mark.parametrize("shape", [(16, 16), (32, 48), (96, 96)])
def test_restatement_matches_pil(crops, shape):
    """PSNR(restatement, PIL) >= PSNR(PIL, original) + 15 dB at qualities 50, 62, 75: the restatement
    is libjpeg up to its integer 'islow' DCT flipping a few quantised coefficients against a float
    DCT.  Observed minimum gap over these 36 cases: 16.3 dB (32x48 leaves, q = 50; 16.5 dB at 16x16,
    where one flipped coefficient is a large share of 768 values; >= 23.4 dB on every 96x96 case); the restatement in
    fp32 against fp64 differs in 0 pixels on all of them."""
    gaps = []
    for im in crops[shape]:
        for q in (50, 62, 75):
            ref, pil = R.jpeg_roundtrip(im, q), pil_roundtrip(im, q)
            near, far = R.psnr(ref, pil), R.psnr(pil, im)
            gaps.append(near - far)
            assert near >= far + 15.0, (shape, q, near, far)
            assert np.array_equal(ref, R.jpeg_roundtrip(im, q, np.float32))
    print(f"{shape}: minimum PSNR gap {min(gaps):.2f} dB")


def test_quality_zero_is_identity_in_the_restatement(crops):
    im = crops[(16, 16)][0]
    assert np.array_equal(R.jpeg_roundtrip(im, 0), im)


def test_quant_tables():
    assert np.array_equal(R.quant_table(R.LUMA_Q, 50), R.LUMA_Q)
    assert np.array_equal(R.quant_table(R.CHROMA_Q, 50), R.CHROMA_Q)
    assert R.quant_table(R.LUMA_Q, 75)[0, 0] == 8
    assert R.quant_table(R.LUMA_Q, 100).max() == 1 and R.quant_table(R.CHROMA_Q, 1).max() == 255


def test_symbols_exported_and_bound(built_lib):
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(built_lib, name) is not None


def test_struct_layouts_match_c(tmp_path):
    import subprocess
    from conftest import ROOT
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "isr.h"
#define F(s, m) printf(#s "." #m " %zu\n", offsetof(s, m))
int main(void) {
  printf("isr_jpeg_desc %zu\nisr_hls_moments_desc %zu\nisr_iso_noise_desc %zu\n", sizeof(isr_jpeg_desc),
         sizeof(isr_hls_moments_desc), sizeof(isr_iso_noise_desc));
  F(isr_jpeg_desc, src); F(isr_jpeg_desc, quality); F(isr_hls_moments_desc, partials);
  F(isr_iso_noise_desc, hue_noise); F(isr_iso_noise_desc, apply);
  printf("blocks %d\n", ISR_HLS_PARTIAL_BLOCKS);
  return 0;
}
"""
    (tmp_path / "probe.c").write_text(probe)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                   check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True).stdout
    c = dict(line.split() for line in out.splitlines())
    cls = {"isr_jpeg_desc": _lib.IsrJpegDesc, "isr_hls_moments_desc": _lib.IsrHlsMomentsDesc,
           "isr_iso_noise_desc": _lib.IsrIsoNoiseDesc}
    for key, val in c.items():
        if key == "blocks":
            assert int(val) == _lib.HLS_PARTIAL_BLOCKS
        elif "." in key:
            s, m = key.split(".")
            assert getattr(cls[s], m).offset == int(val), key
        else:
            assert ctypes.sizeof(cls[key]) == int(val), key


def test_quality_is_checked_on_the_python_side():
    x = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    for bad in (-1, 101, 62.5):
        with pytest.raises(ValueError, match="0..100"):
            degrade.jpeg_roundtrip(x, bad)
    with pytest.raises(ValueError, match="0..100"):
        degrade.jpeg_roundtrip(x, torch.tensor([101]))
    with pytest.raises(ValueError, match="integer"):
        degrade.jpeg_roundtrip(x, torch.tensor([62.0]))
    with pytest.raises(ValueError, match="quality range"):
        data.NoisyTransform(device="cpu", jpeg_p=0.5, jpeg_quality=(75, 50))


def test_degradations_refuse_cpu_tensors():
    x = torch.zeros(2, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP"):
        degrade.jpeg_roundtrip(x, 60)
    with pytest.raises(RuntimeError, match="HIP"):
        degrade.hls_l_moments(x)
    with pytest.raises(RuntimeError, match="HIP"):
        degrade.iso_noise(x, 0.03, 0.3, None)
    with pytest.raises(RuntimeError, match="HIP"):
        data.NoisyTransform(device="cpu", jpeg_p=0.5)(x)
    with pytest.raises(RuntimeError, match="HIP"):
        data.NoisyTransform.reference(device="cpu")(x)


def old_noisy_formula(crops_u8, seed, device, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, var_limit=(10.0, 50.0),
                      p=0.5):
    """NoisyTransform as it was before the ISO / JPEG stages: three draws, float all the way."""
    g = torch.Generator(device=device).manual_seed(seed)
    m = torch.tensor(mean, device=device).view(1, 3, 1, 1)
    s = torch.tensor(std, device=device).view(1, 3, 1, 1)
    x = crops_u8.to(device).float()
    n = x.shape[0]
    var = torch.empty(n, 1, 1, 1, device=device).uniform_(*var_limit, generator=g)
    apply = (torch.rand(n, 1, 1, 1, device=device, generator=g) < p).float()
    noise = torch.randn(x.shape, device=device, generator=g) * var.sqrt() * apply
    noisy = (x + noise).clamp_(0, 255).div_(255.0)
    return (x / 255.0 * 2.0 - 1.0).contiguous(), ((noisy - m) / s).contiguous(), g


def test_default_noisy_transform_is_unchanged():
    crops = torch.randint(0, 256, (8, 3, 16, 16), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    for seed in (0, 5):
        t = data.NoisyTransform(device="cpu", seed=seed)
        assert t.iso_p == 0 and t.jpeg_p == 0
        hr, lr = t(crops)
        hr0, lr0, g = old_noisy_formula(crops, seed, "cpu")
        assert torch.equal(hr, hr0) and torch.equal(lr, lr0)
        # and the generator stands where it stood: the next draw is the same
        assert torch.equal(torch.rand(4, generator=t.gen), torch.rand(4, generator=g))
    r = data.NoisyTransform.reference(device="cpu")
    assert r.iso_p == 0.5 and r.jpeg_p == 0.5 and r.jpeg_quality == (50, 75)
