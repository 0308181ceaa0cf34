"""The dihedral transforms without a GPU: the group itself (tests/dihedral_ref.py against
isr_dihedral_inverse) and the command-line and constructor ends of both features.  What isr_dihedral,
isr_ensemble_expand_u8 and isr_ensemble_reduce refuse is in tests/test_capi_refusals.py."""
import pytest
import torch

import dihedral_ref as ref
from image_super_resolution_amd import _lib


def test_the_eight_ops_are_different_and_each_has_its_inverse():
    x = torch.arange(3 * 5, dtype=torch.float32).view(1, 1, 3, 5) ** 2  # asymmetric, non-square
    results = [ref.apply_ref(x, k) for k in range(8)]
    for k, y in enumerate(results):
        assert tuple(y.shape[-2:]) == ((5, 3) if k % 2 else (3, 5)), k
        assert torch.equal(ref.apply_ref(y, ref.inverse_ref(k)), x), k
    for a in range(8):
        for b in range(a + 1, 8):
            assert results[a].shape != results[b].shape or not torch.equal(results[a], results[b]), (a, b)
    # the element formulas include/isr.h states, on one op of each kind
    h, w = 3, 5
    p = x[0, 0]
    assert all(results[1][0, 0, i, j] == p[j, w - 1 - i] for i in range(w) for j in range(h))
    assert all(results[4][0, 0, i, j] == p[i, w - 1 - j] for i in range(h) for j in range(w))
    assert all(results[7][0, 0, i, j] == p[h - 1 - j, w - 1 - i] for i in range(w) for j in range(h))


def test_inverse_entry_point(built_lib):
    for k in range(8):
        assert built_lib.isr_dihedral_inverse(k) == ref.inverse_ref(k), k
    for k in (-1, 8):
        assert built_lib.isr_dihedral_inverse(k) < 0, k
        assert b"dihedral_inverse" in built_lib.isr_last_error()
    from image_super_resolution_amd import dihedral
    assert [dihedral.inverse(k) for k in range(8)] == [0, 3, 2, 1, 4, 5, 6, 7]
    with pytest.raises(ValueError):
        dihedral.inverse(8)


def test_python_entry_points_refuse_cpu_tensors():
    from image_super_resolution_amd import dihedral
    u8 = torch.zeros(1, 3, 4, 4, dtype=torch.uint8)
    f32 = torch.zeros(4, 3, 4, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        dihedral.apply(u8, 1)
    with pytest.raises(RuntimeError, match="HIP"):
        dihedral.expand_u8(u8)
    with pytest.raises(RuntimeError, match="HIP"):
        dihedral.reduce(f32, f32)


def test_augment_argument():
    from image_super_resolution_amd import data
    with pytest.raises(ValueError, match="bogus"):
        data.GPUTransform(4, device="cpu", augment="bogus")
    with pytest.raises(ValueError, match="bogus"):
        data.NoisyTransform(device="cpu", augment="bogus")
    # off the GPU: "none" is the transform it always was, anything else has no path
    crops = torch.randint(0, 256, (2, 3, 16, 16), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    hr, lr = data.GPUTransform(4, device="cpu", augment="none")(crops)
    hr0, lr0 = data.GPUTransform(4, device="cpu")(crops)
    assert torch.equal(hr, hr0) and torch.equal(lr, lr0)
    with pytest.raises(RuntimeError, match="HIP"):
        data.GPUTransform(4, device="cpu", augment="flip")(crops)


def test_train_parser_takes_augment():
    import train
    assert train.augment_of(train.parse([])) == "none"
    assert not hasattr(train.parse([]), "augment")  # absent, as --lr_filter is
    assert train.augment_of(train.parse(["--augment", "dihedral"])) == "dihedral"
    assert train.augment_of(train.parse(["--train_denoise", "--augment", "flip"])) == "flip"
    with pytest.raises(SystemExit):
        train.parse(["--augment", "rot45"])


def test_rs_parser_refuses_self_ensemble_for_video(capsys):
    import rs
    assert rs.parse(["--src", "in.png"]).self_ensemble is False
    assert rs.parse(["--src", "in.png", "--self_ensemble"]).self_ensemble is True
    for name in ("clip.mp4", "clip.y4m", "clip.rgb"):
        with pytest.raises(SystemExit):
            rs.parse(["--src", name, "--self_ensemble"])
        assert "--self_ensemble is for stills" in capsys.readouterr().err
    with pytest.raises(ValueError, match="stills"):  # and the function itself, before it touches a device
        rs.runer(src="clip.mp4", save_dir="out.mp4", self_ensemble=True)


def test_tile_upscaler_needs_run_f32():
    from image_super_resolution_amd import tiler
    with pytest.raises(TypeError, match="run_f32"):
        tiler.TileUpscaler(lambda x: x, 2, device="cpu", self_ensemble=True)
    tiler.TileUpscaler(lambda x: x, 2, device="cpu")  # as before
    # the memory helper: more than one plain forward of the 8 copies' worth, growing with the batch
    a, b = tiler.ensemble_forward_bytes(1, 24, 40, 1), tiler.ensemble_forward_bytes(2, 24, 40, 1)
    assert b > a > tiler.forward_bytes(4, 24, 40, 1)
