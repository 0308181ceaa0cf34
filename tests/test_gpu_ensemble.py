"""The x8 geometric self-ensemble of tiler.TileUpscaler on the GPU, bit for bit against a restatement that
builds the member batches with tests/dihedral_ref.py, calls the same run_f32 on them, averages with reduce_ref
and stitches with the tiler's own tile list.  Batch composition is the same on both sides, so nothing here
claims that a forward is independent of its batch: only the expand / reduce kernels and the tiler's
bookkeeping are under test."""
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

import dihedral_ref as ref
from conftest import ROOT
from image_super_resolution_amd import models, tiler
from image_super_resolution_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


class RampRunner:
    """A 'network' of torch ops that commutes with no flip and no rotation: nearest x2 of x / 127.5 - 1 plus a
    ramp along the width and a different one along the height, clamped to the tanh range."""
    scale = 2

    def __init__(self):
        self.batches = []

    def run_f32(self, x: torch.Tensor) -> torch.Tensor:
        self.batches.append(x.shape[0])
        y = torch.nn.functional.interpolate(x.float() / 127.5 - 1, scale_factor=2, mode="nearest")
        h, w = y.shape[-2:]
        y = y + torch.arange(w, device=x.device).view(1, 1, 1, w) * 0.004 \
              - torch.arange(h, device=x.device).view(1, 1, h, 1) * 0.0015
        return y.clamp(-1, 1).contiguous()

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return torch.round((self.run_f32(x) + 1) / 2 * 255).clamp(0, 255).to(torch.uint8)


def restated_canvas(image: torch.Tensor, run_f32, scale: int, window: int, halo: int, batch: int) -> torch.Tensor:
    """The ensembled canvas of a uint8 [3, H, W] CPU image, made as the module docstring says."""
    s = scale
    tiles = tiler.plan_tiles(image.shape[1], image.shape[2], window, halo)
    groups = defaultdict(list)
    for t in tiles:
        groups[t.in_shape].append(t)
    canvas = torch.zeros((3, image.shape[1] * s, image.shape[2] * s), dtype=torch.uint8)
    for lst in groups.values():
        for i in range(0, len(lst), batch):
            chunk = lst[i:i + batch]
            x = torch.stack([image[:, t.y0:t.y1, t.x0:t.x1] for t in chunk])
            even, odd = ref.expand_ref(x)
            y = ref.reduce_ref(run_f32(even.to(DEV)).cpu(), run_f32(odd.to(DEV)).cpu())
            for j, t in enumerate(chunk):
                oy, ox = (t.y - t.y0) * s, (t.x - t.x0) * s
                canvas[:, t.y * s:(t.y + t.h) * s, t.x * s:(t.x + t.w) * s] = y[j, :, oy:oy + t.h * s, ox:ox + t.w * s]
    return canvas


def _image(h, w, seed):
    return torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_plumbing_with_a_non_equivariant_runner():
    image = _image(37, 53, 0)  # window 16, halo 3: ragged, non-square tiles
    runner = RampRunner()
    up = tiler.TileUpscaler(runner, 2, window=16, halo=3, batch=4, device=DEV, self_ensemble=True)
    canvas = up(image).cpu()
    want = restated_canvas(image, RampRunner().run_f32, 2, 16, 3, 4)
    assert torch.equal(canvas, want), f"{(canvas != want).sum().item()} of {want.numel()} bytes differ"
    # the runner is not equivariant: the plain canvas is another picture, so the equality above says something
    plain = tiler.TileUpscaler(RampRunner(), 2, window=16, halo=3, batch=4, device=DEV)(image).cpu()
    assert not torch.equal(plain, canvas)
    assert all(b % 4 == 0 for b in runner.batches)  # every forward was a 4 x group batch


def test_a_runner_without_run_f32_is_refused():
    with pytest.raises(TypeError, match="run_f32"):
        tiler.TileUpscaler(lambda x: x, 2, device=DEV, self_ensemble=True)


def test_memory_rule_cuts_the_group():
    image = _image(37, 53, 1)
    kw = dict(window=16, halo=3, batch=2, device=DEV, self_ensemble=True)
    roomy, tight = RampRunner(), RampRunner()
    a = tiler.TileUpscaler(roomy, 2, mem_budget=1 << 40, **kw)(image)
    # just below what two of the largest tiles need together: every group runs tile by tile
    small = min(tiler.ensemble_forward_bytes(2, *t.in_shape, 1) for t in tiler.plan_tiles(37, 53, 16, 3))
    b = tiler.TileUpscaler(tight, 2, mem_budget=small - 1, **kw)(image)
    assert max(roomy.batches) == 8 and set(tight.batches) == {4}
    assert torch.equal(a, b)


@pytest.fixture(scope="module")
def checkpoint_file(tmp_path_factory):
    net = models.ResNet(1, 0.2, scaleRate=2)
    path = tmp_path_factory.mktemp("ensemble") / "gen.pt"
    torch.save(synth_state_dict(net.state_dict(), seed=3), path)
    return path


@pytest.fixture(scope="module")
def runner(checkpoint_file):
    import rs
    return tiler.runner_for(rs.build_model(str(checkpoint_file), 0.2, MEAN, STD), DEV)


def test_the_real_generator(runner):
    image = _image(40, 56, 2)
    kw = dict(window=24, halo=4, batch=2, device=DEV)
    first = runner(image[None, :, :24, :24].to(DEV).contiguous()).clone()  # a uint8 plan, before any fp32 one
    canvas = tiler.TileUpscaler(runner, 2, self_ensemble=True, **kw)(image).cpu()
    want = restated_canvas(image, runner.run_f32, 2, 24, 4, 2)
    assert torch.equal(canvas, want), f"{(canvas != want).sum().item()} of {want.numel()} bytes differ"
    assert any(len(k) == 4 and k[3] == "f32" for k in runner.plans) and (1, 24, 24) in runner.plans
    # the uint8 plans still serve plain calls with the same bits
    assert torch.equal(runner(image[None, :, :24, :24].to(DEV).contiguous()), first)
    # off means off: the canvas of an upscaler built without the argument
    off = tiler.TileUpscaler(runner, 2, self_ensemble=False, **kw)(image)
    assert torch.equal(off, tiler.TileUpscaler(runner, 2, **kw)(image))
    assert not torch.equal(off.cpu(), canvas)


def test_rs_self_ensemble_end_to_end(runner, checkpoint_file, tmp_path):
    from PIL import Image
    image = _image(40, 56, 4)
    Image.fromarray(image.permute(1, 2, 0).numpy()).save(tmp_path / "in.png")
    cmd = [sys.executable, str(ROOT / "rs.py"), "--model", str(checkpoint_file), "--src", str(tmp_path / "in.png"),
           "--save_dir", str(tmp_path / "out.png"), "--window_size", "24", "--halo", "4", "--batch_size", "2",
           "--self_ensemble"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = torch.from_numpy(np.asarray(Image.open(tmp_path / "out.png")).copy()).permute(2, 0, 1)
    canvas = tiler.TileUpscaler(runner, 2, window=24, halo=4, batch=2, device=DEV, self_ensemble=True)(image).cpu()
    assert torch.equal(out, canvas)
    plain = tiler.TileUpscaler(runner, 2, window=24, halo=4, batch=2, device=DEV)(image).cpu()
    assert not torch.equal(out, plain)
