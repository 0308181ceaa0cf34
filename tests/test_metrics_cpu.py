"""The image metrics without a GPU: the fp64 restatement against the oracle, the C struct layout,
Evaluator.merge across a gloo world, train.py's flags (the refusals: tests/test_capi_refusals.py)."""
import ctypes
import os
import socket
import subprocess

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_ref as M
from conftest import ROOT
from image_super_resolution_amd import _lib
from oracle import ref_cpu as R


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_window_sums_to_one():
    w = M.window()
    assert w.shape == (11, 11) and w.dtype == torch.float64
    assert abs(w.sum().item() - 1.0) <= 1e-15
    assert torch.equal(w, w.t()) and w[5, 5] == w.max()


def test_psnr_y_matches_oracle():
    g = torch.Generator().manual_seed(3)
    # float64 images: the oracle forms the luma in its input's precision, and fp32 lumas alone
    # move a PSNR by 3e-7 dB
    a = torch.rand(2, 3, 40, 52, generator=g, dtype=torch.float64)
    b = torch.rand(2, 3, 40, 52, generator=g, dtype=torch.float64)
    assert abs(M.psnr_y(a, b) - R.psnr_y(a, b)) <= 1e-9
    # the per-image form the kernel reports, pooled the way the oracle pools a batch
    m = M.metrics(a, b, "unit", "unit")
    pooled = -10 * torch.log10(m["mse_y"].mean()).item()
    assert abs(pooled - R.psnr_y(a, b)) <= 1e-9
    # PSNR on [0, 1] with peak 1 is the oracle's peak-2 PSNR of the same images in tanh space
    p = -10 * torch.log10(M.metrics(a, b, "unit", "unit", border=0)["mse"].mean()).item()
    assert abs(p - R.psnr(a * 2 - 1, b * 2 - 1)) <= 1e-9


def test_ssim_of_an_image_with_itself_is_one():
    g = torch.Generator().manual_seed(4)
    a = torch.rand(2, 3, 30, 33, generator=g)
    s = M.metrics(a, a.clone(), "unit", "unit")["ssim_y"]
    assert (s - 1).abs().max().item() <= 1e-12


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "isr.h"
#define F(m) printf(#m " %zu\n", offsetof(isr_metrics_desc, m))
int main(void) {
  printf("sizeof %zu\n", sizeof(isr_metrics_desc));
  F(n); F(h); F(w); F(border); F(a); F(b); F(a_u8); F(b_u8); F(a_scale); F(a_shift); F(b_scale); F(b_shift);
  F(clamp); F(quantize); F(out);
  return 0;
}
"""


def test_metrics_desc_layout_matches_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(c.pop("sizeof")) == ctypes.sizeof(_lib.IsrMetricsDesc)
    assert set(c) == {f[0] for f in _lib.IsrMetricsDesc._fields_}
    for name, off in c.items():
        assert getattr(_lib.IsrMetricsDesc, name).offset == int(off), name


# Per-image values that are small dyadic rationals: every partial sum is exact in fp64, so the
# merged means can be compared with == whatever the order of the additions.
VALUES = torch.tensor([[30.25, 32.5, 0.875], [28.0, 29.75, 0.8125], [31.5, 33.25, 0.9375], [27.125, 28.5, 0.75],
                       [35.0, 36.625, 0.96875]], dtype=torch.float64)


def _batch(rows):
    from image_super_resolution_amd.metrics import Metrics
    v = VALUES[rows]
    return Metrics(v[:, 0], v[:, 1], v[:, 2], torch.zeros(len(v), dtype=torch.float64),
                   torch.zeros(len(v), dtype=torch.float64))


def _merge_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from image_super_resolution_amd.metrics import Evaluator
        ev = Evaluator("cpu")
        for i in range(rank, 5, world):  # images rank::world, one at a time
            ev.add(_batch([i]))
        assert ev.state().dtype == torch.float64 and ev.state().device.type == "cpu"
        ev.all_reduce()
        q.put((rank, ev.result()))
    finally:
        dist.destroy_process_group()


def test_evaluator_merge_over_a_gloo_world():
    from image_super_resolution_amd.metrics import Evaluator
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    single = Evaluator("cpu")
    single.add(_batch([0, 1, 2]))
    single.add(_batch([3, 4]))
    want = single.result()
    assert want["images"] == 5 and want["psnr"] == VALUES[:, 0].sum().item() / 5
    assert res[0] == want and res[1] == want
    # merge(state) is the same addition without a process group
    a, b = Evaluator("cpu"), Evaluator("cpu")
    a.add(_batch([0, 2, 4]))
    b.add(_batch([1, 3]))
    a.merge(b.state())
    assert a.result() == want


OLD_DEFAULTS = dict(resnet=False, scale=2, train_denoise=False, worker=2, batch_size=16, work_dir="./",
                    momentum=0.999, weight_decay=0.0, lr=1e-4, epochs=300, dml=False, mean=False, resume=False,
                    L1_loss=False, rs_deep=16, shape=96, save_name="checkpoint", lr2=0.01, seed=100, add_rate=0.2,
                    enchant=False, tpu=False, synthetic=False, synthetic_kind="smooth", dist_backend="nccl",
                    steps=None, vgg_weights=None, dis_miopen=False)


def test_train_flags(tmp_path, monkeypatch):
    import train
    monkeypatch.chdir(tmp_path)  # no ./train_images.json here: --data keeps its literal default
    got = vars(train.parse([]))
    assert {k: got[k] for k in OLD_DEFAULTS} == OLD_DEFAULTS and got["data"] == ""
    assert set(got) - set(OLD_DEFAULTS) - {"data"} == {"val", "val_synthetic", "val_shape", "val_every"}
    assert (got["val"], got["val_synthetic"], got["val_shape"], got["val_every"]) == ("", 0, 512, 1)
    o = train.parse(["--val", "val_images.json", "--val_synthetic", "3", "--val_shape", "130", "--val_every", "2"])
    assert (o.val, o.val_synthetic, o.val_shape, o.val_every) == ("val_images.json", 3, 130, 2)
    with pytest.raises(SystemExit):
        train.parse(["--val_every", "0"])
