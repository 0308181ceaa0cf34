#!/usr/bin/env python3
"""Time the dihedral kernels (csrc/dihedral.hip) and measure what the x8 geometric self-ensemble buys and
costs on the committed trained weights (one MI355X).

(a) Kernel times: isr_dihedral for k = 1 (a quarter turn: the transposing path) and k = 4 (a mirror) on
    16 x 3 x 512² uint8; isr_ensemble_expand_u8 on 8 x 3 x 128² and isr_ensemble_reduce on the matching x4
    member outputs (2 x [32, 3, 512, 512] fp32 -> uint8).  Bare entry points on preallocated buffers; beside
    each, the same result made with torch ops in the same process (flip / rot90 / contiguous; eight slices
    taken back, added and quantised), first compared for equality.  Warm-up, then `--runs` windows of
    `--iters` calls between two device events; the median per call in µs.  Bytes: what the kernel must move
    once (read + written) over its time, as GB/s and as a share of the 8 TB/s HBM peak; a time within 2x of an
    empty launch's is marked launch_bound (its rate says nothing about the kernel).
(b) Quality: tests/golden/trained_resnet_x4.safetensors on the 16 held-out dead-leaves tiles of bench.py
    (weights.heldout_tiles): PSNR and PSNR-Y against HR (metrics.image_metrics on the uint8 outputs, 4-pixel
    border) of the plain uint8 forward and of the ensemble, and the difference.
(c) Cost: one ensembled batch of 8 tiles (expand, two fp32 forwards of 32 images, reduce) against the plain
    forward of the 8 tiles, and the share of the ensembled batch spent in expand + reduce.

    python tools/bench_ensemble.py --out profiles/ensemble_bench.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from _timing import timed  # noqa: E402
from image_super_resolution_amd import _lib, checkpoint, dihedral, engine, metrics, tiler  # noqa: E402
from image_super_resolution_amd.weights import IMAGENET_MEAN, IMAGENET_STD, heldout_tiles  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, spec
DEV = torch.device("cuda")


def rate(us: float, moved: int, empty_us: float) -> dict:
    return {"launch_us": us, "bytes_moved": moved, "gb_per_s": round(moved / us / 1e3, 1),
            "share_of_hbm_peak": round(1e6 * moved / HBM_PEAK_BYTES_PER_S / us, 4), "launch_bound": bool(us < 2 * empty_us)}


def torch_members_back(even, odd):
    """The eight member outputs in the order k = 0..7, each taken back with torch ops (device)."""
    n = even.shape[0] // 4
    out = []
    for k in range(8):
        m = (odd if k % 2 else even)[(k // 2) * n:(k // 2 + 1) * n]
        j = (4 - k) % 4 if k < 4 else k
        out.append(torch.rot90(m.flip(-1) if j >= 4 else m, j % 4, dims=(-2, -1)))
    return out


def torch_reduce_u8(even, odd):
    ms = torch_members_back(even, odd)
    s = ms[0]
    for m in ms[1:]:
        s = s + m
    return torch.round((s * 0.125 + 1) / 2 * 255).clamp_(0, 255).to(torch.uint8)


def kernels(iters: int, runs: int, empty_us: float) -> dict:
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=DEV).manual_seed(0)
    res = {}
    x = torch.randint(0, 256, (16, 3, 512, 512), dtype=torch.uint8, device=DEV, generator=g)
    y = torch.empty_like(x)
    for k, name, via_torch in ((1, "dihedral_k1_rot90", lambda: torch.rot90(x, 1, dims=(-2, -1)).contiguous()),
                               (4, "dihedral_k4_flip", lambda: x.flip(-1))):
        d = _lib.IsrDihedralDesc(16, 3, 512, 512, 1, k, None, x.data_ptr(), y.data_ptr())
        _lib.check(lib.isr_dihedral(ctypes.byref(d), stream), "isr_dihedral")
        if not torch.equal(y, via_torch()):
            raise RuntimeError(f"isr_dihedral op {k} differs from torch")
        r = rate(timed(lambda: lib.isr_dihedral(ctypes.byref(d), stream), iters, runs), 2 * x.numel(), empty_us)
        r["torch_us"] = timed(via_torch, iters, runs)
        res[name] = {"shape": [16, 3, 512, 512], **r}
        print(f"[bench_ensemble] {name}: {r}", file=sys.stderr, flush=True)

    t = torch.randint(0, 256, (8, 3, 128, 128), dtype=torch.uint8, device=DEV, generator=g)
    even = torch.empty((32, 3, 128, 128), dtype=torch.uint8, device=DEV)
    odd = torch.empty_like(even)
    d = _lib.IsrEnsembleExpandDesc(8, 128, 128, t.data_ptr(), even.data_ptr(), odd.data_ptr())

    def torch_expand():
        mem = [torch.rot90(t.flip(-1) if k >= 4 else t, k % 4, dims=(-2, -1)) for k in range(8)]
        return torch.cat(mem[0::2]), torch.cat(mem[1::2])
    _lib.check(lib.isr_ensemble_expand_u8(ctypes.byref(d), stream), "isr_ensemble_expand_u8")
    te, to = torch_expand()
    if not (torch.equal(even, te) and torch.equal(odd, to)):
        raise RuntimeError("isr_ensemble_expand_u8 differs from torch")
    r = rate(timed(lambda: lib.isr_ensemble_expand_u8(ctypes.byref(d), stream), iters, runs), 9 * t.numel(), empty_us)
    r["torch_us"] = timed(torch_expand, iters, runs)
    res["expand_u8"] = {"shape": [8, 3, 128, 128], **r}
    print(f"[bench_ensemble] expand: {r}", file=sys.stderr, flush=True)

    fe = torch.rand((32, 3, 512, 512), device=DEV, generator=g) * 2 - 1
    fo = torch.rand((32, 3, 512, 512), device=DEV, generator=g) * 2 - 1
    out = torch.empty((8, 3, 512, 512), dtype=torch.uint8, device=DEV)
    d = _lib.IsrEnsembleReduceDesc(8, 512, 512, fe.data_ptr(), fo.data_ptr(), out.data_ptr(), 1)
    _lib.check(lib.isr_ensemble_reduce(ctypes.byref(d), stream), "isr_ensemble_reduce")
    if not torch.equal(out, torch_reduce_u8(fe, fo)):
        raise RuntimeError("isr_ensemble_reduce differs from torch")
    r = rate(timed(lambda: lib.isr_ensemble_reduce(ctypes.byref(d), stream), iters, runs),
             4 * (fe.numel() + fo.numel()) + out.numel(), empty_us)
    r["torch_us"] = timed(lambda: torch_reduce_u8(fe, fo), max(iters // 10, 5), runs)
    res["reduce_to_u8"] = {"shape_out": [8, 3, 512, 512], **r}
    print(f"[bench_ensemble] reduce: {r}", file=sys.stderr, flush=True)
    return res


def quality_and_cost(res_kernels: dict, runs: int) -> tuple[dict, dict]:
    sd = checkpoint.load_module_state(ROOT / "tests" / "golden" / "trained_resnet_x4.safetensors")
    gw = engine.pack_generator({k: v.to(DEV) for k, v in sd.items()}, enchant=False, device=DEV)
    runner = tiler.GeneratorRunner(gw, IMAGENET_MEAN, IMAGENET_STD, DEV)
    _, hr = heldout_tiles(16, 128, 4)
    hr_u8 = (hr * 255.0).round().to(torch.uint8).to(DEV)
    lr = torch.nn.functional.interpolate(hr_u8.float(), size=(128, 128), mode="bilinear", align_corners=False)
    lr_u8 = (lr + 0.5).floor_().to(torch.uint8)  # train.py's LR: cv2 INTER_LINEAR of the uint8 crop, rounded half up

    def ensembled(x):
        even, odd = dihedral.expand_u8(x)
        return dihedral.reduce(runner.run_f32(even), runner.run_f32(odd), out_u8=True)

    plain = torch.cat([runner(lr_u8[i:i + 8]) for i in (0, 8)])
    ens = torch.cat([ensembled(lr_u8[i:i + 8]) for i in (0, 8)])
    runner.verify()

    def psnr(sr):
        m = metrics.image_metrics(sr, hr_u8, sr_space="u8", hr_space="u8", border=4, quantize=True)
        return float(m.psnr.mean()), float(m.psnr_y.mean()), float(m.ssim_y.mean())
    p, e = psnr(plain), psnr(ens)
    quality = {"weights": "tests/golden/trained_resnet_x4.safetensors", "tiles": 16, "lr": [128, 128], "scale": 4,
               "plain": {"psnr": round(p[0], 4), "psnr_y": round(p[1], 4), "ssim_y": round(p[2], 5)},
               "ensemble": {"psnr": round(e[0], 4), "psnr_y": round(e[1], 4), "ssim_y": round(e[2], 5)},
               "gain_db": {"psnr": round(e[0] - p[0], 4), "psnr_y": round(e[1] - p[1], 4)},
               "bytes_changed_share": round(float((plain != ens).float().mean()), 4)}
    x8 = lr_u8[:8].contiguous()
    plain_us = timed(lambda: runner(x8), 5, runs, warmup=2)
    ens_us = timed(lambda: ensembled(x8), 3, runs, warmup=2)
    runner.verify()
    glue_us = res_kernels["expand_u8"]["launch_us"] + res_kernels["reduce_to_u8"]["launch_us"]
    cost = {"batch": [8, 3, 128, 128], "plain_forward_us": plain_us, "ensembled_batch_us": ens_us,
            "ensemble_over_plain": round(ens_us / plain_us, 2), "expand_plus_reduce_us": round(glue_us, 2),
            "expand_plus_reduce_share": round(glue_us / ens_us, 5)}
    return quality, cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--commit", default=None, help="the commit the numbers were measured on, recorded as given")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_ensemble.py times the HIP kernels and needs a GPU")
    one = torch.zeros(1, device=DEV)
    empty_us = timed(lambda: one.add_(1.0), args.iters, args.runs)
    res = kernels(args.iters, args.runs, empty_us)
    quality, cost = quality_and_cost(res, args.runs)
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "hbm_peak_tb_per_s": HBM_PEAK_BYTES_PER_S / 1e12,
           "empty_launch_us": empty_us, "iters": args.iters, "runs": args.runs, "kernels": res, "quality": quality,
           "cost": cost}
    text = json.dumps(doc, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
