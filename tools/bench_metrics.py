#!/usr/bin/env python3
"""Time isr_image_metrics (metrics.image_metrics) on the shapes the project uses (GPU).

Cases: a training batch, 16 x 3 x 512², as fp32 tanh output against fp32 tanh truth and as uint8
against uint8, and one 3 x 2160 x 3840 uint8 pair (a 4K still).  Per case: warm-up, then `--runs`
windows of `--iters` calls between two device events in one process; the median and the minimum per
call in µs, GB/s of algorithmic bytes (both inputs read once; the 32 bytes written per image are
left out) and that rate as a fraction of the 8 TB/s HBM peak.  The call includes its two launches and
the workspace / output allocation from torch's caching allocator.

For scale only, the same three metrics by torch ops on the same GPU (fp32 F.conv2d with the 11 x 11
window over the five moment planes), timed the same way.  It is not a reference: its fp32 moments
miss the flat-image SSIM by 1e-4.

--val-share also runs `train.py --resnet` (x4, batch 16, 512² leaves crops) for three short epochs
with --val_synthetic 16 and reports the validation pass (the `seconds` field of val_*.jsonl) next
to the time of the epoch's training steps.

    python tools/bench_metrics.py --val-share --out profiles/metrics_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_super_resolution_amd import metrics  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, spec


def timed(fn, iters: int, runs: int, warmup: int = 5) -> list[float]:
    """µs per call of `fn`, one figure per run (device events around `iters` calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    return out


def torch_metrics(a01: torch.Tensor, b01: torch.Tensor, border: int = 4):
    """The same quantities by torch ops in fp32 (for scale)."""
    a, b = a01[..., border:-border, border:-border], b01[..., border:-border, border:-border]
    mse = (a - b).pow(2).flatten(1).mean(1)
    wv = torch.tensor([65.481, 128.553, 24.966], device=a.device).view(1, 3, 1, 1)
    x, y = (a * wv).sum(1, keepdim=True) + 16.0, (b * wv).sum(1, keepdim=True) + 16.0
    mse_y = ((x - y) / 255.0).pow(2).flatten(1).mean(1)
    k = torch.arange(11, dtype=torch.float32, device=a.device) - 5
    g = torch.exp(-(k[:, None] ** 2 + k[None, :] ** 2) / 4.5)
    g = (g / g.sum())[None, None]
    mx, my = F.conv2d(x, g), F.conv2d(y, g)
    vx, vy, cxy = F.conv2d(x * x, g) - mx * mx, F.conv2d(y * y, g) - my * my, F.conv2d(x * y, g) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return mse, mse_y, s.flatten(1).mean(1)


def case(name: str, a: torch.Tensor, b: torch.Tensor, space: str, iters: int, runs: int) -> dict:
    nbytes = a.numel() * a.element_size() + b.numel() * b.element_size()
    t = timed(lambda: metrics.image_metrics(a, b, sr_space=space, hr_space=space), iters, runs)
    to01 = (lambda v: v.float() / 255.0) if space == "u8" else (lambda v: v * 0.5 + 0.5)
    tt = timed(lambda: torch_metrics(to01(a), to01(b)), max(1, iters // 4), runs, warmup=2)
    med = statistics.median(t)
    return {"case": name, "shape": list(a.shape), "dtype": str(a.dtype).replace("torch.", ""), "iters": iters,
            "runs": runs, "us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
            "algorithmic_bytes": nbytes, "gb_per_s": round(nbytes / med / 1e3, 1),
            "fraction_of_8tb_per_s": round(nbytes / (med * 1e-6) / HBM_PEAK, 4),
            "torch_ops_fp32_us_median": round(statistics.median(tt), 2)}


def val_share(steps: int) -> dict:
    import train
    from image_super_resolution_amd import trainer
    epochs = []
    orig = trainer.train

    def timed_train(*a, **k):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = orig(*a, **k)
        e1.record()
        torch.cuda.synchronize()
        epochs.append(e0.elapsed_time(e1) / 1e3)
        return r

    trainer.train = timed_train
    try:
        with tempfile.TemporaryDirectory() as d:
            train.main(train.parse(["--resnet", "--scale", "4", "--synthetic", "--synthetic_kind", "leaves", "--shape",
                                    "512", "--batch_size", "16", "--epochs", "3", "--steps", str(steps), "--val_synthetic",
                                    "16", "--val_shape", "512", "--work_dir", d, "--save_name", "bench"]))
            vals = [json.loads(s) for s in (Path(d) / "val_bench.jsonl").read_text().splitlines()]
    finally:
        trainer.train = orig
    ep, va = epochs[-1], vals[-1]["seconds"]  # the third epoch: plans and code objects are warm
    return {"case": "validation_share", "model": "ResNet(16, 0.2, x4)", "batch": 16, "hr_crop": 512,
            "steps_per_epoch": steps, "epoch_train_seconds": [round(v, 3) for v in epochs],
            "val_seconds": [v["seconds"] for v in vals], "val_images": vals[-1]["images"],
            "share_of_this_epoch": round(va / (ep + va), 4),
            "share_of_a_500_step_epoch": round(va / (ep / steps * 500 + va), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--val-share", action="store_true")
    ap.add_argument("--val-steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON here (train.py prints to stdout too)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_metrics.py times the HIP kernels and needs a GPU")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    res = []
    a = torch.rand(16, 3, 512, 512, generator=g, device=dev) * 2 - 1
    b = (a + 0.05 * torch.randn(a.shape, generator=g, device=dev)).clamp_(-1, 1)
    res.append(case("batch_fp32_tanh", a, b, "tanh", args.iters, args.runs))
    au, bu = ((a + 1) * 127.5).round().to(torch.uint8), ((b + 1) * 127.5).round().to(torch.uint8)
    res.append(case("batch_uint8", au, bu, "u8", args.iters, args.runs))
    s = torch.randint(0, 256, (1, 3, 2160, 3840), generator=g, device=dev, dtype=torch.uint8)
    s2 = (s.int() + torch.randint(-3, 4, s.shape, generator=g, device=dev)).clamp_(0, 255).to(torch.uint8)
    res.append(case("still_4k_uint8", s, s2, "u8", args.iters, args.runs))
    if args.val_share:
        res.append(val_share(args.val_steps))
    text = json.dumps({"device": torch.cuda.get_device_name(0), "results": res}, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
