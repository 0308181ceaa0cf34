#!/usr/bin/env python3
"""Time the PIL-exact LR synthesis (isr_resample_u8, csrc/resample.hip) as the fused training
transform, on the training batch 16 x 3 x 96² and on cfg3's 16 x 3 x 512², at x4 and x2 (GPU).

Per shape and scale, on dead-leaves crops, for each of the six filters: the fused transform (HR
crops -> hr fp32 + lr fp32, one launch) as the bare library entry point on preallocated buffers
and as the data.GPUTransform call (which also allocates its outputs from torch's caching
allocator).  Beside them, in the same process on the same batch: isr_sr_transform, the cv2 path
and the thing to compare against; and the host resize of the batch through Pillow (one thread,
wall clock, no copies counted).  Warm-up, then `--runs` windows of `--iters` calls between two
device events; the median per call in µs.

Bytes: what the transform must move (uint8 crops in, fp32 hr and lr out), over the bare entry
point's time, as GB/s and as a share of the 8 TB/s HBM peak.  A case whose bare time is within
2x of an empty launch's (`empty_launch_us`, a one-element torch kernel timed the same way) is
marked launch_bound: its rate says nothing about the kernel.

The cfg3 training step (tools/bench_train.py, a fresh child process) gives the transform's share
of a step; --no-train-step leaves it out.

    python tools/bench_resample.py --out profiles/resample_bench.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from _timing import host_ms, timed, train_step_ms  # noqa: E402
from image_super_resolution_amd import _lib, data, degrade  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, spec


def pil_resize_ms(x: np.ndarray, size: int, name: str, runs: int) -> float:
    from PIL import Image
    flt = getattr(Image, name.upper())
    ims = [Image.fromarray(np.ascontiguousarray(im.transpose(1, 2, 0))) for im in x]
    return host_ms(lambda: [im.resize((size, size), flt).load() for im in ims], runs)


def case(n: int, t: int, scale: int, iters: int, runs: int, empty_us: float) -> dict:
    dev = torch.device("cuda")
    x = data.leaves_hr_u8(n, t, torch.Generator(device=dev).manual_seed(0), device=dev)
    lt = t // scale
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mean = (ctypes.c_float * 3)(*data.IMAGENET_MEAN)
    std = (ctypes.c_float * 3)(*data.IMAGENET_STD)
    hr = torch.empty((n, 3, t, t), device=dev)
    lr = torch.empty((n, 3, lt, lt), device=dev)
    moved = x.numel() + 4 * hr.numel() + 4 * lr.numel()
    floor_us = 1e6 * moved / HBM_PEAK_BYTES_PER_S

    sd = _lib.IsrSrTransformDesc(x.data_ptr(), hr.data_ptr(), lr.data_ptr(), n, t, scale, 1, mean, std)
    cv2_tf = data.GPUTransform(scale, hr_norm=True, device=dev)
    res = {"shape": [n, 3, t, t], "scale": scale, "iters": iters, "runs": runs, "bytes_moved": moved,
           "hbm_floor_us": round(floor_us, 2),
           "sr_transform_launch_us": timed(lambda: lib.isr_sr_transform(ctypes.byref(sd), stream), iters, runs),
           "sr_transform_call_us": timed(lambda: cv2_tf(x), iters, runs), "filters": {}}
    xh = x.cpu().numpy()
    for name in degrade.RESAMPLE_FILTERS:
        f = degrade.RESAMPLE_FILTERS.index(name)
        bx, cx, ks = degrade._device_tables(dev, t, lt, (f,))
        rd = _lib.IsrResampleDesc(n, t, t, lt, lt, 1, ks, ks, x.data_ptr(), bx.data_ptr(), cx.data_ptr(), bx.data_ptr(),
                                  cx.data_ptr(), None, None, lr.data_ptr(), hr.data_ptr(), 1, mean, std)
        _lib.check(lib.isr_resample_u8(ctypes.byref(rd), stream), "isr_resample_u8")
        tf = data.GPUTransform(scale, hr_norm=True, device=dev, lr_filter=name)
        launch = timed(lambda: lib.isr_resample_u8(ctypes.byref(rd), stream), iters, runs)
        r = {"taps_per_lr_pixel": int(ks) * int(ks), "fused_launch_us": launch,
             "fused_call_us": timed(lambda: tf(x), iters, runs),
             "ratio_to_sr_transform": round(launch / res["sr_transform_launch_us"], 2),
             "gb_per_s": round(moved / launch / 1e3, 1),
             "share_of_hbm_peak": round(floor_us / launch, 3),
             "launch_bound": bool(launch < 2 * empty_us),
             "host_pil_resize_ms": pil_resize_ms(xh, lt, name, min(runs, 5))}
        res["filters"][name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-train-step", action="store_true", help="skip the cfg3 training step (a child process)")
    ap.add_argument("--commit", default=None, help="the commit the numbers were measured on, recorded as given")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_resample.py times the HIP kernels and needs a GPU")
    one = torch.zeros(1, device="cuda")
    empty_us = timed(lambda: one.add_(1.0), args.iters, args.runs)
    res = [case(16, t, s, args.iters, args.runs, empty_us) for t in (96, 512) for s in (4, 2)]
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "hbm_peak_tb_per_s": HBM_PEAK_BYTES_PER_S / 1e12,
           "empty_launch_us": empty_us, "results": res}
    if not args.no_train_step:
        step = train_step_ms()
        cfg3 = next(r for r in res if r["shape"][2] == 512 and r["scale"] == 4)
        doc["cfg3_train_step_ms"] = step
        doc["cfg3_share_of_step"] = {"sr_transform": round(cfg3["sr_transform_call_us"] / 1e3 / step, 5),
                                     **{k: round(v["fused_call_us"] / 1e3 / step, 5)
                                        for k, v in cfg3["filters"].items()}}
    text = json.dumps(doc, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
