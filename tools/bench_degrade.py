#!/usr/bin/env python3
"""Time the training-data degradations (image_super_resolution_amd.degrade, csrc/degrade.hip) on
the denoise training batch, 16 x 3 x 96², and on 16 x 3 x 512² (GPU).

Per shape, on dead-leaves crops: the JPEG round trip at per-image qualities 50..75 and the ISO
noise, each as the Python call (kernels, the noise draws of torch.poisson / torch.randn for the ISO
noise, and the output / workspace allocations from torch's caching allocator) and as the bare
library entry points on preallocated buffers; NoisyTransform with GaussNoise only and as the
reference's three-stage pipeline.  Warm-up, then `--runs` windows of `--iters` calls between two
device events in one process; the median per call in µs.

Beside them: the host JPEG round trip of the same batch through PIL (encode + decode of every image,
one thread, wall clock, the device-to-host and host-to-device copies left out), and one denoise
training step of tools/bench_denoise.py at the same batch (a fresh child process).

    python tools/bench_degrade.py --out profiles/degrade_bench.json
"""
from __future__ import annotations

import argparse
import ctypes
import functools
import io
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import _timing  # noqa: E402
from image_super_resolution_amd import _lib, data, degrade  # noqa: E402

timed = functools.partial(_timing.timed, warmup=5)


def pil_roundtrip_ms(x: np.ndarray, q: np.ndarray, runs: int) -> float:
    from PIL import Image
    hwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))

    def roundtrip():
        for im, qi in zip(hwc, q):
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, format="JPEG", quality=int(qi))
            buf.seek(0)
            np.asarray(Image.open(buf).convert("RGB"))
    return _timing.host_ms(roundtrip, runs)


def train_step_ms(batch: int, size: int) -> float:
    return _timing.train_step_ms("bench_denoise.py", ("--batch", "1", "--size", "96", "--train-batch", str(batch),
                                                      "--train-size", str(size)), "train_step_ms", timeout=600)


def case(n: int, t: int, iters: int, runs: int) -> dict:
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    x = data.leaves_hr_u8(n, t, g, device=dev)
    q = torch.randint(50, 76, (n,), generator=g, device=dev, dtype=torch.int32)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    out = torch.empty_like(x)
    jd = _lib.IsrJpegDesc(n, t, t, x.data_ptr(), out.data_ptr(), q.data_ptr())
    nb = lib.isr_jpeg_roundtrip_workspace_bytes(ctypes.byref(jd))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    lum = torch.poisson(torch.full((n, t, t), 8.0, device=dev), generator=g)
    hue = torch.randn((n, t, t), device=dev, generator=g) * 5.0
    on = torch.ones(n, dtype=torch.int32, device=dev)
    mom = torch.empty((n, 2), dtype=torch.float64, device=dev)
    part = torch.empty((n, _lib.HLS_PARTIAL_BLOCKS, 2), dtype=torch.int64, device=dev)
    md = _lib.IsrHlsMomentsDesc(n, t, t, x.data_ptr(), mom.data_ptr(), part.data_ptr())
    nd = _lib.IsrIsoNoiseDesc(n, t, t, x.data_ptr(), out.data_ptr(), lum.data_ptr(), hue.data_ptr(), on.data_ptr())

    def raw_iso():
        lib.isr_hls_l_moments(ctypes.byref(md), stream)
        lib.isr_iso_noise(ctypes.byref(nd), stream)

    gauss = data.NoisyTransform(device=dev, seed=1)
    ref = data.NoisyTransform.reference(device=dev, seed=1)
    px = n * t * t
    res = {"shape": [n, 3, t, t], "iters": iters, "runs": runs,
           "jpeg_roundtrip_call_us": timed(lambda: degrade.jpeg_roundtrip(x, q), iters, runs),
           "jpeg_roundtrip_launches_us": timed(lambda: lib.isr_jpeg_roundtrip(ctypes.byref(jd), ws.data_ptr(), nb, stream),
                                               iters, runs),
           "iso_noise_call_us": timed(lambda: degrade.iso_noise(x, 0.03, 0.3, g), iters, runs),
           "iso_noise_launches_us": timed(raw_iso, iters, runs),
           "noisy_transform_gauss_us": timed(lambda: gauss(x), iters, runs),
           "noisy_transform_reference_us": timed(lambda: ref(x), iters, runs)}
    res["jpeg_launches_mpix_per_s"] = round(px / res["jpeg_roundtrip_launches_us"], 1)
    res["host_pil_roundtrip_ms"] = pil_roundtrip_ms(x.cpu().numpy(), q.cpu().numpy(), min(runs, 5))
    res["denoise_train_step_ms"] = train_step_ms(n, t)
    res["reference_transform_share_of_step"] = round(res["noisy_transform_reference_us"] / 1e3 /
                                                     res["denoise_train_step_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_degrade.py times the HIP kernels and needs a GPU")
    res = [case(16, 96, args.iters, args.runs), case(16, 512, args.iters, args.runs)]
    text = json.dumps({"device": torch.cuda.get_device_name(0), "results": res}, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
