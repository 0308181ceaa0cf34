#!/usr/bin/env python3
"""Time the YUV 4:2:0 colour kernels (isr_yuv420_to_rgb_u8 / isr_rgb_to_yuv420_u8, csrc/yuv.hip)
against the torch layout copies they replace in the video path (GPU).

Per case (frame size, batch, layout; left siting, BT.709 limited): the bare library entry points on
preallocated buffers, and beside each, in the same process, the copy of video.FrameUpscaler's
rgb-mode body on the same frame size: the HWC -> CHW permute copy in, the flip + permute copy out.
Five warm-up calls, then `--runs` windows of `--iters` calls between two device events; the median
per call in µs with the windows' min and max.  The batch-1 1080p outputs are first compared with
the numpy restatement (tests/yuv_ref.py) at the timed size.

Bytes: what the call must move (frame bytes + RGB bytes; the copies: RGB bytes in + out) over its
time, as GB/s.  Working sets below the 256 MiB last-level cache are marked `fits_llc`: their rate is
not an HBM rate.  A case within 2x of an empty launch (`empty_launch_us`) is marked launch_bound.

    python tools/bench_yuv.py --out profiles/yuv_bench.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import yuv_ref  # noqa: E402
from image_super_resolution_amd import _lib, yuv  # noqa: E402

LLC_BYTES = 256 << 20
CASES = [(1080, 1920, 1, "i420"), (1080, 1920, 4, "i420"), (2160, 3840, 1, "i420"), (2160, 3840, 4, "i420"),
         (2160, 3840, 1, "nv12"), (2160, 3840, 4, "nv12")]


def windows(fn, iters: int, runs: int, warmup: int = 5) -> dict:
    """µs per call of `fn`: the median of `runs` windows of `iters` calls between device events, and
    the windows' min and max."""
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
    return {"us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def rated(t: dict, moved: int, empty_us: float) -> dict:
    return dict(t, bytes_moved=moved, gb_per_s=round(moved / t["us"] / 1e3, 1), fits_llc=bool(moved < LLC_BYTES),
                launch_bound=bool(t["us"] < 2 * empty_us))


def case(h: int, w: int, n: int, layout: str, iters: int, runs: int, empty_us: float) -> dict:
    dev = torch.device("cuda")
    fmt = yuv.YUVFormat(layout, "bt709", False, "left")
    g = torch.Generator(device=dev).manual_seed(h + n)
    frames = torch.randint(0, 256, (n, 3 * h // 2, w), generator=g, dtype=torch.uint8, device=dev)
    rgb = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8, device=dev)
    rgb_out, frames_out = torch.empty_like(rgb), torch.empty_like(frames)
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_in = yuv._desc(n, h, w, fmt, frames.data_ptr(), rgb_out.data_ptr())
    d_out = yuv._desc(n, h, w, fmt, rgb.data_ptr(), frames_out.data_ptr())
    _lib.check(lib.isr_yuv420_to_rgb_u8(ctypes.byref(d_in), stream), "isr_yuv420_to_rgb_u8")
    _lib.check(lib.isr_rgb_to_yuv420_u8(ctypes.byref(d_out), stream), "isr_rgb_to_yuv420_u8")
    checked = False
    if n == 1 and h <= 1080:
        f = frames.cpu().numpy().reshape(n, -1)
        if not np.array_equal(rgb_out.cpu().numpy(), yuv_ref.yuv420_to_rgb(f, h, w, "bt709", False, "left", layout)):
            raise RuntimeError(f"isr_yuv420_to_rgb_u8 differs from the restatement at {n}x{h}x{w} {layout}")
        if not np.array_equal(frames_out.cpu().numpy().reshape(n, -1),
                              yuv_ref.rgb_to_yuv420(rgb.cpu().numpy(), "bt709", False, "left", layout)):
            raise RuntimeError(f"isr_rgb_to_yuv420_u8 differs from the restatement at {n}x{h}x{w} {layout}")
        checked = True
    moved = frames.numel() + rgb.numel()
    res = {"shape": [n, h, w], "layout": layout, "siting": "left", "matrix": "bt709", "range": "limited",
           "iters": iters, "runs": runs, "checked_against_restatement": checked}
    res["yuv420_to_rgb"] = rated(windows(lambda: lib.isr_yuv420_to_rgb_u8(ctypes.byref(d_in), stream), iters, runs),
                                 moved, empty_us)
    res["rgb_to_yuv420"] = rated(windows(lambda: lib.isr_rgb_to_yuv420_u8(ctypes.byref(d_out), stream), iters, runs),
                                 moved, empty_us)
    # the copies of FrameUpscaler's rgb-mode body on the same frame size
    hwc = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8, device=dev)
    chw, bgr = torch.empty_like(rgb), torch.empty_like(hwc)
    res["torch_hwc_to_chw_copy"] = rated(windows(lambda: chw.copy_(hwc.permute(0, 3, 1, 2)), iters, runs),
                                         2 * rgb.numel(), empty_us)
    res["torch_flip_permute_copy"] = rated(windows(lambda: bgr.copy_(rgb.flip(1).permute(0, 2, 3, 1)), iters, runs),
                                           2 * rgb.numel(), empty_us)
    print(f"[bench_yuv] {n}x{h}x{w} {layout}: in {res['yuv420_to_rgb']['us']} us (copy "
          f"{res['torch_hwc_to_chw_copy']['us']}), out {res['rgb_to_yuv420']['us']} us (copy "
          f"{res['torch_flip_permute_copy']['us']})", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--commit", default=None, help="the commit the numbers were measured on, recorded as given")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_yuv.py times the HIP kernels and needs a GPU")
    one = torch.zeros(1, device="cuda")
    empty_us = windows(lambda: one.add_(1.0), args.iters, args.runs)["us"]
    res = [case(h, w, n, lay, args.iters, args.runs, empty_us) for h, w, n, lay in CASES]
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "empty_launch_us": empty_us,
           "method": f"5 warm-up calls, {args.runs} windows of {args.iters} calls between device events, one process; "
                     "median (min, max) per call", "results": res}
    text = json.dumps(doc, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
