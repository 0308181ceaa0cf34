#!/usr/bin/env python3
"""Time the 10-bit YUV 4:2:0 colour kernels (isr_yuv420_to_rgb_16 / isr_rgb_to_yuv420_16, csrc/yuv16.hip)
in each RGB kind beside the 8-bit kernels (csrc/yuv.hip) on the same frame size, and the video path
(BASELINE configs[4]: 1080p -> 4K, x2 RRDB) with 10-bit frames on both sides against the 8-bit YUV mode,
all in one process (GPU).

Per case (frame size, layout; batch 1, left siting, BT.709 limited): the bare library entry points on
preallocated buffers.  Five warm-up calls, then `--runs` windows of `--iters` calls between two device
events; the median per call in µs with the windows' min and max.  The 1080p outputs are first compared
with the numpy restatement (tests/yuv16_ref.py) at the timed size.

Bytes: what the call must move (frame bytes + RGB bytes of the kind) over its time, as GB/s, and that
rate's share of the 8 TB/s HBM peak.  Working sets below the 256 MiB last-level cache are marked
`fits_llc`: their rate is not an HBM rate.  A case within 2x of an empty launch (`empty_launch_us`) is
marked launch_bound.

The video part replays FrameUpscaler's captured graph (`--video_reps` replays per window) and streams
`--frames` frames through VideoUpscaler into a NullRecorder, the 8-bit and the 10-bit upscaler
alternating window by window.

    python tools/bench_yuv16.py --out profiles/yuv16_bench.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import yuv16_ref  # noqa: E402
from bench_yuv import LLC_BYTES, windows  # noqa: E402
from image_super_resolution_amd import _lib, engine, models, video, yuv  # noqa: E402
from image_super_resolution_amd.weights import synth_state_dict  # noqa: E402

HBM_PEAK_GB_S = 8000.0
CASES = [(1080, 1920, "i420"), (2160, 3840, "i420"), (2160, 3840, "nv12")]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def rated(t: dict, moved: int, empty_us: float) -> dict:
    gbs = moved / t["us"] / 1e3
    return dict(t, bytes_moved=moved, gb_per_s=round(gbs, 1), share_of_hbm_peak=round(gbs / HBM_PEAK_GB_S, 4),
                fits_llc=bool(moved < LLC_BYTES), launch_bound=bool(t["us"] < 2 * empty_us))


def case(h: int, w: int, layout: str, iters: int, runs: int, empty_us: float) -> dict:
    dev = torch.device("cuda")
    n = 1
    fmt = yuv.YUVFormat(layout, "bt709", False, "left", 10)
    fmt8 = yuv.YUVFormat(layout, "bt709", False, "left")
    g = torch.Generator(device=dev).manual_seed(h)
    words = torch.randint(0, 1024, (n, 3 * h // 2, w), generator=g, dtype=torch.int16, device=dev) << fmt.shift
    frames = words.view(torch.uint8).reshape(n, 3 * h // 2, 2 * w)
    rgb = torch.randint(0, 1024, (n, 3, h, w), generator=g, dtype=torch.int16, device=dev)
    tanh = torch.rand((n, 3, h, w), generator=g, device=dev) * 2.2 - 1.1
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"shape": [n, h, w], "layout": layout, "pix_fmt": fmt.pix_fmt, "siting": "left", "matrix": "bt709",
           "range": "limited", "iters": iters, "runs": runs}
    args = ("bt709", False, "left", layout, fmt.shift)
    check = h <= 1080
    res["checked_against_restatement"] = check
    f_np = frames.cpu().numpy().reshape(n, -1) if check else None

    def timed(name, fn, d, moved):
        _lib.check(fn(ctypes.byref(d), stream), name)
        res[name] = rated(windows(lambda: fn(ctypes.byref(d), stream), iters, runs), moved, empty_us)

    # yuv -> rgb, both kinds
    for kind, dtype, size in (("u16", torch.int16, 2), ("norm_f32", torch.float32, 4)):
        out = torch.empty((n, 3, h, w), dtype=dtype, device=dev)
        d = yuv._desc16(n, h, w, fmt, kind, frames.data_ptr(), out.data_ptr(), MEAN, STD)
        timed(f"yuv420_to_rgb_16[{kind}]", lib.isr_yuv420_to_rgb_16, d, frames.numel() + size * rgb.numel())
        if check:
            want = yuv16_ref.yuv420_to_rgb(f_np, h, w, *args)
            if kind == "norm_f32":
                want = yuv16_ref.normalise(want, MEAN, np.array(yuv.inv_std_of(STD), np.float32))
            else:
                want = want.view(np.int16)
            if not np.array_equal(out.cpu().numpy(), want):
                raise RuntimeError(f"isr_yuv420_to_rgb_16 [{kind}] differs from the restatement at {h}x{w} {layout}")
    # rgb -> yuv, both kinds
    for kind, src, size in (("u16", rgb, 2), ("tanh_f32", tanh, 4)):
        out = torch.empty_like(frames)
        d = yuv._desc16(n, h, w, fmt, kind, src.data_ptr(), out.data_ptr())
        timed(f"rgb_to_yuv420_16[{kind}]", lib.isr_rgb_to_yuv420_16, d, frames.numel() + size * rgb.numel())
        if check:
            vals = rgb.cpu().numpy() if kind == "u16" else yuv16_ref.quantise(tanh.cpu().numpy())
            if not np.array_equal(out.cpu().numpy().reshape(n, -1), yuv16_ref.rgb_to_yuv420(vals, *args)):
                raise RuntimeError(f"isr_rgb_to_yuv420_16 [{kind}] differs from the restatement at {h}x{w} {layout}")
    # the 8-bit kernels on the same frame size
    frames8 = torch.randint(0, 256, (n, 3 * h // 2, w), generator=g, dtype=torch.uint8, device=dev)
    rgb8 = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8, device=dev)
    out_rgb8, out_frames8 = torch.empty_like(rgb8), torch.empty_like(frames8)
    moved8 = frames8.numel() + rgb8.numel()
    timed("yuv420_to_rgb_u8", lib.isr_yuv420_to_rgb_u8, yuv._desc(n, h, w, fmt8, frames8.data_ptr(), out_rgb8.data_ptr()), moved8)
    timed("rgb_to_yuv420_u8", lib.isr_rgb_to_yuv420_u8, yuv._desc(n, h, w, fmt8, rgb8.data_ptr(), out_frames8.data_ptr()), moved8)
    for k16, k8 in (("yuv420_to_rgb_16[u16]", "yuv420_to_rgb_u8"), ("yuv420_to_rgb_16[norm_f32]", "yuv420_to_rgb_u8"),
                    ("rgb_to_yuv420_16[u16]", "rgb_to_yuv420_u8"), ("rgb_to_yuv420_16[tanh_f32]", "rgb_to_yuv420_u8")):
        res[k16]["gb_per_s_over_8_bit_kernel"] = round(res[k16]["gb_per_s"] / res[k8]["gb_per_s"], 3)
    print(f"[bench_yuv16] {h}x{w} {fmt.pix_fmt}: " + ", ".join(
        f"{k} {v['us']} us {v['gb_per_s']} GB/s" for k, v in res.items() if isinstance(v, dict)), file=sys.stderr, flush=True)
    return res


def video_part(frames_n: int, reps: int, runs: int, blocks: int, h: int, w: int) -> dict:
    """cfg5 with yuv420p on both sides and with yuv420p10le on both sides: graph-only GPU time per frame and
    end-to-end frames/s, the two upscalers alternating window by window."""
    dev = torch.device("cuda")
    sd = synth_state_dict(models.ResNet(blocks, 0.2, scaleRate=2).state_dict(), seed=0)
    gw = engine.pack_generator({k: v.to(dev) for k, v in sd.items()}, enchant=False, device=dev)
    chw = torch.from_numpy(np.stack(list(video.SyntheticVideo(w, h, 8)))).permute(0, 3, 1, 2).contiguous().to(dev)
    modes = {}
    for pix in ("yuv420p", "yuv420p10le"):
        up = video.FrameUpscaler(gw, h, w, 1, device=dev, pix_fmt_in=pix, pix_fmt_out=pix)
        src = chw if pix == "yuv420p" else (chw.to(torch.int16) << 2)
        frames = list(yuv.rgb_to_yuv420(src, up.yuv_in).cpu().numpy())
        frames = [frames[i % len(frames)] for i in range(frames_n)]
        up(torch.from_numpy(np.stack(frames[:1])))
        pipe = video.VideoUpscaler(up)
        pipe.run(frames[:2], video.NullRecorder())  # warm the pinned path
        torch.cuda.synchronize()
        modes[pix] = dict(up=up, pipe=pipe, frames=frames, gpu_ms=[], fps=[])
    for _ in range(runs):
        for m in modes.values():
            up = m["up"]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(up.stream)
            for _ in range(reps):
                up.run_async()
            e1.record(up.stream)
            torch.cuda.synchronize()
            m["gpu_ms"].append(e0.elapsed_time(e1) / reps)
            t0 = time.perf_counter()
            n = m["pipe"].run(m["frames"], video.NullRecorder())
            torch.cuda.synchronize()
            m["fps"].append(n / (time.perf_counter() - t0))
    out = {"in": f"{w}x{h}", "blocks": blocks, "batch": 1, "frames": frames_n, "graph_replays_per_window": reps,
           "windows": runs, "data": "synthetic frames, synthetic weights, NullRecorder (no encoder)"}
    for pix, m in modes.items():
        out[pix] = {"gpu_ms_per_frame": round(statistics.median(m["gpu_ms"]), 3), "gpu_ms_min": round(min(m["gpu_ms"]), 3),
                    "gpu_ms_max": round(max(m["gpu_ms"]), 3), "fps": round(statistics.median(m["fps"]), 3),
                    "fps_min": round(min(m["fps"]), 3), "fps_max": round(max(m["fps"]), 3),
                    "h2d_bytes_per_frame": int(np.prod(m["up"].in_frame_shape)),
                    "d2h_bytes_per_frame": int(np.prod(m["up"].out_frame_shape))}
    out["fps_10_bit_over_8_bit"] = round(out["yuv420p10le"]["fps"] / out["yuv420p"]["fps"], 4)
    out["gpu_ms_10_bit_over_8_bit"] = round(out["yuv420p10le"]["gpu_ms_per_frame"] / out["yuv420p"]["gpu_ms_per_frame"], 4)
    print(f"[bench_yuv16] cfg5: {json.dumps({k: v for k, v in out.items() if k.startswith(('yuv', 'fps', 'gpu'))})}",
          file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=24, help="frames per end-to-end window of the video part")
    ap.add_argument("--video_reps", type=int, default=5)
    ap.add_argument("--video_runs", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--video_size", default="1920x1080")
    ap.add_argument("--no_video", action="store_true")
    ap.add_argument("--commit", default=None, help="the commit the numbers were measured on, recorded as given")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_yuv16.py times the HIP kernels and needs a GPU")
    one = torch.zeros(1, device="cuda")
    empty_us = windows(lambda: one.add_(1.0), args.iters, args.runs)["us"]
    res = [case(h, w, lay, args.iters, args.runs, empty_us) for h, w, lay in CASES]
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "empty_launch_us": empty_us,
           "hbm_peak_gb_per_s": HBM_PEAK_GB_S,
           "method": f"5 warm-up calls, {args.runs} windows of {args.iters} calls between device events, one process; "
                     "median (min, max) per call; bytes are the algorithm's (frame + RGB of the kind)", "results": res}
    if not args.no_video:
        vw, vh = (int(v) for v in args.video_size.lower().split("x"))
        doc["cfg5"] = video_part(args.frames, args.video_reps, args.video_runs, args.blocks, vh, vw)
    text = json.dumps(doc, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
