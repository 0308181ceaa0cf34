#!/usr/bin/env python3
"""Video super-resolution throughput (BASELINE configs[4]): 1080p → 4K with the
x2 RRDB generator (ResNet(16, 0.2, scaleRate=2), synthetic weights), uint8 frames
through video.VideoUpscaler (pinned staging, HIP-graph forward, writer thread)
into a NullRecorder.  Prints one JSON line: end-to-end fps and the graph-only
per-batch GPU time.  `--pix_fmt yuv420p|nv12` stages 8-bit 4:2:0 frames on both sides (the colour
kernels of csrc/yuv.hip inside the graph) instead of rgb24 in / bgr24 out; `--windows N` times the
end-to-end run N times and reports the median with the windows' min and max.

python tools/bench_video.py [--frames 24] [--batch 1] [--height 1080 --width 1920] [--pix_fmt yuv420p]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_super_resolution_amd import engine, models, video  # noqa: E402
from image_super_resolution_amd.weights import synth_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--pix_fmt", choices=("rgb24", "yuv420p", "nv12"), default="rgb24")
    ap.add_argument("--windows", type=int, default=1, help="end-to-end runs timed (median, min and max reported)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    sd = synth_state_dict(models.ResNet(args.blocks, 0.2, scaleRate=2).state_dict(), seed=0)
    gw = engine.pack_generator({k: v.to(dev) for k, v in sd.items()}, enchant=False, device=dev)
    yuv_mode = args.pix_fmt != "rgb24"
    fmts = dict(pix_fmt_in=args.pix_fmt, pix_fmt_out=args.pix_fmt) if yuv_mode else {}
    up = video.FrameUpscaler(gw, args.height, args.width, args.batch, device=dev, graph=not args.no_graph, **fmts)
    src = list(video.SyntheticVideo(args.width, args.height, min(args.frames, 8)))
    if yuv_mode:  # the same pictures as 4:2:0 frames of the upscaler's input format
        from image_super_resolution_amd import yuv
        chw = torch.from_numpy(np.stack(src)).permute(0, 3, 1, 2).contiguous().to(dev)
        src = list(yuv.rgb_to_yuv420(chw, up.yuv_in).cpu().numpy())
    frames = [src[i % len(src)] for i in range(args.frames)]
    # graph-only GPU time per batch
    up(torch.from_numpy(np.stack(frames[:args.batch])))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5
    e0.record(up.stream)
    for _ in range(reps):
        up.run_async()
    e1.record(up.stream)
    torch.cuda.synchronize()
    gpu_ms = e0.elapsed_time(e1) / reps
    # the persistent trunk kernel alone (its launch replayed on the plan's stream): its share of
    # the per-batch GPU time, and the batch's trunk FLOPs per second
    import ctypes

    from image_super_resolution_amd import ops
    plan = up.plan.subs[0] if hasattr(up.plan, "subs") else up.plan
    chain = getattr(plan, "chain", None)
    trunk_ms = None
    if chain is not None:
        with torch.cuda.stream(up.stream):
            sp = ops._stream()
            t0e, t1e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0e.record(up.stream)
            for _ in range(reps):
                chain.fn(ctypes.byref(chain.desc), sp)
            t1e.record(up.stream)
        torch.cuda.synchronize()
        trunk_ms = t0e.elapsed_time(t1e) / reps
        assert not chain.failed()
    frame_flops = engine.generator_flops(args.height, args.width, args.blocks, 1)
    # end to end
    pipe = video.VideoUpscaler(up)
    rec = video.NullRecorder()
    pipe.run(frames[:2 * args.batch], rec)  # warm the pinned path
    torch.cuda.synchronize()
    fps = []
    for _ in range(max(1, args.windows)):
        t0 = time.perf_counter()
        n = pipe.run(frames, rec)
        torch.cuda.synchronize()
        fps.append(n / (time.perf_counter() - t0))
    fps.sort()
    dt = n / fps[len(fps) // 2]
    H, W = up.out_hw
    print(json.dumps({"metric": "video SR frames/s (1080p -> 4K, x2 RRDB)", "value": round(n / dt, 3),
                      "unit": "frames/s", "windows": len(fps), "fps_min": round(fps[0], 3), "fps_max": round(fps[-1], 3),
                      "pix_fmt_in": up.pix_fmt_in, "pix_fmt_out": up.pix_fmt_out,
                      "h2d_bytes_per_frame": int(np.prod(up.in_frame_shape)),
                      "d2h_bytes_per_frame": int(np.prod(up.out_frame_shape)),
                      "frames": n, "batch": args.batch, "in": f"{args.width}x{args.height}",
                      "out": f"{W}x{H}", "graph": not args.no_graph,
                      "gpu_ms_per_batch": round(gpu_ms, 3), "gpu_fps": round(args.batch * 1e3 / gpu_ms, 3),
                      "trunk": "persistent trunk kernel" if chain is not None else "per-conv launches",
                      "trunk_ms_per_batch": None if trunk_ms is None else round(trunk_ms, 3),
                      "trunk_share": None if trunk_ms is None else round(trunk_ms / gpu_ms, 4),
                      "model_tflops_per_s": round(frame_flops * args.batch / gpu_ms / 1e9, 1),
                      "tflop_per_frame": round(frame_flops / 1e12, 2),
                      "out_mpix_s": round(n * H * W / dt / 1e6, 1),
                      "data": "synthetic frames, synthetic weights, NullRecorder (no encoder)"}))


if __name__ == "__main__":
    main()
