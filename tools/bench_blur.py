#!/usr/bin/env python3
"""Time the blur degradations (isr_blur_u8, csrc/blur.hip) and the blind LR chain
(data.LRDegrade) on the training batch 16 x 3 x 96² and on cfg3's 16 x 3 x 512² (GPU).

Per shape, on dead-leaves crops: the bare library entry point on preallocated buffers for k = 3,
5, 7, linear (a rotated anisotropic Gaussian table; every linear kind runs the same loop) and
median, every image of the batch the same case; and one mixed batch as the chain launches it.
Each output is first compared with the numpy restatement (tests/blur_ref.py) at the timed size.
Beside them, in the same process on the same batch: isr_resample_u8 (bicubic x4 to uint8), the
neighbouring kernel; scipy.ndimage's correlate / median_filter of the batch on one host thread
(wall clock, no copies counted); and the `blind` chain (`train.py --lr_degrade blind`) and the
chain with every stage at p = 1, as LRDegrade calls (these allocate their outputs from torch's
caching allocator and include the host draws and the table upload).  Warm-up, then `--runs` windows
of `--iters` calls between two device events; the median per call in µs.

Bytes: what a blur must move (uint8 in, uint8 out) over the bare entry point's time, as GB/s and
as a share of the 8 TB/s HBM peak.  A case whose bare time is within 2x of an empty launch's
(`empty_launch_us`, a one-element torch kernel timed the same way) is marked launch_bound: its
rate says nothing about the kernel.

The cfg3 training step (tools/bench_train.py, a fresh child process) gives the chain's share of a
step; --no-train-step leaves it out.

    python tools/bench_blur.py --out profiles/blur_bench.json
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
sys.path.insert(0, str(ROOT / "tests"))
import blur_ref  # noqa: E402
from _timing import host_ms, timed, train_step_ms  # noqa: E402
from image_super_resolution_amd import _lib, data, degrade  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, spec
GAUSS = dict(sigma_x=3.0, sigma_y=0.6, angle=0.7)


def case(n: int, t: int, iters: int, runs: int, empty_us: float, host_runs: int) -> dict:
    from scipy import ndimage
    dev = torch.device("cuda")
    x = data.leaves_hr_u8(n, t, torch.Generator(device=dev).manual_seed(0), device=dev)
    xh = x.cpu().numpy()
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty_like(x)
    moved = 2 * x.numel()
    floor_us = 1e6 * moved / HBM_PEAK_BYTES_PER_S
    res = {"shape": [n, 3, t, t], "iters": iters, "runs": runs, "bytes_moved": moved, "hbm_floor_us": round(floor_us, 3),
           "blur": {}}

    def launch(ks, med, tables):
        """A timed bare launch of per-image (ksize, median, table) on device arrays; checked first."""
        kd = torch.tensor(ks, dtype=torch.int32, device=dev)
        md = torch.tensor(med, dtype=torch.int32, device=dev)
        td = torch.from_numpy(np.ascontiguousarray(tables.reshape(n, 49))).to(dev)
        d = _lib.IsrBlurDesc(n, t, t, x.data_ptr(), out.data_ptr(), kd.data_ptr(), md.data_ptr(), td.data_ptr())
        _lib.check(lib.isr_blur_u8(ctypes.byref(d), stream), "isr_blur_u8")
        if not np.array_equal(out.cpu().numpy(), blur_ref.blur_u8(xh, ks, med, tables)):
            raise RuntimeError(f"isr_blur_u8 differs from the restatement at {n}x3x{t}x{t}, ksize {ks[0]}, median {med[0]}")
        us = timed(lambda: lib.isr_blur_u8(ctypes.byref(d), stream), iters, runs)
        print(f"[bench_blur] {n}x3x{t}x{t} ksize {ks[0]} median {med[0]}: {us} us", file=sys.stderr, flush=True)
        return {"launch_us": us, "gb_per_s": round(moved / us / 1e3, 1), "share_of_hbm_peak": round(floor_us / us, 4),
                "launch_bound": bool(us < 2 * empty_us)}

    for k in (3, 5, 7):
        table = blur_ref.taps("gaussian", k, **GAUSS)
        w = blur_ref.normalized("gaussian", k, **GAUSS)
        lin = launch([k] * n, [0] * n, np.stack([table] * n))
        lin["host_scipy_correlate_ms"] = host_ms(
            lambda: [ndimage.correlate(p.astype(np.float64), w, mode="mirror") for im in xh for p in im], host_runs)
        med = launch([k] * n, [1] * n, np.zeros((n, 7, 7), dtype=np.int32))
        med["host_scipy_median_filter_ms"] = host_ms(
            lambda: [ndimage.median_filter(p, size=k, mode="nearest") for im in xh for p in im], host_runs)
        res["blur"][f"linear_k{k}"] = lin
        res["blur"][f"median_k{k}"] = med
    # the mix a chain launch sees: every kind and k, and copy-through images
    kinds = [("box", 3), ("gaussian", 5), ("motion", 7), ("median", 3), ("median", 5), ("median", 7), ("copy", 0),
             ("gaussian", 7)]
    mot = dict(x1=1, y1=6, x2=5, y2=0)
    ks = [kinds[i % 8][1] for i in range(n)]
    med = [int(kinds[i % 8][0] == "median") for i in range(n)]
    tabs = np.stack([np.zeros((7, 7), dtype=np.int32) if kinds[i % 8][0] in ("median", "copy") else
                     blur_ref.taps(kinds[i % 8][0], ks[i], **(GAUSS if kinds[i % 8][0] == "gaussian" else
                                                              mot if kinds[i % 8][0] == "motion" else {}))
                     for i in range(n)])
    res["blur"]["mixed"] = launch(ks, med, tabs)

    f = degrade.RESAMPLE_FILTERS.index("bicubic")
    lt = t // 4
    bx, cx, kk = degrade._device_tables(dev, t, lt, (f,))
    dst = torch.empty((n, 3, lt, lt), dtype=torch.uint8, device=dev)
    mean = (ctypes.c_float * 3)(*data.IMAGENET_MEAN)
    std = (ctypes.c_float * 3)(*data.IMAGENET_STD)
    rd = _lib.IsrResampleDesc(n, t, t, lt, lt, 1, kk, kk, x.data_ptr(), bx.data_ptr(), cx.data_ptr(), bx.data_ptr(),
                              cx.data_ptr(), None, dst.data_ptr(), None, None, 0, mean, std)
    _lib.check(lib.isr_resample_u8(ctypes.byref(rd), stream), "isr_resample_u8")
    res["resample_bicubic_x4_u8_launch_us"] = timed(lambda: lib.isr_resample_u8(ctypes.byref(rd), stream), iters, runs)

    chain_iters = max(iters // 10, 10)
    blind = data.LRDegrade.preset("blind", seed=1, device=dev)
    blur = data.LRDegrade.preset("blur", seed=1, device=dev)
    every = data.LRDegrade(iso_p=1.0, jpeg_p=1.0, blur_p=1.0, gauss_p=1.0, seed=1, device=dev)
    plain = data.GPUTransform(4, hr_norm=True, device=dev)
    with_blind = data.GPUTransform(4, hr_norm=True, device=dev, degrade=data.LRDegrade.preset("blind", seed=2, device=dev))
    res["chain"] = {"iters": chain_iters,
                    "blind_call_us": timed(lambda: blind(x), chain_iters, runs),
                    "blur_preset_call_us": timed(lambda: blur(x), chain_iters, runs),
                    "every_stage_p1_call_us": timed(lambda: every(x), chain_iters, runs),
                    "transform_cv2_x4_call_us": timed(lambda: plain(x), chain_iters, runs),
                    "transform_cv2_x4_blind_call_us": timed(lambda: with_blind(x), chain_iters, runs)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--no-train-step", action="store_true", help="skip the cfg3 training step (a child process)")
    ap.add_argument("--commit", default=None, help="the commit the numbers were measured on, recorded as given")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_blur.py times the HIP kernels and needs a GPU")
    torch.set_num_threads(1)
    one = torch.zeros(1, device="cuda")
    empty_us = timed(lambda: one.add_(1.0), args.iters, args.runs)
    res = [case(16, t, args.iters, args.runs, empty_us, args.host_runs) for t in (96, 512)]
    doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "hbm_peak_tb_per_s": HBM_PEAK_BYTES_PER_S / 1e12,
           "empty_launch_us": empty_us, "results": res}
    if not args.no_train_step:
        step = train_step_ms()
        cfg3 = next(r for r in res if r["shape"][2] == 512)["chain"]
        doc["cfg3_train_step_ms"] = step
        doc["cfg3_share_of_step"] = {
            "blind_chain": round(cfg3["blind_call_us"] / 1e3 / step, 5),
            "every_stage_p1": round(cfg3["every_stage_p1_call_us"] / 1e3 / step, 5),
            "transform_cv2_x4": round(cfg3["transform_cv2_x4_call_us"] / 1e3 / step, 5),
            "transform_cv2_x4_blind": round(cfg3["transform_cv2_x4_blind_call_us"] / 1e3 / step, 5)}
    text = json.dumps(doc, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
