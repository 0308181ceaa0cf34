#!/usr/bin/env python3
"""Drop-in for the reference's rs.py image branch (rs.py:118-124 CLI,
rs.py:78-114 tiling loop): upscale one still with the HIP generator.

    python rs.py --model res_checkpoint_16_0.2.pt --src in.png --save_dir out.png \
                 --window_size 512 --batch_size 8 [--halo 32]

Multi-GPU: launch with torch.distributed.run; tiles are
dealt across ranks and rank 0 writes the image.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 rs.py ...

`--ref HR.png` (image branch) compares the written uint8 still with a ground-truth image of the
same size on the device and prints one JSON line (psnr, psnr_y, ssim_y; `--ref_border` pixels
cropped from every side, default 4; metrics.image_metrics).

`--self_ensemble` (image branch) runs every tile as its eight flipped and rotated copies, takes each
fp32 output back and averages them before the only rounding to 8 bits (the "+" of EDSR+; 8 x the forward's
cost, tiler.TileUpscaler(self_ensemble=True)); `--ref` then measures the ensembled still.  A video source
refuses the flag.

`--model` takes a checkpoint written by this package's train.py (state_dicts,
loaded with weights_only=True) or a state_dict / .safetensors file; the
reference's TorchScript export is not executed.
Video (rs.py:54-76, BASELINE cfg5): container formats are decoded / encoded by
the ffmpeg binary through raw pipes (as the reference does); headerless rgb24
input (.rgb, with --video_size WxH) and bgr24 output (.bgr / .raw save_dir) work
without ffmpeg.  The per-batch forward is a captured HIP graph (video.py).

    python rs.py --model ck.pt --src clip.mp4 --save_dir out.mp4 --batch_size 2

8-bit YUV 4:2:0 frames (half the bytes of rgb24, converted on the GPU inside the graph): a .y4m
(YUV4MPEG2), .yuv / .i420 (headerless I420) or .nv12 source is read as such, a .y4m / .yuv / .nv12
save_dir is written as such, both without ffmpeg; for container formats `--pix_fmt yuv420p|nv12`
selects what is piped from and to ffmpeg.  `--yuv_matrix`, `--yuv_range`, `--yuv_siting` override
what a .y4m header says (default: limited range, left siting, BT.709 at a height of 720 or more
and BT.601 below, for the input and the output frame each).

    python rs.py --model ck.pt --src clip.y4m --save_dir out.y4m

10-bit 4:2:0 (what HEVC Main10 and AV1 decoders hand over): a C420p10 .y4m is read as such; `--pix_fmt
yuv420p10le|p010le` pipes 10-bit frames from and to ffmpeg and says that a raw .yuv / .i420 / .nv12
source holds 16-bit words.  The output has the input's depth unless `--out_depth 8|10` says otherwise
(an 8-bit source written at 10 bits keeps what the network computes below the 8-bit step).  A 10-bit
side is converted straight to the network's fp32 input and straight from its fp32 output.

    python rs.py --model ck.pt --src clip.mkv --save_dir out.mp4 --pix_fmt yuv420p10le
    python rs.py --model ck.pt --src clip8.y4m --save_dir out10.y4m --out_depth 10
"""
from __future__ import annotations

import argparse
import json
import os
import time
from pathlib import Path

import numpy as np
import torch

from image_super_resolution_amd import checkpoint, models, tiler, video

VID_FORMATS = video.VID_FORMATS
RAW_FORMATS = video.RGB_FORMATS
YUV_FORMATS = video.YUV_FORMATS
YUV_OUT = {".y4m": "yuv420p", ".yuv": "yuv420p", ".nv12": "nv12"}  # save_dir suffix -> pix_fmt (at 8 bits)


def read_image(path: Path) -> torch.Tensor:
    """uint8 [3,H,W] RGB (torchvision.io.read_image(..., ImageReadMode.RGB))."""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"))
    return torch.from_numpy(arr.copy()).permute(2, 0, 1).contiguous()


def write_png(img: torch.Tensor, path: Path) -> None:
    from PIL import Image
    Image.fromarray(img.permute(1, 2, 0).contiguous().cpu().numpy()).save(path.as_posix(), format="PNG")


def build_model(path: str, add_rate: float, mean, std) -> models.Model:
    sd = checkpoint.load_module_state(path, ("ema", "gen_net"))
    gen = checkpoint.generator_from_state(sd, add_rate)
    m = models.Model(gen)
    m.init_normalize(mean, std)
    return m.fuse().eval()


def read_ref(ref_path: Path, out_hw) -> torch.Tensor:
    """The --ref image, refused before any work when it is not the size the output will have."""
    ref = read_image(ref_path)
    if tuple(ref.shape[1:]) != tuple(out_hw):
        raise ValueError(f"--ref {ref_path}: the reference is {ref.shape[2]}x{ref.shape[1]} but the output will be "
                         f"{out_hw[1]}x{out_hw[0]} (width x height)")
    return ref


def compare_with_ref(out: torch.Tensor, ref: torch.Tensor, ref_path: Path, border: int, device) -> dict:
    """--ref: PSNR / PSNR-Y / SSIM-Y of the written uint8 still against a ground-truth image, on
    the device (metrics.image_metrics with `quantize`: the values the saved file holds)."""
    from image_super_resolution_amd import metrics
    m = metrics.image_metrics(out.to(device), ref.to(device), sr_space="u8", hr_space="u8", border=border,
                              quantize=True)
    vals = torch.stack([m.psnr, m.psnr_y, m.ssim_y, m.mse, m.mse_y]).cpu()[:, 0].tolist()
    return {"ref": ref_path.as_posix(), "border": border, "psnr": vals[0], "psnr_y": vals[1], "ssim_y": vals[2],
            "mse": vals[3], "mse_y": vals[4]}


def video_formats(kw, source, result: Path):
    """(pix_fmt_in, yuv_in, pix_fmt_out, yuv_out) of a video run.  The input's format is the source's
    (a .y4m header's siting and range, unless a --yuv_* flag is given); the output's follows the
    save_dir suffix, for a container --pix_fmt, and inherits the input's siting, range and depth;
    --out_depth sets the output's depth apart (rgb24 input counts as 8 bits).  A 10-bit .y4m has no tag for
    center siting: without --yuv_siting such an output is left-sited."""
    flags = {k: kw.get(f"yuv_{k}") for k in ("matrix", "range", "siting")}

    def with_flags(fmt: video.YUVFormat) -> video.YUVFormat:
        return video.YUVFormat(fmt.layout, flags["matrix"] or fmt.matrix,
                               fmt.full_range if flags["range"] is None else flags["range"] == "full",
                               flags["siting"] or fmt.siting, fmt.depth)

    yuv_in = getattr(source, "yuv", None)
    pix_in = "rgb24" if yuv_in is None else source.pix_fmt
    if yuv_in is not None:
        yuv_in = with_flags(yuv_in)
    suffix = result.suffix.lower()
    if suffix in (".bgr", ".raw"):
        pix_out = "bgr24"
    elif suffix in YUV_OUT:
        pix_out = YUV_OUT[suffix]
    else:
        pix_out = "bgr24" if (kw.get("pix_fmt") or "rgb24") == "rgb24" else kw["pix_fmt"]
    yuv_out = None
    if pix_out != "bgr24":
        like = yuv_in or video.YUVFormat()
        # a file of frames inherits the input's depth; a container follows --pix_fmt
        depth = kw.get("out_depth") or (like.depth if suffix in YUV_OUT else video.yuvmod.PIX_FMT_DEPTH[pix_out])
        siting = like.siting
        if depth == 10 and suffix == ".y4m" and flags["siting"] is None:
            siting = "left"
        yuv_out = with_flags(video.YUVFormat(video.yuvmod.PIX_FMTS[pix_out], "auto", like.full_range, siting, depth))
        pix_out = yuv_out.pix_fmt
    return pix_in, yuv_in, pix_out, yuv_out


def run_video(kw, device) -> None:
    """rs.py:54-76: frames → HIP graph forward → BGR (or 4:2:0) frames → recorder."""
    src, result = Path(kw["src"]), Path(kw["save_dir"])
    wh = kw.get("video_size")
    w, h = (int(v) for v in wh.lower().split("x")) if wh else (None, None)
    source = video.open_video(src, w, h, kw.get("fps") or 30.0, kw.get("pix_fmt") or "rgb24")
    pix_in, yuv_in, pix_out, yuv_out = video_formats(kw, source, result)
    model = build_model(kw["model"], kw["add_rate"], kw["mean"], kw["std"])
    runner = tiler.runner_for(model, device)
    up = video.FrameUpscaler(runner.gw, source.height, source.width, kw["batch_size"], runner.mean, runner.std,
                             device, pix_fmt_in=pix_in, pix_fmt_out=pix_out, yuv_in=yuv_in, yuv_out=yuv_out)
    H, W = up.out_hw
    if result.suffix.lower() == ".y4m":
        rec = video.Y4MRecorder(result, (W, H), source.fps, up.yuv_out)
    elif result.suffix.lower() in (".bgr", ".raw", *YUV_OUT):
        rec = video.RawRecorder(result, (W, H), source.fps)
    else:
        result = result.with_suffix(".mp4")
        rec = video.FFMPEG_recorder(result.as_posix(), (W, H), source.fps, pix_fmt=pix_out, yuv=up.yuv_out)
    t0 = time.perf_counter()
    n = video.VideoUpscaler(up).run(source, rec)
    rec.stopRecorder()
    dt = time.perf_counter() - t0
    if src.suffix.lower() in VID_FORMATS:
        rec.addAudio(src.as_posix())
    print(f"{n} frames {source.width}x{source.height} -> {W}x{H} in {dt:.2f}s ({n / dt:.2f} fps) -> {result}")


def runer(**kw):
    src, result = Path(kw["src"]), Path(kw["save_dir"])
    if kw.get("wino") is not None:  # the default of every pack / plan below (else ISR_WINO, else off)
        from image_super_resolution_amd import engine
        engine.WINO_DEFAULT = engine.wino_mode(kw["wino"])
    if is_video(kw["src"]):
        if kw.get("self_ensemble"):
            raise ValueError(SELF_ENSEMBLE_VIDEO.format(src=src))
        if not torch.cuda.is_available():
            raise RuntimeError("rs.py runs the HIP generator and needs a GPU")
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(device)
        return run_video(kw, device)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise RuntimeError("rs.py runs the HIP generator and needs a GPU")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=device)
    mean, std = kw["mean"], kw["std"]
    model = build_model(kw["model"], kw["add_rate"], mean, std)
    runner = tiler.runner_for(model, device)
    up = tiler.TileUpscaler(runner, runner.scale, window=kw["window_size"], halo=kw["halo"],
                            batch=kw["batch_size"], device=device, shard=kw.get("shard", "windows"),
                            gather=kw.get("gather", "device"), self_ensemble=bool(kw.get("self_ensemble")))
    image = read_image(src)
    ref = None
    if kw.get("ref"):  # every rank checks, so a refusal ends them all
        ref = read_ref(Path(kw["ref"]), (image.shape[1] * runner.scale, image.shape[2] * runner.scale))
    if rank == 0:
        print("input shape", tuple(image.shape))
    t0 = time.perf_counter()
    out = up(image, rank=rank, world=world)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if rank == 0:
        result = result.with_suffix(".png")
        write_png(out, result)
        mpix = out.shape[1] * out.shape[2] / 1e6
        print("output shape", tuple(out.shape), result.as_posix(), f"{dt:.3f}s {mpix / dt:.1f} MPix/s")
        if kw.get("ref"):
            print(json.dumps(compare_with_ref(out, ref, Path(kw["ref"]), kw.get("ref_border", 4), device)))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


SELF_ENSEMBLE_VIDEO = ("--self_ensemble is for stills: {src} is a video source, and eight forwards per frame is "
                       "not a video feature")


def is_video(src: str) -> bool:
    return Path(src).suffix.lower() in VID_FORMATS + RAW_FORMATS + YUV_FORMATS


def parse(argv=None):
    """The parsed command line; what the flags rule out together is refused here, before any work."""
    p = build_parser()
    opt = p.parse_args(argv)
    if opt.self_ensemble and is_video(opt.src):
        p.error(SELF_ENSEMBLE_VIDEO.format(src=opt.src))
    return opt


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument("--model", type=str, default="")
    p.add_argument("--src", type=str, default="")
    p.add_argument("--save_dir", type=str, default="result.jpg")
    p.add_argument("--window_size", type=int, default=96)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--worker", type=int, default=4, help="accepted for CLI compatibility (decode is in-process)")
    p.add_argument("--halo", type=int, default=0, help="LR pixels of context around each window (0 = reference)")
    p.add_argument("--shard", choices=("windows", "bands", "blocks"), default="windows",
                   help="windows (the reference's, default), full-width bands or a 2-D grid of blocks with the "
                        "same halo: fewer, larger forwards (cfg4 on one MI355X: 576 vs 460 MPix/s with --halo 32)")
    p.add_argument("--gather", choices=("device", "host"), default="device",
                   help="multi-GPU: finished tiles to rank 0's device (p2p) or into one shared host canvas")
    p.add_argument("--add_rate", type=float, default=0.2)
    p.add_argument("--mean", type=float, nargs=3, default=(0.485, 0.456, 0.406))
    p.add_argument("--std", type=float, nargs=3, default=(0.229, 0.224, 0.225))
    p.add_argument("--video_size", type=str, default=None, help="WxH of a raw rgb24 video input")
    p.add_argument("--fps", type=float, default=None, help="frame rate of a raw rgb24 video input")
    p.add_argument("--wino", choices=("off", "final", "rdb"), default=None,
                   help="opt-in fp16 Winograd F(2,3) convs: the RDB final convs or all RDB convs; the trunk then "
                        "runs per conv (default off, or ISR_WINO)")
    p.add_argument("--ref", type=str, default="", help="ground-truth image of the output's size: after the still "
                   "is written, print one JSON line with its PSNR / PSNR-Y / SSIM-Y against it (image branch)")
    p.add_argument("--self_ensemble", action="store_true",
                   help="image branch: average the outputs of the 8 flipped / rotated copies of every tile in fp32 "
                        "before the only rounding (geometric self-ensemble, 8 x the cost); refused for video")
    p.add_argument("--ref_border", type=int, default=4, help="pixels cropped from every side before the metrics")
    p.add_argument("--pix_fmt", choices=("rgb24", "yuv420p", "nv12", "yuv420p10le", "p010le"), default="rgb24",
                   help="video through ffmpeg: the frames piped from the decoder and to the encoder (rgb24: rgb24 in, "
                        "bgr24 out; yuv420p / nv12: 8-bit 4:2:0 both ways, yuv420p10le / p010le: 10-bit, colour "
                        "conversion on the GPU).  .y4m / .yuv / .i420 / .nv12 sources and save_dirs carry their own "
                        "layout; for a raw .yuv / .i420 / .nv12 source a 10-bit name says it holds 16-bit words")
    p.add_argument("--out_depth", type=int, choices=(8, 10), default=None,
                   help="4:2:0 output: bits per sample (default: the input's; rgb24 input counts as 8)")
    p.add_argument("--yuv_matrix", choices=("auto", "bt601", "bt709"), default=None,
                   help="4:2:0 frames: the matrix (default auto: bt709 at a height of 720 or more, else bt601)")
    p.add_argument("--yuv_range", choices=("limited", "full"), default=None,
                   help="4:2:0 frames: the range (default: the .y4m header's, else limited)")
    p.add_argument("--yuv_siting", choices=("left", "center"), default=None,
                   help="4:2:0 frames: the chroma siting (default: the .y4m header's, else left)")
    return p


if __name__ == "__main__":
    runer(**vars(parse()))
