"""PSNR, PSNR-Y and SSIM-Y on the device (libisr's isr_image_metrics, include/isr.h).

The reference computes no metric: it defines the BT.601 luma with a 4-pixel crop (Ychannel,
utils/datasets.py:159-166) and writes a val_images.json (utils/general.py:107-111), and neither is
used.  The definitions here are the literature's, on the region left after cropping `border`
pixels from every side, everything on the [0, 1] scale:

* PSNR    = -10 log10(mean (a - b)^2) over the three channels (peak 1; on the same images this is
  the peak-2 PSNR of the [-1, 1] tanh space);
* PSNR-Y  = the same on Y = (65.481 r + 128.553 g + 24.966 b + 16) / 255;
* SSIM-Y  = mean SSIM (Wang et al. 2004) of Y*255: 11 x 11 Gaussian window of sigma 1.5 normalised
  to sum 1, valid positions only, biased window-weighted variances, C1 = (0.01*255)^2,
  C2 = (0.03*255)^2.

Inputs stay where they are: uint8 or fp32 NCHW device tensors in one of the spaces below, mapped
to [0, 1] inside the kernel.  Nothing here synchronises with the host except `Evaluator.result`.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib
from .data import IMAGENET_MEAN, IMAGENET_STD

SPACES = ("u8", "tanh", "unit", "norm")


class Metrics(NamedTuple):
    """Per-image device fp64 tensors [n]."""
    psnr: torch.Tensor
    psnr_y: torch.Tensor
    ssim_y: torch.Tensor
    mse: torch.Tensor
    mse_y: torch.Tensor


def _affine(space: str, mean, std):
    """(scale[3], shift[3]) with value in [0, 1] = v * scale + shift."""
    if space == "u8":
        return (1.0 / 255.0,) * 3, (0.0,) * 3
    if space == "tanh":
        return (0.5,) * 3, (0.5,) * 3
    if space == "unit":
        return (1.0,) * 3, (0.0,) * 3
    if space == "norm":
        return tuple(float(v) for v in std), tuple(float(v) for v in mean)
    raise ValueError(f"image_metrics: space {space!r} is not one of {SPACES}")


def _checked(t: torch.Tensor, space: str, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"image_metrics: {what} must be a HIP device tensor (the metrics run on the MI355X HIP "
                           f"path only; got {getattr(t, 'device', type(t))})")
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"image_metrics: {what} must be [n, 3, h, w] or [3, h, w], got {tuple(t.shape)}")
    want = torch.uint8 if space == "u8" else torch.float32
    if t.dtype != want:
        raise ValueError(f"image_metrics: {what} in space {space!r} must be {want}, got {t.dtype}")
    return t.contiguous()


def image_metrics(sr: torch.Tensor, hr: torch.Tensor, *, sr_space: str, hr_space: str, border: int = 4,
                  clamp: bool = True, quantize: bool = False, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                  stream: torch.cuda.Stream | None = None) -> Metrics:
    """Metrics of the estimate `sr` against the ground truth `hr` (same shape), one kernel pass.

    Spaces: "u8" (uint8 0..255), "tanh" ([-1, 1], the generator's output), "unit" ([0, 1]) and
    "norm" (Normalize'd with `mean` / `std`).  `clamp` clamps both to [0, 1]; `quantize` rounds
    them to the 8-bit value a saved image holds.  PSNR is inf where the error is 0."""
    sa, ha = _affine(sr_space, mean, std)
    sb, hb = _affine(hr_space, mean, std)
    a, b = _checked(sr, sr_space, "sr"), _checked(hr, hr_space, "hr")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"image_metrics: sr {tuple(a.shape)} on {a.device} and hr {tuple(b.shape)} on {b.device} "
                         "must have one shape and device")
    n, _, h, w = a.shape
    lib = _lib.load()
    f3 = ctypes.c_float * 3
    with torch.cuda.device(a.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        out = torch.empty((n, 4), dtype=torch.float64, device=a.device)
        d = _lib.IsrMetricsDesc(n, h, w, int(border), a.data_ptr(), b.data_ptr(), int(a.dtype == torch.uint8),
                                int(b.dtype == torch.uint8), f3(*sa), f3(*ha), f3(*sb), f3(*hb), int(bool(clamp)),
                                int(bool(quantize)), out.data_ptr())
        nbytes = lib.isr_image_metrics_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            raise _lib.IsrError("isr_image_metrics refused the descriptor: " +
                                lib.isr_last_error().decode(errors="replace"))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        cur = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.isr_image_metrics(ctypes.byref(d), ws.data_ptr(), nbytes, cur), "isr_image_metrics")
        mse, mse_y, ssim = out[:, 0], out[:, 1], out[:, 2]
        return Metrics(-10.0 * torch.log10(mse), -10.0 * torch.log10(mse_y), ssim, mse, mse_y)


class Evaluator:
    """Running means of PSNR / PSNR-Y / SSIM-Y over images, accumulated on the device.

    `update` adds a batch's per-image values into a 4-element fp64 accumulator (sums of psnr,
    psnr_y, ssim_y, and the image count) without touching the host; `result` is the only host
    read.  `state` / `merge` expose that accumulator as a plain tensor, so a data-parallel run
    combines its ranks with one all_reduce(SUM) (`all_reduce`)."""

    def __init__(self, device=None):
        self.acc = torch.zeros(4, dtype=torch.float64, device=device) if device is not None else None

    def add(self, m: Metrics) -> None:
        """Add per-image values already computed (tensors [n] on the accumulator's device)."""
        s = torch.stack([m.psnr.double().sum(), m.psnr_y.double().sum(), m.ssim_y.double().sum(),
                         torch.full((), float(m.psnr.numel()), dtype=torch.float64, device=m.psnr.device)])
        if self.acc is None:
            self.acc = torch.zeros(4, dtype=torch.float64, device=s.device)
        self.acc += s

    def update(self, sr: torch.Tensor, hr: torch.Tensor, **kw) -> Metrics:
        """image_metrics(sr, hr, **kw) added to the running sums; returns the batch's values."""
        m = image_metrics(sr, hr, **kw)
        self.add(m)
        return m

    def state(self) -> torch.Tensor:
        if self.acc is None:
            raise RuntimeError("Evaluator.state: nothing accumulated and no device given")
        return self.acc.clone()

    def merge(self, state: torch.Tensor) -> None:
        state = state.to(torch.float64)
        if self.acc is None:
            self.acc = torch.zeros(4, dtype=torch.float64, device=state.device)
        self.acc += state.to(self.acc.device)

    def all_reduce(self, group=None) -> None:
        """Sum the accumulators of every rank of `group` (one collective)."""
        import torch.distributed as dist
        dist.all_reduce(self.acc, op=dist.ReduceOp.SUM, group=group)

    def result(self) -> dict:
        """{"psnr", "psnr_y", "ssim_y": means over images, "images": count}: the one host read."""
        if self.acc is None:
            return {"psnr": float("nan"), "psnr_y": float("nan"), "ssim_y": float("nan"), "images": 0}
        p, py, s, n = self.acc.tolist()
        if n == 0:
            return {"psnr": float("nan"), "psnr_y": float("nan"), "ssim_y": float("nan"), "images": 0}
        return {"psnr": p / n, "psnr_y": py / n, "ssim_y": s / n, "images": int(n)}
