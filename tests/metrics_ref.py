"""fp64 restatement of the three image metrics (CPU, test-only), written from their definitions.

Everything is on the region left after cropping `border` pixels from every side, on the [0, 1]
scale:
  mse_rgb  mean over 3*hc*wc values of (a - b)^2
  mse_y    mean over hc*wc of (Ya - Yb)^2, Y = oracle.ref_cpu.y_channel (BT.601 luma)
  ssim_y   Wang et al. 2004 on Y*255: 11 x 11 Gaussian window (sigma 1.5, normalised to sum 1) from
           the formula, valid positions only (F.conv2d without padding, float64), biased
           window-weighted variances, C1 = (0.01*255)^2, C2 = (0.03*255)^2, mean of the SSIM map.
Spaces: "u8" (x/255), "tanh" (x*0.5 + 0.5), "unit" (x), "norm" (x*std + mean).  The C ABI carries
the affine as fp32 (isr_metrics_desc.a_scale ...), so the restatement rounds std / mean to fp32 as
well: with other constants a value next to a quantisation tie could round the other way.
"""
import math

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def window() -> torch.Tensor:
    """The 11 x 11 Gaussian of sigma 1.5, normalised to sum 1 (float64)."""
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k[:, None] ** 2 + k[None, :] ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def to_unit(x: torch.Tensor, space: str, *, clamp=True, quantize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[n,3,h,w] in `space` → float64 in [0, 1] with the clamp / quantise options."""
    x = x.double()
    if space == "u8":
        x = x / 255.0
    elif space == "tanh":
        x = x * 0.5 + 0.5
    elif space == "norm":
        s = torch.tensor(std, dtype=torch.float32).double().view(1, 3, 1, 1)
        m = torch.tensor(mean, dtype=torch.float32).double().view(1, 3, 1, 1)
        x = x * s + m
    elif space != "unit":
        raise ValueError(space)
    if clamp:
        x = x.clamp(0.0, 1.0)
    if quantize:
        x = torch.round(x * 255.0) / 255.0  # round half even
    return x


def crop(x: torch.Tensor, border: int) -> torch.Tensor:
    return x[..., border:x.shape[-2] - border, border:x.shape[-1] - border]


def ssim_y(a01: torch.Tensor, b01: torch.Tensor) -> torch.Tensor:
    """Per-image mean SSIM of the luma of two float64 [n,3,h,w] images in [0, 1] (already cropped)."""
    x = (R.y_channel(a01) * 255.0)[:, None]
    y = (R.y_channel(b01) * 255.0)[:, None]
    w = window()[None, None]
    mx, my = F.conv2d(x, w), F.conv2d(y, w)
    vx = F.conv2d(x * x, w) - mx * mx
    vy = F.conv2d(y * y, w) - my * my
    cxy = F.conv2d(x * y, w) - mx * my
    s = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return s.flatten(1).mean(1)


def metrics(a, b, a_space, b_space, border=4, clamp=True, quantize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """dict of float64 [n] tensors: mse, mse_y, ssim_y, psnr, psnr_y (PSNR = -10 log10(mse), peak 1)."""
    a01 = crop(to_unit(a, a_space, clamp=clamp, quantize=quantize, mean=mean, std=std), border)
    b01 = crop(to_unit(b, b_space, clamp=clamp, quantize=quantize, mean=mean, std=std), border)
    mse = ((a01 - b01) ** 2).flatten(1).mean(1)
    mse_y = ((R.y_channel(a01) - R.y_channel(b01)) ** 2).flatten(1).mean(1)
    return {"mse": mse, "mse_y": mse_y, "ssim_y": ssim_y(a01, b01), "psnr": -10 * torch.log10(mse),
            "psnr_y": -10 * torch.log10(mse_y)}


def mse_u8_exact(a: torch.Tensor, b: torch.Tensor, border=4) -> list:
    """mse_rgb of two uint8 images from the exact integer sum of squares, divided once."""
    d = crop(a.to(torch.int64), border) - crop(b.to(torch.int64), border)
    count = d[0].numel()
    return [int(s) / (float(count) * 65025.0) for s in (d * d).flatten(1).sum(1)]


def psnr_y(a01: torch.Tensor, b01: torch.Tensor, border: int = 4) -> float:
    """PSNR of the luma over the whole batch, the quantity oracle.ref_cpu.psnr_y defines."""
    d = R.y_channel(crop(a01.double(), border)) - R.y_channel(crop(b01.double(), border))
    mse = (d ** 2).mean().item()
    return math.inf if mse == 0 else -10.0 * math.log10(mse)
