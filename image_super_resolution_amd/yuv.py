"""8-bit YUV 4:2:0 video frames on the device (libisr's csrc/yuv.hip, include/isr.h): I420 / NV12
frames <-> planar uint8 RGB [n, 3, h, w], BT.601 or BT.709, limited or full range, left (MPEG-2 /
H.264 / HEVC) or center (JPEG / MPEG-1) chroma siting, in integer arithmetic from coefficients made
on the host by libisr (`coeffs`, plain C++).  What a video decoder hands over and an encoder takes,
so the video path (video.py) can stage 1.5 bytes per pixel instead of 3 and needs no RGB conversion
on the host.

GPU-only, like the rest of the product path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .ops import _stream

LAYOUTS = ("i420", "nv12")      # index = ISR_YUV_I420 / NV12
MATRICES = ("bt601", "bt709")   # index = ISR_YUV_BT601 / BT709
SITINGS = ("left", "center")    # index = ISR_YUV_SITING_LEFT / CENTER
PIX_FMTS = {"yuv420p": "i420", "nv12": "nv12"}  # ffmpeg's name -> layout


@dataclass(frozen=True)
class YUVFormat:
    """One 4:2:0 frame format.  matrix "auto" resolves per frame size (`resolved`): bt709 at a
    height of 720 or more, bt601 below, the usual player rule for untagged video; an upscaler's
    input and output frames each resolve by their own height."""
    layout: str = "i420"
    matrix: str = "auto"
    full_range: bool = False
    siting: str = "left"

    def __post_init__(self):
        if self.layout not in LAYOUTS:
            raise ValueError(f"YUVFormat: unknown layout {self.layout!r}; one of {', '.join(LAYOUTS)}")
        if self.matrix != "auto" and self.matrix not in MATRICES:
            raise ValueError(f"YUVFormat: unknown matrix {self.matrix!r}; auto, {', '.join(MATRICES)}")
        if self.siting not in SITINGS:
            raise ValueError(f"YUVFormat: unknown siting {self.siting!r}; one of {', '.join(SITINGS)}")

    @classmethod
    def of_pix_fmt(cls, pix_fmt: str, **kw) -> "YUVFormat":
        if pix_fmt not in PIX_FMTS:
            raise ValueError(f"not a 4:2:0 pixel format: {pix_fmt!r}; one of {', '.join(PIX_FMTS)}")
        return cls(layout=PIX_FMTS[pix_fmt], **kw)

    @property
    def pix_fmt(self) -> str:
        return "nv12" if self.layout == "nv12" else "yuv420p"

    def resolved(self, height: int) -> "YUVFormat":
        if self.matrix != "auto":
            return self
        return YUVFormat(self.layout, "bt709" if height >= 720 else "bt601", self.full_range, self.siting)


def check_size(h: int, w: int) -> None:
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"4:2:0 frames need an even height and width of at least 2, got {w}x{h}")


def frame_bytes(h: int, w: int) -> int:
    check_size(h, w)
    return 3 * h * w // 2


def coeffs(matrix: str, full_range: bool = False):
    """(fwd int32 [3, 3]: rows Y, Cb, Cr over R, G, B; inv int32 [5]: cy, crv, cbu, cgu, cgv) with 16
    fractional bits, from libisr's host code (isr_yuv_coeffs, no GPU)."""
    if matrix not in MATRICES:
        raise ValueError(f"coeffs: unknown matrix {matrix!r}; one of {', '.join(MATRICES)}")
    fwd, inv = np.zeros((3, 3), dtype=np.int32), np.zeros(5, dtype=np.int32)
    _lib.check(_lib.load().isr_yuv_coeffs(MATRICES.index(matrix), int(bool(full_range)), fwd.ctypes.data,
                                          inv.ctypes.data), "isr_yuv_coeffs")
    return fwd, inv


def _desc(n: int, h: int, w: int, fmt: YUVFormat, src: int, dst: int) -> _lib.IsrYuvDesc:
    fmt = fmt.resolved(h)
    fwd, inv = coeffs(fmt.matrix, fmt.full_range)
    return _lib.IsrYuvDesc(n, h, w, LAYOUTS.index(fmt.layout), SITINGS.index(fmt.siting), int(fmt.full_range),
                           (ctypes.c_int32 * 9)(*fwd.ravel().tolist()), (ctypes.c_int32 * 5)(*inv.tolist()), src, dst)


def _on_device(t, what: str) -> None:
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what}: the input must be a HIP device tensor (the colour conversion runs on the "
                           f"MI355X HIP path only; got {getattr(t, 'device', type(t))})")
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: expected uint8, got {t.dtype}")


def yuv420_to_rgb(frames: torch.Tensor, h: int, w: int, fmt: YUVFormat = YUVFormat(),
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 frames [n, 3 h w / 2] (or [n, 3 h / 2, w], or one flat frame) -> uint8 RGB [n, 3, h, w]:
    one isr_yuv420_to_rgb_u8 launch on the current stream."""
    _on_device(frames, "yuv420_to_rgb")
    fb = frame_bytes(h, w)
    if frames.numel() == 0 or frames.numel() % fb:
        raise ValueError(f"yuv420_to_rgb: {frames.numel()} bytes is not a whole number of {w}x{h} 4:2:0 frames")
    x = frames.contiguous()
    n = x.numel() // fb
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.uint8, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (n, 3, h, w)):
        raise ValueError(f"yuv420_to_rgb: out must be a contiguous uint8 device tensor {(n, 3, h, w)}")
    with torch.cuda.device(x.device):
        d = _desc(n, h, w, fmt, x.data_ptr(), out.data_ptr())
        _lib.check(_lib.load().isr_yuv420_to_rgb_u8(ctypes.byref(d), _stream()), "isr_yuv420_to_rgb_u8")
    return out


def rgb_to_yuv420(rgb: torch.Tensor, fmt: YUVFormat = YUVFormat(), out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 RGB [n, 3, h, w] -> uint8 frames [n, 3 h / 2, w] (a frame's bytes in order: the Y plane's
    rows, then the chroma of the layout): one isr_rgb_to_yuv420_u8 launch on the current stream."""
    _on_device(rgb, "rgb_to_yuv420")
    if rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"rgb_to_yuv420: expected uint8 [n, 3, h, w], got {tuple(rgb.shape)}")
    x = rgb.contiguous()
    n, _, h, w = x.shape
    check_size(h, w)
    if out is None:
        out = torch.empty((n, 3 * h // 2, w), dtype=torch.uint8, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * frame_bytes(h, w)):
        raise ValueError(f"rgb_to_yuv420: out must be a contiguous uint8 device tensor of {n} x {frame_bytes(h, w)} bytes")
    with torch.cuda.device(x.device):
        d = _desc(n, h, w, fmt, x.data_ptr(), out.data_ptr())
        _lib.check(_lib.load().isr_rgb_to_yuv420_u8(ctypes.byref(d), _stream()), "isr_rgb_to_yuv420_u8")
    return out
