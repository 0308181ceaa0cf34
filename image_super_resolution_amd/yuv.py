"""8-bit YUV 4:2:0 video frames on the device (libisr's csrc/yuv.hip, include/isr.h): I420 / NV12
frames <-> planar uint8 RGB [n, 3, h, w], BT.601 or BT.709, limited or full range, left (MPEG-2 /
H.264 / HEVC) or center (JPEG / MPEG-1) chroma siting, in integer arithmetic from coefficients made
on the host by libisr (`coeffs`, plain C++).  What a video decoder hands over and an encoder takes,
so the video path (video.py) can stage 1.5 bytes per pixel instead of 3 and needs no RGB conversion
on the host.

A YUVFormat of depth 10 (csrc/yuv16.hip) is yuv420p10le (I420 order) or p010le (NV12 order, the sample in
the high bits of its word): frames are still uint8 byte tensors, 3 h w bytes each, of little-endian
16-bit words (on the host: a numpy '<u2' view).  The RGB side is then an int16 tensor of 0..1023
(torch has no arithmetic on uint16; the bits are those of a uint16), the head's normalised fp32 input
(`normalize=`) or the tail's fp32 tanh (an fp32 `rgb`).

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
PIX_FMTS = {"yuv420p": "i420", "nv12": "nv12", "yuv420p10le": "i420", "p010le": "nv12"}  # ffmpeg's name -> layout
PIX_FMT_DEPTH = {"yuv420p": 8, "nv12": 8, "yuv420p10le": 10, "p010le": 10}
DEPTHS = (8, 10)
RGB_KINDS = ("u16", "norm_f32", "tanh_f32")  # index = ISR_RGB_U16 / NORM_F32 / TANH_F32


@dataclass(frozen=True)
class YUVFormat:
    """One 4:2:0 frame format.  matrix "auto" resolves per frame size (`resolved`): bt709 at a
    height of 720 or more, bt601 below, the usual player rule for untagged video; an upscaler's
    input and output frames each resolve by their own height.  depth 10: samples in 16-bit words,
    yuv420p10le (i420) or p010le (nv12)."""
    layout: str = "i420"
    matrix: str = "auto"
    full_range: bool = False
    siting: str = "left"
    depth: int = 8

    def __post_init__(self):
        if self.layout not in LAYOUTS:
            raise ValueError(f"YUVFormat: unknown layout {self.layout!r}; one of {', '.join(LAYOUTS)}")
        if self.matrix != "auto" and self.matrix not in MATRICES:
            raise ValueError(f"YUVFormat: unknown matrix {self.matrix!r}; auto, {', '.join(MATRICES)}")
        if self.siting not in SITINGS:
            raise ValueError(f"YUVFormat: unknown siting {self.siting!r}; one of {', '.join(SITINGS)}")
        if self.depth not in DEPTHS:
            raise ValueError(f"YUVFormat: depth {self.depth!r}; 8 or 10")

    @classmethod
    def of_pix_fmt(cls, pix_fmt: str, **kw) -> "YUVFormat":
        if pix_fmt not in PIX_FMTS:
            raise ValueError(f"not a 4:2:0 pixel format: {pix_fmt!r}; one of {', '.join(PIX_FMTS)}")
        return cls(layout=PIX_FMTS[pix_fmt], depth=PIX_FMT_DEPTH[pix_fmt], **kw)

    @property
    def pix_fmt(self) -> str:
        if self.depth == 10:
            return "p010le" if self.layout == "nv12" else "yuv420p10le"
        return "nv12" if self.layout == "nv12" else "yuv420p"

    @property
    def shift(self) -> int:
        """The sample's position in its 16-bit word (depth 10): p010le keeps it in the high bits."""
        return 16 - self.depth if self.depth > 8 and self.layout == "nv12" else 0

    def resolved(self, height: int) -> "YUVFormat":
        if self.matrix != "auto":
            return self
        return YUVFormat(self.layout, "bt709" if height >= 720 else "bt601", self.full_range, self.siting, self.depth)


def check_size(h: int, w: int) -> None:
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"4:2:0 frames need an even height and width of at least 2, got {w}x{h}")


def frame_bytes(h: int, w: int, depth: int = 8) -> int:
    check_size(h, w)
    if depth not in DEPTHS:
        raise ValueError(f"frame_bytes: depth {depth!r}; 8 or 10")
    return 3 * h * w // 2 if depth == 8 else 3 * h * w


def frame_shape(h: int, w: int, depth: int = 8) -> tuple[int, int]:
    """A frame as rows of bytes: (3h/2, w), at depth 10 (3h/2, 2w)."""
    check_size(h, w)
    return (3 * h // 2, w if depth == 8 else 2 * w)


def coeffs(matrix: str, full_range: bool = False, depth: int = 8):
    """(fwd int32 [3, 3]: rows Y, Cb, Cr over R, G, B; inv int32 [5]: cy, crv, cbu, cgu, cgv) with 16
    fractional bits, from libisr's host code (isr_yuv_coeffs, at another depth isr_yuv_coeffs_depth; no
    GPU)."""
    if matrix not in MATRICES:
        raise ValueError(f"coeffs: unknown matrix {matrix!r}; one of {', '.join(MATRICES)}")
    fwd, inv = np.zeros((3, 3), dtype=np.int32), np.zeros(5, dtype=np.int32)
    if depth == 8:
        _lib.check(_lib.load().isr_yuv_coeffs(MATRICES.index(matrix), int(bool(full_range)), fwd.ctypes.data,
                                              inv.ctypes.data), "isr_yuv_coeffs")
    else:
        _lib.check(_lib.load().isr_yuv_coeffs_depth(MATRICES.index(matrix), int(bool(full_range)), int(depth),
                                                    fwd.ctypes.data, inv.ctypes.data), "isr_yuv_coeffs_depth")
    return fwd, inv


def _desc(n: int, h: int, w: int, fmt: YUVFormat, src: int, dst: int) -> _lib.IsrYuvDesc:
    fmt = fmt.resolved(h)
    fwd, inv = coeffs(fmt.matrix, fmt.full_range)
    return _lib.IsrYuvDesc(n, h, w, LAYOUTS.index(fmt.layout), SITINGS.index(fmt.siting), int(fmt.full_range),
                           (ctypes.c_int32 * 9)(*fwd.ravel().tolist()), (ctypes.c_int32 * 5)(*inv.tolist()), src, dst)


def inv_std_of(std) -> list[float]:
    """The fp32 reciprocals ISR_RGB_NORM_F32 multiplies by: 1 / std in fp64 rounded to fp32, the head
    descriptor's own (ops.py)."""
    return [float(np.float32(1.0 / float(s))) for s in std]


def _desc16(n: int, h: int, w: int, fmt: YUVFormat, kind: str, src: int, dst: int, mean=(0.0, 0.0, 0.0),
            std=(1.0, 1.0, 1.0)) -> _lib.IsrYuv16Desc:
    fmt = fmt.resolved(h)
    fwd, inv = coeffs(fmt.matrix, fmt.full_range, fmt.depth)
    return _lib.IsrYuv16Desc(n, h, w, LAYOUTS.index(fmt.layout), SITINGS.index(fmt.siting), int(fmt.full_range),
                             fmt.depth, fmt.shift, RGB_KINDS.index(kind), (ctypes.c_int32 * 9)(*fwd.ravel().tolist()),
                             (ctypes.c_int32 * 5)(*inv.tolist()), (ctypes.c_float * 3)(*[float(m) for m in mean]),
                             (ctypes.c_float * 3)(*inv_std_of(std)), src, dst)


def _on_device(t, what: str, dtypes=(torch.uint8,)) -> None:
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what}: the input must be a HIP device tensor (the colour conversion runs on the "
                           f"MI355X HIP path only; got {getattr(t, 'device', type(t))})")
    if t.dtype not in dtypes:
        raise ValueError(f"{what}: expected {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")


U16_DTYPES = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)  # int16 is the default


def _yuv420_to_rgb16(frames, h, w, fmt, out, normalize):
    """Depth 10: byte frames [n, 3 h w] -> int16 RGB of 0..1023, or with normalize=(mean, std) the head's
    fp32 input ((v / 1023 - mean) / std as the head forms it: times the fp32 reciprocal of std)."""
    _on_device(frames, "yuv420_to_rgb")
    fb = frame_bytes(h, w, fmt.depth)
    if frames.numel() == 0 or frames.numel() % fb:
        raise ValueError(f"yuv420_to_rgb: {frames.numel()} bytes is not a whole number of {w}x{h} 4:2:0 frames of "
                         f"{fmt.depth} bits")
    x = frames.contiguous()
    n = x.numel() // fb
    dtypes = (torch.float32,) if normalize is not None else U16_DTYPES
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=dtypes[0], device=x.device)
    elif not (out.is_cuda and out.dtype in dtypes and out.is_contiguous() and tuple(out.shape) == (n, 3, h, w)):
        raise ValueError(f"yuv420_to_rgb: out must be a contiguous {dtypes[0]} device tensor {(n, 3, h, w)}")
    mean, std = normalize if normalize is not None else ((0.0,) * 3, (1.0,) * 3)
    with torch.cuda.device(x.device):
        d = _desc16(n, h, w, fmt, "norm_f32" if normalize is not None else "u16", x.data_ptr(), out.data_ptr(), mean, std)
        _lib.check(_lib.load().isr_yuv420_to_rgb_16(ctypes.byref(d), _stream()), "isr_yuv420_to_rgb_16")
    return out


def _rgb_to_yuv420_16(rgb, fmt, out):
    """Depth 10: int16 / uint16 RGB of 0..1023, or the tail's fp32 tanh, -> byte frames [n, 3h/2, 2w]."""
    _on_device(rgb, "rgb_to_yuv420", (*U16_DTYPES, torch.float32))
    if rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"rgb_to_yuv420: expected [n, 3, h, w], got {tuple(rgb.shape)}")
    x = rgb.contiguous()
    n, _, h, w = x.shape
    fb = frame_bytes(h, w, fmt.depth)
    if out is None:
        out = torch.empty((n, *frame_shape(h, w, fmt.depth)), dtype=torch.uint8, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * fb):
        raise ValueError(f"rgb_to_yuv420: out must be a contiguous uint8 device tensor of {n} x {fb} bytes")
    with torch.cuda.device(x.device):
        d = _desc16(n, h, w, fmt, "tanh_f32" if x.dtype == torch.float32 else "u16", x.data_ptr(), out.data_ptr())
        _lib.check(_lib.load().isr_rgb_to_yuv420_16(ctypes.byref(d), _stream()), "isr_rgb_to_yuv420_16")
    return out


def yuv420_to_rgb(frames: torch.Tensor, h: int, w: int, fmt: YUVFormat = YUVFormat(),
                  out: torch.Tensor | None = None, *, normalize=None) -> torch.Tensor:
    """uint8 frames [n, 3 h w / 2] (or [n, 3 h / 2, w], or one flat frame) -> uint8 RGB [n, 3, h, w]:
    one isr_yuv420_to_rgb_u8 launch on the current stream.  A depth-10 `fmt`: byte frames [n, 3 h w] ->
    int16 RGB of 0..1023, or with normalize=(mean, std) the head's normalised fp32 input: one
    isr_yuv420_to_rgb_16 launch."""
    if fmt.depth != 8:
        return _yuv420_to_rgb16(frames, h, w, fmt, out, normalize)
    if normalize is not None:
        raise ValueError("yuv420_to_rgb: normalize= needs a depth-10 format (8-bit frames give uint8 RGB, which the "
                         "head normalises itself)")
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
    rows, then the chroma of the layout): one isr_rgb_to_yuv420_u8 launch on the current stream.  A
    depth-10 `fmt`: int16 / uint16 RGB of 0..1023, or an fp32 `rgb` taken as the tail's tanh output, ->
    byte frames [n, 3 h / 2, 2 w]: one isr_rgb_to_yuv420_16 launch."""
    if fmt.depth != 8:
        return _rgb_to_yuv420_16(rgb, fmt, out)
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
