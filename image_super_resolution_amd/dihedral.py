"""The eight flips and rotations of an image (the dihedral group D4) on the device: libisr's
isr_dihedral, isr_ensemble_expand_u8 and isr_ensemble_reduce (include/isr.h has the definition).

An op id is k = r + 4 f: `torch.rot90(x.flip(-1) if f else x, r, dims=(-2, -1))`, a flip along the width
first, then r counter-clockwise quarter turns; an odd r swaps height and width.  `apply` is the training
augmentation's primitive (data.GPUTransform(augment=...)); `expand_u8` and `reduce` are the two ends of the
x8 geometric self-ensemble (tiler.TileUpscaler(self_ensemble=True)).  HIP only: a CPU tensor raises."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ops import _stream

N_OPS = 8


def inverse(k: int) -> int:
    """The op that undoes op k: (4 - k) % 4 for a rotation, k itself for a reflection (isr_dihedral_inverse)."""
    r = _lib.load().isr_dihedral_inverse(int(k))
    if r < 0:
        raise ValueError(f"dihedral.inverse: op {k} is not in 0..7")
    return r


def _device_batch(x, what: str, dtypes) -> torch.Tensor:
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise RuntimeError(f"{what}: the input must be a HIP device tensor (the dihedral transforms run on the MI355X "
                           f"HIP path only; got {getattr(x, 'device', type(x))})")
    if x.dtype not in dtypes or x.dim() != 4:
        raise ValueError(f"{what}: expected a {' or '.join(str(t) for t in dtypes)} [n, c, h, w] batch, got {x.dtype} "
                         f"{tuple(x.shape)}")
    return x.contiguous()


def apply(x: torch.Tensor, k) -> torch.Tensor:
    """Op k of a uint8 or fp32 device batch [n, c, h, w], one isr_dihedral launch.  `k`: an int in 0..7 for
    the whole batch, or a device int32 tensor [n] of per-image ids (square images only; an id outside 0..7 is
    taken & 7 by the kernel, and nothing is read back)."""
    x = _device_batch(x, "dihedral.apply", (torch.uint8, torch.float32))
    n, c, h, w = x.shape
    if isinstance(k, torch.Tensor):
        if not k.is_cuda or k.dtype != torch.int32 or tuple(k.shape) != (n,):
            raise ValueError(f"dihedral.apply: per-image ops must be a device int32 [{n}] tensor, got {k.dtype} "
                             f"{tuple(k.shape)} on {k.device}")
        if h != w:
            raise ValueError(f"dihedral.apply: per-image ops need square images, got {h}x{w}")
        ops, op, swap = k.contiguous(), 0, False
    else:
        op = int(k)
        if not 0 <= op < N_OPS:
            raise ValueError(f"dihedral.apply: op {k} is not in 0..7")
        ops, swap = None, bool(op & 1)
    with torch.cuda.device(x.device):
        y = torch.empty((n, c, w, h) if swap else (n, c, h, w), dtype=x.dtype, device=x.device)
        if y.numel() == 0:
            return y
        d = _lib.IsrDihedralDesc(n, c, h, w, x.element_size(), op, ops.data_ptr() if ops is not None else None,
                                 x.data_ptr(), y.data_ptr())
        _lib.check(_lib.load().isr_dihedral(ctypes.byref(d), _stream()), "isr_dihedral")
    return y


def expand_u8(x: torch.Tensor):
    """(even, odd): the eight members of each image of a uint8 device batch [n, 3, h, w], one launch
    (isr_ensemble_expand_u8).  Member k of image i is image (k // 2) * n + i of `even` [4n, 3, h, w] for
    k = 0, 2, 4, 6 and of `odd` [4n, 3, w, h] for k = 1, 3, 5, 7."""
    x = _device_batch(x, "dihedral.expand_u8", (torch.uint8,))
    n, c, h, w = x.shape
    if c != 3:
        raise ValueError(f"dihedral.expand_u8: expected 3 channels, got {c}")
    with torch.cuda.device(x.device):
        even = torch.empty((4 * n, 3, h, w), dtype=torch.uint8, device=x.device)
        odd = torch.empty((4 * n, 3, w, h), dtype=torch.uint8, device=x.device)
        d = _lib.IsrEnsembleExpandDesc(n, h, w, x.data_ptr(), even.data_ptr(), odd.data_ptr())
        _lib.check(_lib.load().isr_ensemble_expand_u8(ctypes.byref(d), _stream()), "isr_ensemble_expand_u8")
    return even, odd


def reduce(even: torch.Tensor, odd: torch.Tensor, out_u8: bool = True) -> torch.Tensor:
    """The ensemble's average, one launch (isr_ensemble_reduce): `even` fp32 [4n, 3, h, w] and `odd` fp32
    [4n, 3, w, h] are the network's tanh-range outputs for expand_u8's members; each is taken back by its
    inverse op, the eight are added in fp32 in the order k = 0..7 and scaled by 1/8.  out_u8: quantised once,
    as the generator's tail quantises (round half to even of (m + 1) / 2 * 255, clamped); else fp32."""
    even = _device_batch(even, "dihedral.reduce", (torch.float32,))
    odd = _device_batch(odd, "dihedral.reduce", (torch.float32,))
    n4, c, h, w = even.shape
    if c != 3 or n4 % 4 or n4 == 0 or tuple(odd.shape) != (n4, 3, w, h) or odd.device != even.device:
        raise ValueError(f"dihedral.reduce: expected even [4n, 3, h, w] and odd [4n, 3, w, h] on one device, got "
                         f"{tuple(even.shape)} and {tuple(odd.shape)}")
    with torch.cuda.device(even.device):
        y = torch.empty((n4 // 4, 3, h, w), dtype=torch.uint8 if out_u8 else torch.float32, device=even.device)
        d = _lib.IsrEnsembleReduceDesc(n4 // 4, h, w, even.data_ptr(), odd.data_ptr(), y.data_ptr(), int(out_u8))
        _lib.check(_lib.load().isr_ensemble_reduce(ctypes.byref(d), _stream()), "isr_ensemble_reduce")
    return y
