"""What the training plans (train_engine, denoise, discriminator, vgg) share on the host: the
stride-2 weight algebra, one trainable-conv record with its packing rules, the train-mode
BatchNorm steps and the lease that holds a plan while a live autograd graph needs it.

Stride 2 on the stride-1 kernel, exactly (no zero taps beyond a 2x2 window):
  forward   out(y,x) = Σ W[dy][dx] in(2y+dy-1, 2x+dx-1)  is a conv over the
            PixelUnshuffle'd input (x_sub2 view: channel s*cin + c = in[c] at
            (2y'+a, 2x'+b), s = 2a+b) with phase-expanded weights
            W'[co][s*cin+c][ty][tx] = W[co][c][2ty+a-1][2tx+b-1] on taps {0,1}²;
  dgrad     dx(c, 2y'+a, 2x'+b) is a conv over dz with 4*cin outputs
            W''[4c+s][co][ty][tx] = W[co][c][dy][dx] on taps {1,2}²
            (a=0: ty=1↔dy=1; a=1: ty=2↔dy=0, ty=1↔dy=2), stored through the
            PixelShuffle(2) epilogue;
  wgrad     over the x_sub2 view on taps {0,1}² (isr_wgrad_desc.x_sub2 / taps),
            dW gathered from dW'.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from . import ops
from .ops import ActBuffer, round_up


def expand_fwd(w: torch.Tensor) -> torch.Tensor:
    """W [co][ci][3][3] → W' [co][4ci][3][3] for the x_sub2 conv on taps {0,1}²."""
    co, ci = w.shape[:2]
    out = torch.zeros(co, 4 * ci, 3, 3, device=w.device, dtype=torch.float32)
    # phase a: (ty, dy) pairs with dy = 2ty + a - 1 in [0, 2]
    pairs = {0: [(1, 1)], 1: [(0, 0), (1, 2)]}
    for a in (0, 1):
        for b in (0, 1):
            s = 2 * a + b
            for ty, dy in pairs[a]:
                for tx, dx in pairs[b]:
                    out[:, s * ci:(s + 1) * ci, ty, tx] = w[:, :, dy, dx]
    return out


def expand_dgrad(w: torch.Tensor) -> torch.Tensor:
    """W [co][ci][3][3] → W'' [4ci][co][3][3] (output channel 4c+s) on taps {1,2}²."""
    co, ci = w.shape[:2]
    out = torch.zeros(ci, 4, co, 3, 3, device=w.device, dtype=torch.float32)
    pairs = {0: [(1, 1)], 1: [(2, 0), (1, 2)]}  # (ty, dy)
    wt = w.transpose(0, 1)  # [ci][co][3][3]
    for a in (0, 1):
        for b in (0, 1):
            s = 2 * a + b
            for ty, dy in pairs[a]:
                for tx, dx in pairs[b]:
                    out[:, s, :, ty, tx] = wt[:, :, dy, dx]
    return out.reshape(4 * ci, co, 3, 3).contiguous()


def gather_wgrad(dwp: torch.Tensor, ci: int) -> torch.Tensor:
    """dW' [co][4ci][3][3] (wgrad over the unshuffled input) → dW [co][ci][3][3]."""
    co = dwp.shape[0]
    dw = torch.empty(co, ci, 3, 3, device=dwp.device, dtype=dwp.dtype)
    ty_a = {0: (0, 1), 1: (1, 0), 2: (1, 1)}  # dy → (ty, a)
    for dy in range(3):
        ty, a = ty_a[dy]
        for dx in range(3):
            tx, b = ty_a[dx]
            s = 2 * a + b
            dw[:, :, dy, dx] = dwp[:, s * ci:(s + 1) * ci, ty, tx]
    return dw


def _pad_cin(w: torch.Tensor, cin: int) -> torch.Tensor:
    """Zero input channels up to `cin` (the 3-channel first layer of the discriminator / VGG)."""
    return w if w.shape[1] == cin else nn.functional.pad(w, (0, 0, 0, 0, 0, cin - w.shape[1]))


@dataclass(eq=False)
class TrainConv:
    """One conv layer of a training plan: parameter references + packed copies."""
    w: torch.Tensor
    b: torch.Tensor | None
    cin: int
    cout: int
    kind: str                           # "3x3", "s2" (stride 2), "head", "tail"
    cin_p: int | None = None            # forward input channels after zero padding (default cin)
    dgrad_scale: float = 1.0
    sub2: bool = False                  # dgrad reads the PixelShuffle'd gradient (Scaler)
    bn: nn.BatchNorm2d | None = None    # train-mode BatchNorm2d after the conv
    bn_state: ops.BNState | None = None
    fwd: torch.Tensor | None = None
    bwd: torch.Tensor | None = None

    def __post_init__(self):
        if self.cin_p is None:
            self.cin_p = self.cin

    @classmethod
    def of(cls, m: nn.Module, kind: str | None = None, **kw) -> "TrainConv":
        """From a reference block (`.conv`, optional `.bn`) or a bare nn.Conv2d; `kind`
        defaults to the conv's stride ("s2" / "3x3")."""
        conv = getattr(m, "conv", m)
        bn = getattr(m, "bn", None)
        return cls(conv.weight, conv.bias, conv.in_channels, conv.out_channels,
                   kind or ("s2" if conv.stride[0] == 2 else "3x3"),
                   bn=bn if isinstance(bn, nn.BatchNorm2d) else None, **kw)

    def params(self) -> list[torch.Tensor]:
        """The order the autograd Functions return gradients in."""
        ps = [self.w, self.b] + ([self.bn.weight, self.bn.bias] if self.bn is not None else [])
        return [p for p in ps if p is not None]

    @property
    def bias(self) -> torch.Tensor | None:
        return self.b.detach() if self.b is not None else None

    @property
    def stride(self) -> int:
        return 2 if self.kind == "s2" else 1

    def pack(self) -> None:
        """Refresh fwd / bwd from w, in place after the first call (descriptors and the
        batched-pack table hold their addresses)."""
        w = self.w.detach().float()
        if self.kind == "3x3":
            w = _pad_cin(w, self.cin_p)
            self.fwd = ops.pack_conv3x3(w, out=self.fwd)
            self.bwd = ops.pack_conv3x3_dgrad(_pad_cin(w, round_up(self.cin_p, 32)), scale=self.dgrad_scale,
                                              sub2=self.sub2, out=self.bwd)
        elif self.kind == "s2":
            self.fwd = ops.pack_conv3x3(expand_fwd(w), out=self.fwd)
            self.bwd = ops.pack_conv3x3(expand_dgrad(w), out=self.bwd)
        elif self.kind == "head":
            self.fwd = ops.pack_head9x9(w, out=self.fwd)
        else:  # tail: its input gradient is a head9x9 conv with 180°-rotated, transposed weights
            self.fwd = ops.pack_tail9x9(w, out=self.fwd)
            self.bwd = ops.pack_head9x9(w.flip(2, 3).transpose(0, 1).contiguous(), out=self.bwd)


def bn_forward_step(layer: TrainConv, z: ActBuffer, y: ActBuffer, **kw):
    """Train-mode BN of layer's conv output z into y (batch statistics, running update,
    num_batches_tracked); returns the descriptor."""
    d = ops.bn_desc(z, y, layer.cout, layer.bn_state, layer.bn, **kw)
    ops.bn_forward(d, layer.bn_state)
    if layer.bn.num_batches_tracked is not None:
        layer.bn.num_batches_tracked.add_(1)
    return d


def bn_backward_step(layer: TrainConv, z: ActBuffer, g: ActBuffer, dz: ActBuffer,
                     device) -> tuple[torch.Tensor, torch.Tensor]:
    """g (gradient wrt the BN output) → dz (wrt the conv output z); returns (dgamma, dbeta)."""
    dgamma = torch.empty(layer.cout, device=device)
    dbeta = torch.empty(layer.cout, device=device)
    ops.bn_backward(ops.bn_desc(z, g, layer.cout, layer.bn_state, layer.bn, dz=dz, dgamma=dgamma, dbeta=dbeta,
                                update_running=False), layer.bn_state)
    return dgamma, dbeta


class PlanLease:
    """Holds a plan (its saved activations) until the backward ran or the graph died."""

    def __init__(self, plan):
        self.plan = plan
        plan.busy = True

    def release(self):
        if self.plan is not None:
            self.plan.busy = False
            self.plan = None

    def __del__(self):
        self.release()
