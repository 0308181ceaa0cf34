"""CPU restatement of the fp16 Winograd F(2,3) 3x3 conv of isr_conv3x3_wino_fwd (include/isr.h).

Per kernel row ky, input channel c and output pair j (outputs x = 2j, 2j+1; inputs
d0..d3 = x[2j-1 .. 2j+2]; taps g0..g2 = W[co][c][ky][0..2]):

    V0 = d0 - d2   V1 = d1 + d2   V2 = d2 - d1   V3 = d1 - d3     (each rounded once to fp16)
    U0 = g0   U1 = (g0+g1+g2)/2   U2 = (g0-g1+g2)/2   U3 = g2     (fp32, rounded once to fp16)
    M_p = sum_{ky,c} U_p V_p                                      (fp64 here; fp32 on the GPU)
    y(2j) = M0 + M1 + M2       y(2j+1) = M1 - M2 - M3

then v = act(y + bias); v = v*s1 + r1; v = v*s2 + r2, rounded once to fp16.  With both fp16
roundings switched off (`round_uv=False, round_out=False`) this is the plain conv in fp64, which
pins the transform matrices independently of any kernel (tests/test_wino_cpu.py).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def wino_u(W: torch.Tensor, round_uv: bool = True) -> torch.Tensor:
    """Transformed weights U[p][cout][cin][ky] of W [cout, cin, 3, 3]: fp16 (computed in fp32 from
    the fp32 weights in the pack kernel's order, rounded once) or, unrounded, fp64."""
    W = W.detach().cpu()
    g = W.float() if round_uv else W.double()
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
    U = torch.stack([g0, ((g0 + g1) + g2) * 0.5, ((g0 - g1) + g2) * 0.5, g2])
    return U.half() if round_uv else U


def wino_ref(x: torch.Tensor, W: torch.Tensor, bias: torch.Tensor | None = None, *, slope: float = 1.0,
             r1: torch.Tensor | None = None, s1: float = 1.0, r2: torch.Tensor | None = None, s2: float = 1.0,
             round_uv: bool = True, round_out: bool = True) -> torch.Tensor:
    """x [n, cin, h, w] (the values the kernel reads: fp16-representable when round_uv), W fp32
    [cout, cin, 3, 3] → [n, cout, h, w] fp64 (through one fp16 rounding when round_out)."""
    x = x.detach().cpu()
    n, cin, h, w = x.shape
    # the descriptor carries slope / s1 / s2 as fp32
    slope, s1, s2 = (float(torch.tensor(v, dtype=torch.float32)) for v in (slope, s1, s2))
    J = (w + 1) // 2
    # xp column i is x column i - 1; pairs need columns 2j .. 2j+3
    xp = F.pad(x.double(), (1, 2 * J - w + 1, 1, 1))
    d = [xp[..., k:k + 2 * J:2] for k in range(4)]
    V = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    if round_uv:
        # a sum of two fp16 values rounded to fp32 and then to fp16 is correctly rounded (24 >= 2*11 + 2)
        V = [v.float().half() for v in V]
    U = wino_u(W, round_uv)
    M = [F.conv2d(V[p].double(), U[p].double().unsqueeze(-1)) for p in range(4)]  # (3, 1) kernel over (ky, j)
    y = torch.stack([(M[0] + M[1]) + M[2], (M[1] - M[2]) - M[3]], dim=-1).reshape(n, -1, h, 2 * J)[..., :w]
    if bias is not None:
        y = y + bias.detach().cpu().double().view(1, -1, 1, 1)
    y = torch.where(y >= 0, y, y * slope)
    if r1 is not None:
        y = y * s1 + r1.detach().cpu().double()
    if r2 is not None:
        y = y * s2 + r2.detach().cpu().double()
    elif s2 != 1.0:
        y = y * s2
    return y.float().half().double() if round_out else y
