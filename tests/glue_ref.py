"""Plain torch restatements of the glue kernels' contracts in include/isr.h: isr_ew_combine,
isr_nchw_to_blocked / isr_blocked_to_nchw, isr_maxpool2_fwd / isr_maxpool2_bwd, the 3x3 weight pack
layout, and the three regions of an activation buffer that a launch may or may not write.  No HIP,
runs on any device.

Every function takes and returns NCHW fp32 tensors holding bf16-representable values, computes in
fp32 in the kernel's order of operations and rounds once to bf16 at the end (bf16r), so a kernel
whose products are exact (scales that are powers of two, or no scale) must match bit for bit.
`not (m > 0)` is the mask rule everywhere: +0.0 and -0.0 both take mslope."""
import torch


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """One round-to-nearest-even to bf16, kept in fp32."""
    return x.to(torch.bfloat16).float()


def round16(c: int) -> int:
    return (c + 15) // 16 * 16


def _masked(v: torch.Tensor, m: torch.Tensor, mslope: float) -> torch.Tensor:
    """v where m > 0, v * mslope elsewhere (fp32, on the unrounded v)."""
    return torch.where(m > 0, v, v * mslope)


def ew_combine(a, sa, b=None, sb=1.0, m=None, mslope=1.0):
    """isr_ew_combine: y = (a*sa + b*sb) * (m > 0 ? 1 : mslope); b, m optional."""
    v = a * sa
    if b is not None:
        v = v + b * sb
    if m is not None:
        v = _masked(v, m, mslope)
    return bf16r(v)


def nchw_to_blocked(x, scale=None, shift=None, m=None, mslope=1.0, c_pad=None):
    """isr_nchw_to_blocked: v = x*scale[c] + shift[c] (None: 1 / 0), then the mask; returns
    [n, c_pad, h, w] with channels [c, c_pad) zero (c_pad defaults to round16(c)).  m holds at
    least c channels; the first c are used."""
    n, c, h, w = x.shape
    c_pad = round16(c) if c_pad is None else c_pad
    v = x
    if scale is not None:
        v = v * scale.view(1, c, 1, 1)
    if shift is not None:
        v = v + shift.view(1, c, 1, 1)
    if m is not None:
        v = _masked(v, m[:, :c], mslope)
    out = torch.zeros(n, c_pad, h, w, dtype=torch.float32, device=x.device)
    out[:, :c] = bf16r(v)
    return out


def blocked_to_nchw(v, scale=None, shift=None):
    """isr_blocked_to_nchw: fp32 out = v*scale[c] + shift[c], no bf16 rounding."""
    c = v.shape[1]
    t = v.float()
    if scale is not None:
        t = t * scale.view(1, c, 1, 1)
    if shift is not None:
        t = t + shift.view(1, c, 1, 1)
    return t


def _windows(x):
    """The four 2x2 window positions q = 0..3 (row-major: q >> 1 the row, q & 1 the column) of every
    whole window, each [n, c, h//2, w//2]."""
    ho, wo = x.shape[2] // 2, x.shape[3] // 2
    return [x[:, :, (q >> 1):2 * ho:2, (q & 1):2 * wo:2] for q in range(4)]


def maxpool2_fwd(x):
    """isr_maxpool2_fwd: running best over q = 0..3 with a strict > (the max itself has no ties)."""
    win = _windows(x)
    best = win[0].clone()
    for q in range(1, 4):
        best = torch.where(win[q] > best, win[q], best)
    return bf16r(best)


def maxpool2_bwd(x, gy, mslope):
    """isr_maxpool2_bwd: gy goes to the FIRST maximum of each window (strict > against the running
    best, q in row-major order), times mslope where not (x > 0) there; every other position, and
    the rows / columns past 2*(h//2) / 2*(w//2), get 0."""
    win = _windows(x)
    best = win[0].clone()
    arg = torch.zeros(best.shape, dtype=torch.int64, device=x.device)
    for q in range(1, 4):
        better = win[q] > best
        best = torch.where(better, win[q], best)
        arg = torch.where(better, torch.full_like(arg, q), arg)
    ho, wo = best.shape[2], best.shape[3]
    g = torch.zeros_like(x, dtype=torch.float32)
    zero = torch.zeros_like(gy, dtype=torch.float32)
    for q in range(4):
        gk = torch.where(arg == q, gy.float(), zero)
        g[:, :, (q >> 1):2 * ho:2, (q & 1):2 * wo:2] = torch.where(win[q] > 0, gk, gk * mslope)
    return bf16r(g)


def pack_conv3x3(w, dgrad=False, scale=1.0, sub2=False):
    """The packed 3x3 weight layout (csrc/conv3x3.hip, isr_pack_conv3x3 / isr_pack_conv3x3_dgrad) as
    a flat bf16 tensor: out[c16][tap][n][hpos][e] = V[n][c16*16 + (hpos ^ ((n >> 3) & 1))*8 + e][tap]
    with V = w (forward) or, for dgrad, the conv cout -> cin of the layer w [cout, cin, 3, 3]:
    V[n][ci][tap] = scale * w[co(ci)][n][8 - tap], co = ci, or with sub2 co = 4c + s for
    ci = s*(cout/4) + c."""
    v = w.float()
    if dgrad:
        cout, cin = v.shape[:2]
        v = v.flip(2, 3).transpose(0, 1)  # [cin][cout][3][3]
        if sub2:
            v = v.reshape(cin, cout // 4, 4, 3, 3).transpose(1, 2)
        v = v.reshape(cin, cout, 3, 3) * scale
    pcout, pcin = v.shape[:2]
    v = v.reshape(pcout, pcin // 16, 2, 8, 9).permute(1, 4, 0, 2, 3)  # [c16][tap][n][h][e]
    n = torch.arange(pcout, device=v.device)
    h = torch.arange(2, device=v.device).view(1, 2) ^ ((n.view(pcout, 1) >> 3) & 1)  # [n][hpos] -> h
    idx = h.view(1, 1, pcout, 2, 1).expand(pcin // 16, 9, pcout, 2, 8)
    return torch.gather(v, 3, idx).contiguous().to(torch.bfloat16).flatten()


def regions(buf, coff, c):
    """Three boolean masks over buf.t ([n][cs/16][hp][wp][16]) for a launch that writes channels
    [coff, coff + round16(c)) of `buf` (coff a multiple of 16):
      (i)   the valid h x w interior of that channel slice,
      (ii)  its computed-but-invalid part: inside [pad, pad+ha) x [pad, pad+wa), outside h x w,
      (iii) everything else: the border ring, rows / columns past ha / wa, other channels.
    They are disjoint and cover the buffer."""
    assert coff % 16 == 0
    p0, p1 = coff // 16, (coff + round16(c)) // 16
    assert p1 <= buf.t.shape[1]
    p = buf.pad
    valid = torch.zeros(buf.t.shape, dtype=torch.bool, device=buf.t.device)
    computed = torch.zeros_like(valid)
    valid[:, p0:p1, p:p + buf.h, p:p + buf.w, :] = True
    computed[:, p0:p1, p:p + buf.ha, p:p + buf.wa, :] = True
    return valid, computed & ~valid, ~computed
