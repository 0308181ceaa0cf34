"""The restatement of the dihedral transforms (include/isr.h) in torch on the CPU, for the tests: exactly
the expressions of the definition, nothing shared with the kernels.

op k = r + 4 f:  y = torch.rot90(x.flip(-1) if f else x, r, dims=(-2, -1))."""
import torch


def apply_ref(x: torch.Tensor, k) -> torch.Tensor:
    """Op k of [..., h, w]; `k` an int, or a sequence of per-image ids for a square batch [n, c, t, t]."""
    if not isinstance(k, int):
        return torch.stack([apply_ref(img, int(ki)) for img, ki in zip(x, k)])
    if not 0 <= k <= 7:
        raise ValueError(f"op {k} is not in 0..7")
    r, f = k % 4, k // 4
    return torch.rot90(x.flip(-1) if f else x, r, dims=(-2, -1)).contiguous()


def inverse_ref(k: int) -> int:
    return (4 - k) % 4 if k < 4 else k


def expand_ref(x: torch.Tensor):
    """(even [4n, c, h, w], odd [4n, c, w, h]): member k of image i at index (k // 2) * n + i."""
    even = torch.cat([apply_ref(x, k) for k in (0, 2, 4, 6)])
    odd = torch.cat([apply_ref(x, k) for k in (1, 3, 5, 7)])
    return even, odd


def members_ref(even: torch.Tensor, odd: torch.Tensor) -> list:
    """The eight member outputs in the order k = 0..7, each taken back by its inverse op: [n, c, h, w] each."""
    n = even.shape[0] // 4
    out = []
    for k in range(8):
        src = odd if k % 2 else even
        out.append(apply_ref(src[(k // 2) * n:(k // 2 + 1) * n], inverse_ref(k)))
    return out


def reduce_ref(even: torch.Tensor, odd: torch.Tensor, out_u8: bool = True) -> torch.Tensor:
    """fp32 members -> the average: seven sequential fp32 additions in the order k = 0..7, times 0.125; for
    uint8 the generator tail's quantisation, round half to even of (m + 1) / 2 * 255, clamped."""
    assert even.dtype == torch.float32 and odd.dtype == torch.float32
    m0, m1, m2, m3, m4, m5, m6, m7 = members_ref(even, odd)
    s = m0
    s = s + m1
    s = s + m2
    s = s + m3
    s = s + m4
    s = s + m5
    s = s + m6
    s = s + m7
    m = s * 0.125
    if not out_u8:
        return m
    return torch.round(((m + 1) / 2) * 255).clamp(0, 255).to(torch.uint8)


def _all_distinct(lines: torch.Tensor) -> bool:
    """lines [m, length]: no two equal."""
    return torch.unique(lines, dim=0).shape[0] == lines.shape[0]


def distinct_u8(n: int, c: int, h: int, w: int, seed: int) -> torch.Tensor:
    """Random uint8 [n, c, h, w] in which every plane has all rows distinct and all columns distinct, so that
    any row or column landing in the wrong place shows.  A plane of at most 256 pixels is a cut of a random
    permutation of 0..255 (all pixels distinct); a larger one is uniform noise, redrawn until it is so."""
    g = torch.Generator().manual_seed(seed)
    if h * w <= 256:
        x = torch.stack([torch.randperm(256, generator=g)[:h * w] for _ in range(n * c)])
        return x.view(n, c, h, w).to(torch.uint8)
    for _ in range(100):
        x = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.uint8)
        planes = x.view(n * c, h, w)
        if all(_all_distinct(p) and _all_distinct(p.t().contiguous()) for p in planes):
            return x
    raise AssertionError(f"no {h}x{w} plane with distinct rows and columns in 100 draws")
