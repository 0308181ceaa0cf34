"""The 9x9 tail forward (conv2 + tanh, csrc/conv9x9.hip) at every segment height of its walk, against
a float64 CPU reference (tests/exact_ref.py; the premises are checked in tests/test_tail_exact_cpu.py).

The production kernel walks down 32-column strips in segments of sh rows, sh in {8, ..., 512} chosen by
the dispatcher from the shape and the device's CU count.  At sh = 8 the walk makes two iterations, its O
ring never wraps and its steady state (iteration 3 on) never runs, so every case here first PROVES its
sh through isr_tail9x9_segment_rows, and the cases cover all seven heights (shapes from
exact_ref.tail_case and the CU count of the device).

Data: activations are integers in [-3, 3], weights k/256 (|k| <= 2), the bias k/256 (|k| <= 64), drawn
on the device; the pre-activation s is then exact in fp32 in any summation order and lies on the 1/256
grid.  Per case:
  1. sentinel: the output is a view inside a larger sentinel-filled allocation and prefilled itself;
     every element is overwritten (fp32: no 7.0 survives a tanh; uint8: two runs over different fills
     agree with the expected image) and 1024 guard elements on either side stay intact;
  2. variants 5 (twice), 3 and 0 are bit-identical over the whole tensor, in both output types;
  3. fp32: on the referenced strips (everywhere at sh = 8; else the whole height of the first strip of
     image 0 and of the partial last strip of the last image) each output lies strictly inside
     (tanh64(s - 1/512), tanh64(s + 1/512)) and is a function of s (exact_ref.check_tail_fp32).
     Variant 3 runs one code on every 8-row tile, so with (2) the referenced strips pin every pixel;
  4. uint8: the whole image equals clamp(round_half_even((t + 1) / 2 * 255), 0, 255) computed in
     fp32 on the CPU from the kernel's own fp32 output t.
Running the per-tile fallback of outputs past 2 GiB is out of scope (23 GB of activations); the
dispatcher's boundary is in the CPU table."""
import ctypes
import time
import zlib
from dataclasses import dataclass

import pytest
import torch

import exact_ref as X
from exact_ref import BF, FP

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1024
FILL = {torch.float32: (7.0, 7.0), torch.uint8: (7, 200)}   # the two runs of variant 5 start from these


@dataclass(frozen=True)
class Case:
    sh: int
    m: int            # ha = m * max(sh, 32)
    strips: int       # w = 32 * strips - 9
    dt: torch.dtype
    bias: bool = True

    @property
    def name(self):
        return f"sh{self.sh}-m{self.m}-{self.strips}strips-{str(self.dt).replace('torch.', '')}" + \
            ("" if self.bias else "-nobias")


CASES = [
    Case(8, 1, 3, BF), Case(8, 1, 3, FP),
    Case(16, 3, 9, BF), Case(16, 3, 9, FP),
    Case(32, 1, 7, BF, bias=False),
    Case(64, 3, 5, BF), Case(64, 3, 5, FP),
    Case(128, 3, 3, BF),
    Case(256, 1, 16, BF), Case(256, 1, 16, FP),
    Case(512, 1, 32, BF),
]


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def cu_count() -> int:
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def test_cases_cover_the_walk():
    """What the list must hold on this device: all seven heights, three or more segments (an interior one,
    its halo T rows from both neighbours' rows) at 16 and 64, more than one image, a partial last strip,
    h < ha with h % 16 != 0, a block count that is no multiple of 8 (xcd_remap's tail), both storage
    types, a case without bias."""
    cus = cu_count()
    shapes = {c: X.tail_case(c.sh, c.m, cus, c.strips) for c in CASES}
    assert {c.sh for c in CASES} == set(X.TAIL_SH)
    for sh in (16, 64):
        assert any(c.sh == sh and c.m * max(sh, 32) // sh >= 3 for c in CASES)
    blocks = {c: n * c.strips * (c.m * max(c.sh, 32) // c.sh) for c, (n, h, w) in shapes.items()}
    assert any(b % 8 for b in blocks.values()), blocks
    for c, (n, h, w) in shapes.items():
        assert n > 1 and w % 32 and h % 16 and h < c.m * max(c.sh, 32)
    assert {c.dt for c in CASES} == {BF, FP} and any(not c.bias for c in CASES)


def build(c: Case):
    """The case's activation buffer, weights and bias, drawn on the device (seeded by the case's name)."""
    from image_super_resolution_amd import ops
    n, h, w = X.tail_case(c.sh, c.m, cu_count(), c.strips)
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(c.name.encode()))
    buf = ops.ActBuffer.alloc(n, h, w, 64, 4, DEV, dtype=c.dt)
    for i in range(n):  # image by image: the int8 draw and its conversion never hold more than one image
        x = torch.randint(-3, 4, (4, 16, h, w), generator=g, device=DEV, dtype=torch.int8)
        buf.t[i, :, 4:4 + h, 4:4 + w, :] = x.permute(0, 2, 3, 1).to(c.dt)
    W = torch.randint(-2, 3, (3, 64, 9, 9), generator=g, device=DEV).float() / X.TAIL_GRID
    b = torch.randint(-64, 65, (3,), generator=g, device=DEV).float() / X.TAIL_GRID if c.bias else None
    return (n, h, w), buf, W, b, ops.pack_tail9x9(W, f16=c.dt == FP)


def strip_preact(buf, img, x0, W64, b64):
    """float64 s of the strip [x0, x0 + 32) of image img over the full height, from the columns
    [x0 - 4, x0 + 36) of the buffer the kernel reads (rows and columns of its zero border included)."""
    xs = buf.t[img, :, :buf.h + 8, x0:x0 + 40, :].cpu()             # [4, h + 8, 40, 16]
    xs = xs.permute(0, 3, 1, 2).reshape(1, 64, buf.h + 8, 40).double()
    return X.tail_preact(xs, W64, b64)[0, :, :, :min(32, buf.w - x0)]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_tail9x9_exact(c, lib):
    from image_super_resolution_amd import ops
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()      # what earlier tests of the session keep alive is not this case's
    (n, h, w), buf, W, b, wp = build(c)
    numel = n * 3 * h * w

    def run(variant, dt, fill):
        big = torch.full((numel + 2 * GUARD,), fill, device=DEV, dtype=dt)
        out = big[GUARD:GUARD + numel].view(n, 3, h, w)
        d = ops.tail9x9_desc(buf, wp, b, out)
        assert ops.tail9x9_segment_rows(d) == c.sh, (c.name, (n, h, w), ops.tail9x9_segment_rows(d))
        ops.check(lib.isr_tail9x9_fwd_variant(ctypes.byref(d), variant, ops._stream()), f"tail variant {variant}")
        torch.cuda.synchronize()
        assert bool((big[:GUARD] == fill).all()) and bool((big[-GUARD:] == fill).all()), \
            f"{c.name}: variant {variant} wrote outside its {dt} output"
        return out

    def runs(dt):
        """Variant 5 twice (from two fills), 3 and 0: bit-identical; returns the first."""
        a = run(5, dt, FILL[dt][0])
        key = a.view(torch.int32) if dt == torch.float32 else a
        for variant, fill in ((5, FILL[dt][1]), (3, FILL[dt][0]), (0, FILL[dt][1])):
            o = run(variant, dt, fill)
            o = o.view(torch.int32) if dt == torch.float32 else o
            assert torch.equal(o, key), f"{c.name}: variant {variant} differs from the walk in {dt}"
        return a

    a = runs(torch.float32)
    assert bool((a.abs() <= 1).all()), f"{c.name}: an fp32 output kept its sentinel (or left [-1, 1])"
    t1 = time.perf_counter()

    # the referenced strips
    W64, b64 = W.cpu().double(), None if b is None else b.cpu().double()
    last = 32 * (c.strips - 1)
    where = [(i, x0) for i in range(n) for x0 in range(0, w, 32)] if c.sh == 8 else [(0, 0), (n - 1, last)]
    s = torch.cat([strip_preact(buf, i, x0, W64, b64).flatten() for i, x0 in where])
    got = torch.cat([a[i, :, :, x0:x0 + 32].cpu().flatten() for i, x0 in where])
    seen = X.check_tail_fp32(got, s, c.name)
    t2 = time.perf_counter()

    # uint8: the store path, from the kernel's own fp32 output
    want = X.tail_u8_expected(a.cpu())
    u = runs(torch.uint8)
    diff = u != want.to(DEV)
    assert not bool(diff.any()), f"{c.name}: {int(diff.sum())} of {numel} uint8 pixels differ from the fp32 output's image"
    ties = int((a == 0).sum())
    peak = torch.cuda.max_memory_allocated() - held
    t3 = time.perf_counter()
    print(f"\n{c.name}: {(n, h, w)}, {len(where)} strips referenced, {seen}, outputs at exactly 0 (127.5 ties): "
          f"{ties}, peak {peak / 2 ** 20:.0f} MiB, build + fp32 runs {t1 - t0:.2f} s, reference {t2 - t1:.2f} s, "
          f"uint8 {t3 - t2:.2f} s")
    assert peak < 2 ** 31
