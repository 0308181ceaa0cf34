"""The premises of tests/test_gpu_tail_exact.py, on the CPU: the tail helpers of tests/exact_ref.py
against independent restatements, the input conditions of the bracket bar (pre-activations exact in
fp32 and on the 1/256 grid, at most 0.1 % of them past |s| = 4, a bracket at least 16 fp32 ulps wide
on either side, exact uint8 rounding ties present), that the bar passes a correct tanhf and fails an
output computed from a neighbouring grid point, and the tail dispatcher's rule restated in Python
against isr_tail9x9_segment_rows over a table of shapes and CU counts (made-up aligned pointers:
the entry point launches nothing and follows none; what it refuses: tests/test_capi_refusals.py)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
from image_super_resolution_amd import _lib

F64 = torch.float64
P = 0x10000  # aligned, never followed
DRAWS = [(2, 40, 72), (1, 27, 87), (3, 11, 23)]  # the first is the draw the bar's figures were taken on


def _draw(n, h, w, with_bias=True):
    """(x with its zero halo of 4, W, b, s) of one CPU draw."""
    g = X.gen(f"tail-cpu-{n}-{h}-{w}")
    xp = F.pad(X.acts((n, 64, h, w), g), (4, 4, 4, 4))
    W, b = X.tail_weights(g), X.tail_bias(g) if with_bias else None
    return xp, W, b, X.tail_preact(xp, W, b)


def test_tail_inputs_are_exact_in_both_storage_types():
    g = X.gen("tail-inputs")
    W, b, a = X.tail_weights(g), torch.cat([X.tail_bias(g) for _ in range(200)]), X.acts((4000,), g)
    for t in (W, a):
        assert torch.equal(t, t.to(torch.bfloat16).double()) and torch.equal(t, t.to(torch.float16).double())
    assert torch.equal(b, b.float().double())          # the bias stays fp32
    assert W.abs().max().item() == 2 / 256 and set((W * 256).flatten().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert b.abs().max().item() == 64 / 256 and X.granularity(b) == 1 / 256
    # the worst case the sum bound allows for: every |x| = 3, every |w| = 2/256, |bias| = 64/256
    x, Wm = torch.full((1, 64, 9, 9), 3.0, dtype=F64), torch.full((3, 64, 9, 9), 2 / 256, dtype=F64)
    worst = F.conv2d(x, Wm, None, padding=4).max().item() + 64 / 256
    assert worst == 31168 / 256 and worst < 2.0 ** 24 / 256
    X.assert_sum_bound(x, Wm, torch.full((3,), 0.25, dtype=F64), padding=4)


def test_tail_preact_vs_shifted_sums_and_a_strip_slice():
    xp, W, b, s = _draw(*DRAWS[2])
    n, _, hp, wp = xp.shape
    h, w = hp - 8, wp - 8
    ref = b.view(1, 3, 1, 1).expand(n, 3, h, w).clone()
    for ky in range(9):
        for kx in range(9):
            ref += torch.einsum("oc,nchw->nohw", W[:, :, ky, kx], xp[:, :, ky:ky + h, kx:kx + w])
    assert torch.equal(s, ref)
    # the columns [x0 - 4, x0 + 36) of the padded image give the strip at x0 alone
    xp, W, b, s = _draw(*DRAWS[0])
    for x0 in (0, 32, 64):
        part = X.tail_preact(xp[:, :, :, x0:x0 + 40], W, b)
        assert torch.equal(part[..., :min(32, 72 - x0)], s[..., x0:x0 + 32])


@pytest.mark.parametrize("n,h,w", DRAWS)
def test_tail_draw_meets_the_bars_conditions(n, h, w):
    xp, W, b, s = _draw(n, h, w)                       # asserts exactness, the grid and the sum bound
    far = (s.abs() > X.TAIL_SMAX).double().mean().item()
    room = X.tail_bracket_ulps(s)
    key = (s * 256).round()
    ties = int((key == 0).sum())
    print(f"tail draw {(n, h, w)}: std {s.std().item():.3f}, max |s| {s.abs().max().item():.3f}, "
          f"{torch.unique(key).numel()} distinct of {s.numel()}, far {far:.4%}, bracket >= {room.min().item():.1f} "
          f"ulps, s = 0 at {ties}")
    assert far <= X.TAIL_FAR_SHARE
    assert room.min().item() >= 16
    assert torch.unique(key).numel() >= min(500, s.numel() // 8)   # the outputs are no handful of values
    if s.numel() >= 10000:
        # s = 0 gives (tanh + 1) / 2 * 255 = 127.5 exactly: a real tie of the uint8 rounding
        assert ties >= 1
        t0 = torch.zeros(1)
        assert (((t0 + 1) / 2) * 255).item() == 127.5 and X.tail_u8_expected(t0).item() == 128


def test_bracket_is_wide_for_tanhf_and_narrow_for_a_neighbour():
    """Over the whole grid up to |s| = 4: the narrower side of the bracket is 43.85 fp32 ulps at |s| = 4
    and wider everywhere below, and the tanh of either neighbouring grid point lies outside the bracket,
    at every s."""
    s = torch.arange(-1024, 1025, dtype=F64) / 256
    room = X.tail_bracket_ulps(s)
    assert 43.8 <= room.min().item() == room[0].item() == room[-1].item()
    lo, hi = torch.tanh(s - X.TAIL_HSTEP), torch.tanh(s + X.TAIL_HSTEP)
    for step in (-1, 1):
        other = torch.tanh(s + step / 256).float().double()
        assert bool(((other <= lo) | (other >= hi)).all())


def test_check_tail_fp32_passes_tanhf_and_fails_what_it_should():
    xp, W, b, s = _draw(*DRAWS[0])
    good = torch.tanh(s.float())                       # a tanhf of the exact s
    seen = X.check_tail_fp32(good, s)
    print(f"CPU tanhf against float64: {seen}")
    assert seen["pixels"] == s.numel() and seen["zeros"] >= 1 and seen["tanhf_ulps"] <= 4
    i = (0, 1, 17, 40)
    for step in (-1, 1):                               # one pixel from the neighbouring grid point
        bad = good.clone()
        bad[i] = torch.tanh((s[i] + step / 256).float())
        with pytest.raises(AssertionError, match="outside their bracket"):
            X.check_tail_fp32(bad, s)
    bad = good.clone()                                 # one ulp off at one of two equal pre-activations
    key = (s * 256).round().flatten()
    vals, counts = torch.unique(key, return_counts=True)
    twin = int((key == vals[(counts >= 2) & (vals != 0)][0]).nonzero()[0])
    bad.view(-1)[twin] = torch.nextafter(bad.view(-1)[twin], torch.tensor(2.0))
    with pytest.raises(AssertionError, match="different output bits"):
        X.check_tail_fp32(bad, s)
    with pytest.raises(AssertionError, match="have \\|s\\| > "):     # too many saturated pixels
        X.check_tail_fp32(torch.tanh((s * 8).float()), s * 8)
    # past |s| = 4 only the sign and the magnitude are asked
    sf = torch.tensor([5.0, -6.0] + [0.0] * 4000, dtype=F64)
    X.check_tail_fp32(torch.tanh(sf.float()), sf)
    for wrong in ([-1.0, -1.0], [0.99, -1.0], [1.0, -1.0000001]):
        with pytest.raises(AssertionError, match="saturated"):
            X.check_tail_fp32(torch.tensor(wrong + [0.0] * 4000), sf)


def test_tail_u8_expected_rounds_half_to_even_in_fp32():
    t = torch.tensor([-1.0, 1.0, 0.0, -0.5, 0.5, 2.0 ** -7, -(2.0 ** -7)])
    # 0 -> 127.5 -> 128 (even); -0.5 -> 63.75 -> 64; 0.5 -> 191.25 -> 191; +-2^-7 -> 128.496.. / 126.503..
    assert X.tail_u8_expected(t).tolist() == [0, 255, 128, 64, 191, 128, 127]
    # a tie that must go DOWN to the even neighbour: (t + 1) / 2 * 255 = 126.5 needs t = -2 / 255, not an
    # fp32 number, so the store's only exact ties are those of s = 0; torch.round itself is half-even
    assert torch.round(torch.tensor([126.5, 127.5, 0.5, 254.5])).tolist() == [126.0, 128.0, 0.0, 254.0]


# ---------------------------------------------------------------- the dispatcher's rule
def _desc(n, h, w, u8, ha=None, wa=None, **kw):
    ha = -(-h // 32) * 32 if ha is None else ha
    wa = -(-w // 32) * 32 if wa is None else wa
    x = _lib.IsrView(P, ha + 8, wa + 8, 64, 4, 0)
    f = dict(n=n, h=h, w=w, ha=ha, wa=wa, cin=64, x=x, wpack=2 * P, bias=3 * P, y=4 * P, y_u8=int(u8), f16=0)
    f.update(kw)
    return _lib.IsrTailDesc(**f)


def _rule_rows():
    rows = []
    for cus in (64, 256, 304):
        # every height through tail_case (a GPU test's shapes), both outputs
        for sh in X.TAIL_SH:
            for m in (1, 3):
                for strips in (3, 9, 32):
                    try:
                        n, h, w = X.tail_case(sh, m, cus, strips)
                    except AssertionError:   # this strip count cannot give sh on this many CUs (sh 8, 16 only)
                        assert sh <= 16, (sh, m, cus, strips)
                        continue
                    rows += [(n, h, w, u8, cus, sh) for u8 in (False, True)]
        # one block short of filling the CUs at 64 rows, and exactly filling them
        n64 = -(-cus // 3)
        rows += [(n64, 192, 32, False, cus, 64), (n64 - 1, 192, 32, False, cus, 32)]
        # ha % sh decides: 96 = 3 * 32 rows with blocks to spare never walks 64; 544 = 17 * 32 never above 32
        rows += [(cus, 96, 32, False, cus, 32), (cus, 544, 32, True, cus, 32), (cus, 1024, 64, False, cus, 512)]
        # the shapes of the older tail tests
        rows += [(n, h, w, u8, cus, None) for (n, h, w) in [(2, 40, 72), (5, 128, 160), (3, 96, 64), (2, 300, 96)]
                 for u8 in (False, True)]
    # the fp32 2 GiB boundary: 3 * h * w * 4 = 2^31 at h * w = 2^29 / 3 (not an integer); with w = 16384,
    # h = 10922 is the last height under it and 10923 the first over; the same pixels as uint8 walk
    w = 16384
    assert 3 * 10922 * w * 4 < 2 ** 31 <= 3 * 10923 * w * 4
    rows += [(1, 10922, w, False, 256, 64), (1, 10923, w, False, 256, 0), (1, 10923, w, True, 256, 64),
             (4, 10923, w, False, 64, 0), (1, 16384, 32768, True, 256, 512), (1, 16384, 65536, True, 256, 0)]
    # exactly 2^31 bytes: 3 * h * w = 2^31 has no solution, 3 * h * w * 4 = 2^31 neither; one over in uint8
    rows += [(1, 21846, 32768, True, 256, 0), (1, 21845, 32768, True, 256, None)]
    return rows


def test_segment_rows_entry_point_vs_the_restated_rule(built_lib):
    lib = built_lib
    rows = _rule_rows()
    missed, seen = [], set()
    for n, h, w, u8, cus, want in rows:
        rule = X.tail_segment_rule(n, h, w, u8, cus)
        got = lib.isr_tail9x9_segment_rows(ctypes.byref(_desc(n, h, w, u8)), cus)
        seen.add((cus, got))
        if got != rule or (want is not None and got != want):
            missed.append((n, h, w, u8, cus, f"library {got}, rule {rule}, table {want}"))
    assert not missed, "\n".join(map(str, missed))
    for cus in (64, 256, 304):
        assert {sh for c, sh in seen if c == cus} >= set(X.TAIL_SH), (cus, sorted(seen))
    assert (256, 0) in seen and (64, 0) in seen


def test_segment_rows_answers_a_height_not_a_code(built_lib):
    lib = built_lib
    assert lib.isr_tail9x9_segment_rows(ctypes.byref(_desc(2, 40, 72, False)), 256) == 8
    assert math.log2(lib.isr_tail9x9_segment_rows(ctypes.byref(_desc(16, 512, 512, False)), 256)) == 9
