"""The blur family, the parts that need no GPU: libisr's host-side tap builder (isr_blur_taps)
against the numpy restatement (tests/blur_ref.py) as integers, the tables' properties, the
restatement against scipy (linear filters; the derived bound) and against Pillow and scipy (median;
zero differences), the table builder as a stand-alone program under the address and
undefined-behaviour sanitizers, the C ABI's layout and refusals, LRDegrade's refusals on a CPU
device and its host draws, and train.py's --lr_degrade flag."""
import ctypes
import math
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter
from scipy import ndimage

import blur_ref as B
import host_program
from conftest import ROOT
from image_super_resolution_amd import _lib, data, degrade

GAUSSIANS = [(3, 0.8, 0.8, 0.0), (5, 1.1, 1.1, 0.0), (7, 3.0, 0.6, 0.7), (7, 1.4, 1.4, 0.0), (7, 10.0, 10.0, 0.0)]
# (k, x1, y1, x2, y2): one line per octant (steep and shallow, all four sign pairs), horizontal,
# vertical, both diagonals, a 2-pixel line
MOTIONS = [(7, 0, 2, 6, 4), (7, 2, 0, 4, 6), (7, 6, 2, 0, 4), (7, 4, 0, 2, 6), (7, 0, 4, 6, 2), (7, 2, 6, 4, 0),
           (7, 6, 4, 0, 2), (7, 4, 6, 2, 0), (5, 0, 2, 4, 2), (5, 4, 2, 0, 2), (5, 2, 0, 2, 4), (7, 3, 6, 3, 0),
           (7, 0, 0, 6, 6), (7, 6, 0, 0, 6), (5, 4, 4, 0, 0), (3, 1, 1, 2, 1), (5, 2, 2, 2, 3), (7, 0, 0, 1, 0),
           (7, 0, 1, 6, 3), (7, 1, 0, 5, 1), (3, 0, 0, 2, 1)]


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def gauss_kw(sx, sy, a):
    return dict(sigma_x=sx, sigma_y=sy, angle=a)


def all_tables():
    out = [(("box", k), degrade.blur_taps("box", k), B.taps("box", k)) for k in (3, 5, 7)]
    for k, sx, sy, a in GAUSSIANS:
        out.append((("gaussian", k, sx, sy, a), degrade.blur_taps("gaussian", k, **gauss_kw(sx, sy, a)),
                    B.taps("gaussian", k, **gauss_kw(sx, sy, a))))
    for k in (3, 5, 7):  # sigma 0 and an absent sigma: cv2's rule for the ksize
        out.append((("gaussian", k, 0), degrade.blur_taps("gaussian", k, sigma_x=0, sigma_y=0),
                    B.taps("gaussian", k, sigma_x=B.cv2_sigma(k), sigma_y=B.cv2_sigma(k))))
        out.append((("gaussian", k, None), degrade.blur_taps("gaussian", k), B.taps("gaussian", k)))
    for k, x1, y1, x2, y2 in MOTIONS:
        kw = dict(x1=x1, y1=y1, x2=x2, y2=y2)
        out.append((("motion", k, x1, y1, x2, y2), degrade.blur_taps("motion", k, **kw), B.taps("motion", k, **kw)))
    return out


def test_tap_builder_equals_the_restatement():
    for what, got, want in all_tables():
        assert got.dtype == np.int32 and got.shape == (7, 7)
        assert np.array_equal(got, want), (what, got - want)
    assert np.array_equal(degrade.blur_taps(0, 5), B.taps("box", 5))  # the kind as ISR_BLUR_*


def test_motion_lines_are_the_stated_bresenham():
    assert B.bresenham(0, 0, 6, 2) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 2), (6, 2)]
    for k, x1, y1, x2, y2 in MOTIONS:
        line = B.bresenham(x1, y1, x2, y2)
        assert line[0] == (x1, y1) and line[-1] == (x2, y2) and len(line) == max(abs(x2 - x1), abs(y2 - y1)) + 1
        t = degrade.blur_taps("motion", k, x1=x1, y1=y1, x2=x2, y2=y2)
        o, c = (7 - k) // 2, 3
        on = {(x + o, y + o) for x, y in line}
        for y in range(7):
            for x in range(7):
                if (x, y) in on and (x, y) != (c, c):
                    assert t[y, x] == math.floor(65536.0 / len(line) + 0.5), (k, x1, y1, x2, y2, x, y)
                elif (x, y) != (c, c):
                    assert t[y, x] == 0
        if (c, c) not in on:  # the centre holds the rounding residual alone
            assert 0 <= t[c, c] <= 3


def test_table_properties():
    for what, got, _ in all_tables():
        assert int(got.astype(np.int64).sum()) == 65536 and int(got.min()) >= 0, what
        k = what[1]
        o = (7 - k) // 2
        inside = np.zeros((7, 7), dtype=bool)
        inside[o:o + k, o:o + k] = True
        assert not got[~inside].any(), what
        isotropic = what[0] == "box" or (what[0] == "gaussian" and (len(what) == 3 or (what[2] == what[3] and what[4] == 0)))
        if isotropic:
            for m in (got.T, got[::-1], got[:, ::-1], got[::-1, ::-1], got.T[::-1], got.T[:, ::-1], got.T[::-1, ::-1]):
                assert np.array_equal(got, m), what


def test_builder_refusals():
    lib = _lib.load()
    buf = np.zeros(49, dtype=np.int32)
    par = (ctypes.c_double * 4)(0, 0, 1, 1)
    for kind, k, msg in ((3, 3, b"unknown kind"), (-1, 3, b"unknown kind"), (0, 4, b"ksize"), (0, 9, b"ksize"),
                         (1, 1, b"ksize")):
        assert lib.isr_blur_taps(kind, k, ctypes.cast(par, ctypes.c_void_p), buf.ctypes.data) == -2
        assert msg in lib.isr_last_error(), lib.isr_last_error()
    assert lib.isr_blur_taps(0, 3, None, None) == -1 and b"null" in lib.isr_last_error()
    assert lib.isr_blur_taps(2, 3, None, buf.ctypes.data) == -1 and b"params" in lib.isr_last_error()
    assert lib.isr_blur_taps(0, 3, None, buf.ctypes.data) == 0  # box needs no params
    for kw, msg in ((dict(x1=1, y1=1, x2=1, y2=1), "equal"), (dict(x1=0, y1=0, x2=3, y2=0), "integers in"),
                    (dict(x1=-1, y1=0, x2=2, y2=0), "integers in"), (dict(x1=0.5, y1=0, x2=2, y2=0), "integers in")):
        with pytest.raises(_lib.IsrError, match=msg):
            degrade.blur_taps("motion", 3, **kw)
    # six pixels that miss the centre: the taps would sum to 65538, the centre would be -2
    with pytest.raises(_lib.IsrError, match="centre tap"):
        degrade.blur_taps("motion", 7, x1=0, y1=0, x2=5, y2=0)
    with pytest.raises(ValueError):
        B.taps("motion", 7, x1=0, y1=0, x2=5, y2=0)
    with pytest.raises(_lib.IsrError, match="finite"):
        degrade.blur_taps("gaussian", 3, sigma_x=float("nan"), sigma_y=1.0)
    with pytest.raises(ValueError):
        degrade.blur_taps("gauss", 3)
    with pytest.raises(ValueError):
        degrade.blur_taps("box", 3, sigma_x=1.0)
    with pytest.raises(ValueError):
        degrade.blur_taps("motion", 3, x1=0, y1=0)


@pytest.mark.skipif(host_program.GXX is None, reason="needs g++")
def test_tap_builder_standalone_under_sanitizers(tmp_path):
    """csrc/blur_taps.h in a program of its own (tests/blur_taps_main.cpp), plain and with
    -fsanitize=address,undefined (tests/host_program.py): both run clean over every kind, ksize and
    refusal, print the same lines, and those are the tables libisr hands to Python (sum and
    position-weighted sum)."""
    (out,) = host_program.run_plain_and_sanitized(ROOT / "tests" / "blur_taps_main.cpp", tmp_path,
                                                  extra_flags=("-ffp-contract=off",))
    rows = [line.split() for line in out.splitlines()]
    assert {int(r[6]) for r in rows} == {0, 1, 2, 3, 4, 5, 6}  # made, and refused for each of the six reasons
    weights = np.arange(1, 50, dtype=np.int64)
    checked = 0
    for kind, k, p0, p1, p2, p3, code, total, wsum in rows:
        if int(code) != 0:
            continue
        assert int(total) == 65536
        kw = {} if kind == "0" else (gauss_kw(float(p0), float(p1), float(p2)) if kind == "1" else
                                     dict(x1=float(p0), y1=float(p1), x2=float(p2), y2=float(p3)))
        t = degrade.blur_taps(int(kind), int(k), **kw)
        assert int((t.astype(np.int64).ravel() * weights).sum()) == int(wsum), (kind, k, p0, p1, p2, p3)
        checked += 1
    assert checked > 1000


def images(h, w, seed=0):
    rng = np.random.default_rng(seed + 1000 * h + w)
    step = np.zeros((h, w), dtype=np.uint8)
    step[h // 3:, w // 2:] = 255
    ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5) % 256).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (h, w), dtype=np.uint8), (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8),
                     step, ramp])


def test_linear_restatement_against_scipy():
    """floor(correlate(float64, w, mode='mirror') + 0.5) against the integer filter: they differ by at
    most 1, and only where the exact value lies within 0.19 of a half-integer.  The bound: 48 taps off
    by at most half a unit of 2^-16 each and the centre by at most 24.5 units, (48 * 0.5 + 24.5) /
    65536 * 255 = 0.189 of a value."""
    bound = (48 * 0.5 + 24.5) / 65536 * 255
    assert bound < 0.19
    for k, sx, sy, a in GAUSSIANS:
        w = B.normalized("gaussian", k, **gauss_kw(sx, sy, a))
        table = B.taps("gaussian", k, **gauss_kw(sx, sy, a))
        o = (7 - k) // 2
        assert np.abs(table[o:o + k, o:o + k] - w * 65536).sum() <= 48 * 0.5 + 24.5
        for h, wd in ((7, 7), (9, 13), (33, 70)):
            img = images(h, wd)
            exact = np.stack([ndimage.correlate(p.astype(np.float64), w, mode="mirror") for p in img])
            want = np.floor(exact + 0.5)
            got = B.filter_u8(img, table, k).astype(np.float64)
            assert np.abs(B.filter_sums(img, table, k) / 65536.0 - exact).max() <= bound
            diff = got != want
            assert np.abs(got - want).max() <= 1, (k, sx, sy, a, h, wd)
            frac = np.abs(exact - np.floor(exact) - 0.5)
            assert not diff.any() or frac[diff].max() <= 0.19, (k, sx, sy, a, h, wd, frac[diff].max())
            # the 7 x 7 window with the zero taps gives the same pixels
            assert np.array_equal(B.filter_u8(img, table, 7), got.astype(np.uint8))


@pytest.mark.parametrize("k", [3, 5, 7])
def test_median_restatement_equals_pillow_and_scipy(k):
    for h, w in ((7, 7), (9, 13), (33, 70)):
        img = images(h, w, seed=k)
        got = B.median_u8(img, k)
        sp = np.stack([ndimage.median_filter(p, size=k, mode="nearest") for p in img])
        pil = np.stack([np.asarray(Image.fromarray(p).filter(ImageFilter.MedianFilter(k))) for p in img])
        assert int((got != sp).sum()) == 0, (k, h, w)
        assert int((got != pil).sum()) == 0, (k, h, w)


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "isr.h"
#define F(m) printf(#m " %zu\n", offsetof(isr_blur_desc, m))
int main(void) {
  printf("size %zu\n", sizeof(isr_blur_desc));
  F(n); F(h); F(w); F(src); F(dst); F(ksize); F(median); F(taps);
  printf("consts %d %d %d %d %d\n", ISR_BLUR_MAX_K, ISR_BLUR_BITS, ISR_BLUR_BOX, ISR_BLUR_GAUSSIAN, ISR_BLUR_MOTION);
  return 0;
}
"""


def test_desc_layout_matches_c(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                   check=True)
    lines = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines()
    c = {ln.split()[0]: ln.split()[1:] for ln in lines}
    assert int(c["size"][0]) == ctypes.sizeof(_lib.IsrBlurDesc)
    assert [name for name, _ in _lib.IsrBlurDesc._fields_] == ["n", "h", "w", "src", "dst", "ksize", "median", "taps"]
    for name, _ in _lib.IsrBlurDesc._fields_:
        assert getattr(_lib.IsrBlurDesc, name).offset == int(c[name][0]), name
    assert [int(v) for v in c["consts"]] == [B.MAX_K, B.BITS, 0, 1, 2]
    assert degrade.BLUR_KINDS == B.KINDS and degrade.BLUR_MAX_K == B.MAX_K


def test_cpu_tensors_are_refused():
    crops = torch.randint(0, 256, (2, 3, 48, 48), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    for call in (lambda: degrade.filter_u8(crops, B.taps("box", 3)), lambda: degrade.median_u8(crops, 3),
                 lambda: degrade.blur_u8(crops, 3, 0, B.taps("box", 3))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(RuntimeError, match="HIP"):
        data.LRDegrade(blur_p=1.0, device="cpu")(crops)
    with pytest.raises(RuntimeError, match="HIP"):
        data.LRDegrade.preset("blind", device="cpu")(crops)
    with pytest.raises(RuntimeError, match="HIP"):
        data.GPUTransform(4, device="cpu", degrade=data.LRDegrade(blur_p=1.0, device="cpu"))(crops)
    with pytest.raises(ValueError, match="40x40.*16|16.*40x40"):
        data.LRDegrade(jpeg_p=0.5, device="cpu")(crops[..., :40, :40])
    with pytest.raises(ValueError):
        data.LRDegrade(blur_kinds=("gauss",), device="cpu")
    with pytest.raises(ValueError):
        data.LRDegrade(blur_p=1.5, device="cpu")
    # without `degrade` the CPU transform is what it was
    hr, lr = data.GPUTransform(4, device="cpu")(crops)
    hr2, lr2 = data.GPUTransform(4, device="cpu", degrade=None)(crops)
    assert torch.equal(hr, hr2) and torch.equal(lr, lr2)


def test_host_draws_are_reproducible_and_in_range():
    n = 256
    a = data.LRDegrade.blur_params(n, 0.5, data.LRDegrade.BLUR_KINDS, torch.Generator().manual_seed(11))
    b = data.LRDegrade.blur_params(n, 0.5, data.LRDegrade.BLUR_KINDS, torch.Generator().manual_seed(11))
    assert a == b
    assert {r["kind"] for r in a} == set(data.LRDegrade.BLUR_KINDS) and {r["ksize"] for r in a} == {3, 5, 7}
    assert 0.3 < sum(r["apply"] for r in a) / n < 0.7
    refused = 0
    for r in a:
        k, p = r["ksize"], r["params"]
        if r["kind"] == "gaussian":
            assert 0.2 <= p["sigma_x"] <= 3.0 and 0.2 <= p["sigma_y"] <= 3.0 and 0.0 <= p["angle"] < math.pi
            assert np.array_equal(degrade.blur_taps("gaussian", k, **p), B.taps("gaussian", k, **p))
        elif r["kind"] == "motion":
            assert all(0 <= p[v] <= k - 1 for v in p) and (p["x1"], p["y1"]) != (p["x2"], p["y2"])
            try:
                want = B.taps("motion", k, **p)
            except ValueError:  # the six-pixel line that misses the centre: both refuse it
                refused += 1
                with pytest.raises(_lib.IsrError):
                    degrade.blur_taps("motion", k, **p)
                continue
            assert np.array_equal(degrade.blur_taps("motion", k, **p), want)
    assert refused < n // 16


def test_train_flag_lr_degrade(tmp_path, monkeypatch, capsys):
    """--lr_degrade: absent from the parsed namespace when not given (a run without it parses to what
    it did before), blur / blind when given, refused with --train_denoise in a message naming both."""
    import train
    monkeypatch.chdir(tmp_path)
    opt = train.parse([])
    assert "lr_degrade" not in vars(opt) and train.lr_degrade_of(opt, "cpu", 0) is None
    for name in ("blur", "blind"):
        d = train.lr_degrade_of(train.parse(["--lr_degrade", name, "--lr_filter", "bicubic"]), "cpu", 5)
        assert isinstance(d, data.LRDegrade) and d.seed == 5
    assert (d.iso_p, d.jpeg_p, d.jpeg_quality, d.blur_p, d.gauss_p) == (0.05, 0.1, (45, 75), 0.3, 0.1)
    b = data.LRDegrade.preset("blur", device="cpu")
    assert (b.iso_p, b.jpeg_p, b.blur_p, b.gauss_p) == (0.0, 0.0, 0.5, 0.0)
    with pytest.raises(SystemExit) as e:
        train.parse(["--lr_degrade", "blind", "--train_denoise"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--lr_degrade" in err and "--train_denoise" in err
    with pytest.raises(SystemExit):
        train.parse(["--lr_degrade", "sharpen"])
