"""PIL-exact resampling, the parts that need no GPU: the numpy restatement (tests/resample_ref.py)
against the installed Pillow, libisr's host-side coefficient tables (isr_resample_ksize /
isr_resample_tables) against the restatement as integers, the C ABI's refusals, and the table
builder as a stand-alone program under the address and undefined-behaviour sanitizers.

Zero differing values is the condition throughout: Pillow's 8-bit resampler is integer arithmetic
on coefficients rounded from doubles, and the restatement follows its order of operations."""
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import host_program
import resample_ref as R
from conftest import ROOT
from image_super_resolution_amd import _lib, data, degrade

PIL_FILTER = {"nearest": Image.NEAREST, "box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING,
              "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
SHAPES = [((96, 96), (24, 24)), ((96, 96), (32, 32)), ((96, 96), (48, 48)), ((48, 64), (12, 16)),
          ((50, 70), (17, 23)), ((24, 32), (96, 128)), ((33, 47), (66, 141)), ((37, 53), (37, 20)),
          ((64, 64), (64, 64))]
AXES = [(96, 24), (96, 32), (70, 23), (32, 128), (47, 141), (53, 53), (8, 1)]
UNSUPPORTED = -2


def images(h, w):
    """uint8 [3, h, w] test images by kind: noise, ramp, binary 0/255, step edge."""
    rng = np.random.default_rng(h * 1000 + w)
    ramp = np.stack([np.add.outer(np.arange(h) * a, np.arange(w) * b) % 256 for a, b in ((3, 2), (1, 5), (7, 1))])
    step = np.zeros((3, h, w), dtype=np.uint8)
    step[0, :, w // 2:] = 255
    step[1, h // 2:, :] = 255
    step[2, h // 3:, w // 3:] = 255
    return {"noise": rng.integers(0, 256, (3, h, w), dtype=np.uint8), "ramp": ramp.astype(np.uint8),
            "binary": (rng.integers(0, 2, (3, h, w)) * 255).astype(np.uint8), "step": step}


def pil_resize(img, size, name):
    """Image.resize of uint8 [3, h, w] as an RGB image to size = (h, w)."""
    im = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)))
    return np.asarray(im.resize((size[1], size[0]), PIL_FILTER[name])).transpose(2, 0, 1)


@pytest.mark.parametrize("name", R.FILTERS)
def test_restatement_equals_pillow(name):
    for (ih, iw), size in SHAPES:
        for kind, img in images(ih, iw).items():
            diff = int((R.resize(img, size, name) != pil_resize(img, size, name)).sum())
            assert diff == 0, f"{name} {kind} {ih}x{iw} -> {size}: {diff} values differ from Pillow"


def test_the_clip_is_exercised():
    """Sums below 0 and past 255 in both cases the kernel tests lean on, from the restatement's own
    unclipped accumulators (so the 0..255 clip decides pixels there)."""
    lo, hi = 0, 256 << R.PRECISION_BITS
    for name, kind, (ih, iw), size in (("bicubic", "step", (24, 32), (96, 128)),
                                       ("lanczos", "binary", (96, 96), (24, 24))):
        _, sx, sy = R.resize(images(ih, iw)[kind], size, name, return_sums=True)
        smin, smax = min(sx.min(), sy.min()), max(sx.max(), sy.max())
        print(f"{name} {kind} {ih}x{iw} -> {size}: sums in [{smin / (1 << 22):.2f}, {smax / (1 << 22):.2f}]")
        assert smin < lo and smax >= hi, (name, kind, smin, smax)


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


@pytest.mark.parametrize("name", R.FILTERS)
def test_c_tables_equal_the_restatement(lib, name):
    f = R.FILTERS.index(name)
    assert degrade.RESAMPLE_FILTERS == R.FILTERS
    for in_size, out_size in AXES:
        rb, rc = R.tables(name, in_size, out_size)
        assert lib.isr_resample_ksize(f, in_size, out_size) == rc.shape[1] == R.ksize(name, in_size, out_size)
        b, c = degrade.resample_tables(name, in_size, out_size)
        assert b.dtype == c.dtype == np.int32 and b.shape == rb.shape and c.shape == rc.shape
        assert np.array_equal(b, rb) and np.array_equal(c, rc), (name, in_size, out_size)
        assert np.array_equal(degrade.resample_tables(f, in_size, out_size)[1], rc)  # by index too


@pytest.mark.parametrize("name", R.FILTERS)
def test_c_tables_applied_with_numpy_equal_pillow(name):
    for (ih, iw), size in (((50, 70), (17, 23)), ((33, 47), (66, 141)), ((8, 8), (1, 1))):
        img = images(ih, iw)["noise"]
        got = R.apply_tables(img, degrade.resample_tables(name, iw, size[1]), degrade.resample_tables(name, ih, size[0]))
        assert np.array_equal(got, pil_resize(img, size, name)), (name, ih, iw, size)


def test_symbols_declared_and_exported(lib):
    header = (ROOT / "include" / "isr.h").read_text()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("isr_resample_ksize", "isr_resample_tables", "isr_resample_u8"):
        assert re.search(rf"\b{sym}\s*\(", header), sym
        assert re.search(rf"\bT {sym}\b", nm), sym
        assert sym in _lib.SIGNATURES
    for i, name in enumerate(R.FILTERS):
        assert re.search(rf"#define ISR_RESAMPLE_{name.upper()} {i}\b", header)


def _message(lib):
    return lib.isr_last_error().decode()


def test_table_refusals(lib):
    b = np.zeros((64, 2), dtype=np.int32)
    c = np.zeros((64, 49), dtype=np.int32)
    for what, (f, i, o) in {"filter": (6, 32, 8), "filter ": (-1, 32, 8), "ratio": (4, 9, 1), "ratio ": (4, 4, 36),
                            "sizes": (4, 0, 4), "sizes ": (4, 4, 0), "sizes  ": (4, 16385, 16385)}.items():
        assert lib.isr_resample_ksize(f, i, o) == 0 and what.strip() in _message(lib), (what, _message(lib))
        assert lib.isr_resample_tables(f, i, o, b.ctypes.data, c.ctypes.data) == UNSUPPORTED
        assert what.strip() in _message(lib), (what, _message(lib))
    assert lib.isr_resample_tables(4, 32, 8, None, c.ctypes.data) == -1
    assert lib.isr_resample_ksize(5, 16384, 2048) == 49  # the largest footprint: ISR_RESAMPLE_MAX_KSIZE
    with pytest.raises(ValueError):
        degrade.resample_tables("cubic", 32, 8)
    with pytest.raises(_lib.IsrError, match="ratio"):
        degrade.resample_tables("bicubic", 90, 10)


def test_cpu_device_keeps_cv2_and_refuses_the_rest():
    from oracle import ref_cpu
    crops = torch.randint(0, 256, (2, 3, 48, 48), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    for f in ("bicubic", "random"):
        tf = data.GPUTransform(4, lr_filter=f, device="cpu")
        with pytest.raises(RuntimeError, match="HIP"):
            tf(crops)
    with pytest.raises(ValueError):
        data.GPUTransform(4, lr_filter="cubic", device="cpu")
    with pytest.raises(RuntimeError):
        degrade.resample_u8(crops, (12, 12))
    hr, lr = data.GPUTransform(4, device="cpu")(crops)  # what it returned before lr_filter existed
    hr2, lr2 = data.GPUTransform(4, device="cpu", lr_filter="cv2", seed=5)(crops)
    assert torch.equal(hr, hr2) and torch.equal(lr, lr2)
    assert torch.equal(hr, crops.float().div(255.0) * 2.0 - 1.0)
    ref = R.normalize(ref_cpu.cv2_resize_linear_u8(crops.numpy(), 4), data.IMAGENET_MEAN, data.IMAGENET_STD)
    np.testing.assert_allclose(lr.numpy(), ref, rtol=0, atol=2e-6)


@pytest.mark.skipif(host_program.GXX is None, reason="needs g++")
def test_table_builder_standalone_under_sanitizers(lib, tmp_path):
    """csrc/resample_tables.h in a program of its own (tests/resample_tables_main.cpp), plain and with
    -fsanitize=address,undefined (tests/host_program.py): both run clean over the size list and the
    edges of what is supported, print the same sums, and those are the sums of the tables libisr
    hands to Python."""
    args = [str(v) for f in range(6) for io in AXES for v in (f, *io)]
    sweep, listed = host_program.run_plain_and_sanitized(ROOT / "tests" / "resample_tables_main.cpp", tmp_path,
                                                         runs=((), args))
    rows = [tuple(int(v) for v in line.split()) for line in (sweep + listed).splitlines()]
    assert len(rows) == 8 * 21 + 6 * len(AXES)
    assert {r[3] for r in rows} == {0, 1, 2, 3}  # accepted, and refused for each of the three reasons
    w = lambda a: int((a.astype(np.int64).ravel() * (np.arange(a.size) % 97 + 1)).sum())  # noqa: E731
    checked = 0
    for f, i, o, chk, ks, bsum, csum in rows:
        assert (lib.isr_resample_ksize(f, i, o) == ks) and (chk == 0) == (ks > 0)
        if chk == 0 and i * o <= 1 << 16:
            b, c = degrade.resample_tables(f, i, o)
            assert (w(b), w(c)) == (bsum, csum), (f, i, o)
            checked += 1
    assert checked >= 6 * len(AXES)


def test_train_flag_lr_filter(tmp_path, monkeypatch):
    """--lr_filter: cv2 when absent (and then not in the parsed namespace, which is what it was before
    the flag existed), any of GPUTransform.LR_FILTERS when given, refused with --train_denoise."""
    import train
    monkeypatch.chdir(tmp_path)
    opt = train.parse([])
    assert "lr_filter" not in vars(opt) and train.lr_filter_of(opt) == "cv2"
    for f in data.GPUTransform.LR_FILTERS:
        assert train.lr_filter_of(train.parse(["--lr_filter", f])) == f
    assert data.GPUTransform.LR_FILTERS == ("cv2", *degrade.RESAMPLE_FILTERS, "random")
    for bad in (["--lr_filter", "cubic"], ["--lr_filter", "bicubic", "--train_denoise"]):
        with pytest.raises(SystemExit):
            train.parse(bad)
    assert train.lr_filter_of(train.parse(["--lr_filter", "cv2", "--train_denoise"])) == "cv2"
