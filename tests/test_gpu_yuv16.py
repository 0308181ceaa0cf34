"""10-bit YUV 4:2:0 video I/O on the GPU (csrc/yuv16.hip; yuv.py, video.py, rs.py): the two colour kernels
equal the numpy restatement (tests/yuv16_ref.py) bit for bit over every (matrix, range, siting, layout,
shift) and RGB kind on the smallest shapes that reach each path and edge, on extremes (the int32
overflow of the limited-range inverse), at unaligned addresses and on the float kinds' special values;
FrameUpscaler with a 10-bit side equals restatement -> eager plan -> restatement; an 8-bit source gives
consistent 8- and 10-bit output; 10-bit .y4m files stream through VideoUpscaler and rs.py."""
import itertools

import numpy as np
import pytest
import torch

import yuv16_ref as R
import yuv_ref as Y
from image_super_resolution_amd import engine, models, tiler, video, yuv
from image_super_resolution_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOP = 1023

# (matrix, full range, siting, layout, shift): p010le is (nv12, 6) and yuv420p10le (i420, 0); the entry
# points take the other two pairings as well
COMBOS = list(itertools.product(("bt601", "bt709"), (False, True), ("left", "center"), ("i420", "nv12"), (0, 6)))
# (h, w, batch): the smallest frames; (18, 34) the element path with w crossing a 32-column boundary; (2, 16)
# and (4, 32) whole 16-column segments, the 16-byte path of every plane; (6, 8), (10, 24), (24, 40) a ragged
# last segment beside whole ones; (6, 48) x 2 whole segments over several rows and the frame stride
SHAPES = [(2, 2, 1), (2, 4, 1), (4, 2, 1), (6, 10, 1), (18, 34, 1), (2, 16, 1), (6, 8, 1), (4, 32, 1), (10, 24, 1),
          (24, 40, 3), (6, 48, 2)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
INV_STD = np.array(yuv.inv_std_of(STD), dtype=np.float32)  # what the descriptor holds


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def desc_call(fn_name, n, h, w, combo, kind, src, dst, mean=MEAN, std=STD):
    """One launch through yuv._desc16 with the combo's own shift (YUVFormat ties the shift to the layout)."""
    import ctypes
    from image_super_resolution_amd import _lib
    m, fr, s, lay, shift = combo
    d = yuv._desc16(n, h, w, yuv.YUVFormat(lay, m, fr, s, 10), kind, src.data_ptr(), dst.data_ptr(), mean, std)
    d.shift = shift
    _lib.check(getattr(_lib.load(), fn_name)(ctypes.byref(d), yuv._stream()), fn_name)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_rgb(frames, h, w, combo, kind="u16", out=None, n=None):
    n = n or frames.shape[0]
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.int16 if kind == "u16" else torch.float32, device=DEV)
    desc_call("isr_yuv420_to_rgb_16", n, h, w, combo, kind, frames if torch.is_tensor(frames) else dev(frames), out)
    got = out.cpu().numpy()
    return got.view(np.uint16) if kind == "u16" else got


def to_yuv(rgb, combo, out=None):
    """rgb: uint16 [n, 3, h, w] or fp32 (tanh), numpy or device tensor -> uint8 [n, 3 h w]"""
    if not torch.is_tensor(rgb):
        rgb = dev(rgb.view(np.int16) if rgb.dtype == np.uint16 else rgb)
    n, _, h, w = rgb.shape
    if out is None:
        out = torch.empty((n, 3 * h * w), dtype=torch.uint8, device=DEV)
    desc_call("isr_rgb_to_yuv420_16", n, h, w, combo, "tanh_f32" if rgb.dtype == torch.float32 else "u16", rgb, out)
    return out.cpu().numpy().reshape(n, -1)


def random_frames(rng, n, h, w, layout, shift):
    """Random 10-bit samples with random stray bits outside the sample field of every word."""
    planes = [rng.integers(0, 1024, (n, h >> (i > 0), w >> (i > 0))) for i in range(3)]
    stray = rng.integers(0, 65536, (n, 3 * h * w // 2)).astype(np.uint16)
    return R.pack(*planes, layout, shift, stray=stray)


def check_to_yuv(got, rgb, combo, what):
    m, fr, s, lay, shift = combo
    want = R.rgb_to_yuv420(rgb, m, fr, s, lay, shift)
    assert got.shape == want.shape and np.array_equal(got, want), (what, combo, int((got != want).sum()))
    words = got.view("<u2")
    assert not (words & ~np.uint16(TOP << shift)).any(), (what, combo)  # p010: the low 6 bits are 0


@pytest.mark.parametrize("h,w,n", SHAPES)
def test_kernels_equal_the_restatement(h, w, n):
    rng = np.random.default_rng(100 * h + w)
    rgb = rng.integers(0, 1024, (n, 3, h, w)).astype(np.uint16)
    t = rng.uniform(-1.1, 1.1, (n, 3, h, w)).astype(np.float32)
    for combo in COMBOS:
        m, fr, s, lay, shift = combo
        check_to_yuv(to_yuv(rgb, combo), rgb, combo, "u16")
        check_to_yuv(to_yuv(t, combo), R.quantise(t), combo, "tanh")
        frames = random_frames(rng, n, h, w, lay, shift)
        want = R.yuv420_to_rgb(frames, h, w, m, fr, s, lay, shift)
        got = to_rgb(frames, h, w, combo)
        assert got.shape == want.shape and np.array_equal(got, want), (combo, int((got != want).sum()))
        got = to_rgb(frames, h, w, combo, "norm_f32")
        want = R.normalise(want, MEAN, INV_STD)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), combo


def test_python_entry_points():
    """yuv.yuv420_to_rgb / rgb_to_yuv420 dispatch on the format's depth: shapes, dtypes and values."""
    h, w, n = 6, 16, 2
    rng = np.random.default_rng(8)
    for name in ("yuv420p10le", "p010le"):
        fmt = yuv.YUVFormat.of_pix_fmt(name, matrix="bt709", siting="center")
        args = ("bt709", False, "center", fmt.layout, fmt.shift)
        frames = random_frames(rng, n, h, w, fmt.layout, fmt.shift)
        want = R.yuv420_to_rgb(frames, h, w, *args)
        got = yuv.yuv420_to_rgb(dev(frames.reshape(n, 3 * h // 2, 2 * w)), h, w, fmt)
        assert got.dtype == torch.int16 and tuple(got.shape) == (n, 3, h, w) and np.array_equal(got.cpu().numpy(), want.view(np.int16))
        got = yuv.yuv420_to_rgb(dev(frames), h, w, fmt, normalize=(MEAN, STD))
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), R.normalise(want, MEAN, INV_STD))
        rgb = rng.integers(0, 1024, (n, 3, h, w)).astype(np.uint16)
        got = yuv.rgb_to_yuv420(dev(rgb.view(np.int16)), fmt)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 3 * h // 2, 2 * w)
        assert np.array_equal(got.cpu().numpy().reshape(n, -1), R.rgb_to_yuv420(rgb, *args))
        t = rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float32)
        assert np.array_equal(yuv.rgb_to_yuv420(dev(t), fmt).cpu().numpy().reshape(n, -1), R.rgb_to_yuv420(R.quantise(t), *args))
    f10 = yuv.YUVFormat(depth=10)
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(torch.zeros(90, dtype=torch.uint8, device=DEV), 6, 10, f10)  # an 8-bit frame's bytes
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv420(torch.zeros((1, 3, 6, 10), dtype=torch.uint8, device=DEV), f10)
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(torch.zeros(90, dtype=torch.uint8, device=DEV), 6, 10, normalize=(MEAN, STD))


@pytest.mark.parametrize("h,w", [(6, 10), (4, 32)])
def test_kernels_on_extremes(h, w):
    """Planes of 0 and 1023 in every combination: the clamps of both directions run, and the limited-range
    center-sited inverse passes int32 (tests/test_yuv16_cpu.py::test_overflow_premise)."""
    ends = np.array(list(itertools.product((0, TOP), repeat=3)), dtype=np.uint16)  # [8, 3]
    rgb = np.ascontiguousarray(np.broadcast_to(ends[:, :, None, None], (8, 3, h, w)))
    for combo in COMBOS:
        m, fr, s, lay, shift = combo
        planes = [np.broadcast_to(ends[:, i, None, None].astype(np.int64), (8, h >> (i > 0), w >> (i > 0))) for i in range(3)]
        frames = R.pack(*planes, lay, shift)
        peak = []
        want = R.yuv420_to_rgb(frames, h, w, m, fr, s, lay, shift, peak=peak)
        assert want.min() == 0 and want.max() == TOP
        if (m, fr, s) == ("bt709", False, "center"):
            assert peak[0] > 2 ** 31 - 1
        assert np.array_equal(to_rgb(frames, h, w, combo), want), combo
        assert np.array_equal(to_rgb(frames, h, w, combo, "norm_f32"), R.normalise(want, MEAN, INV_STD)), combo
        check_to_yuv(to_yuv(rgb, combo), rgb, combo, "extremes")


def test_kernels_at_unaligned_addresses():
    """w % 16 == 0 at addresses that are only 2-byte (fp32: 4-byte) aligned: each plane falls back to element
    accesses on its own, and nothing outside the output is written (sentinel-filled buffers)."""
    h, w, n = 6, 32, 2
    rng = np.random.default_rng(5)
    fb, rb = R.frame_bytes(h, w), 2 * 3 * h * w
    SENT = 0xA5
    combos = COMBOS[:4] + COMBOS[-4:]
    for off_f, off_r in ((2, 0), (6, 0), (8, 0), (14, 0), (0, 2), (0, 6), (0, 8), (0, 14), (8, 8), (2, 14)):
        fbuf = torch.full((n * fb + 32,), SENT, dtype=torch.uint8, device=DEV)
        rbuf = torch.full((n * rb + 32,), SENT, dtype=torch.uint8, device=DEV)
        fview = fbuf[off_f:off_f + n * fb]
        rview = rbuf[off_r:off_r + n * rb].view(torch.int16).view(n, 3, h, w)
        assert fview.data_ptr() % 16 == off_f and rview.data_ptr() % 16 == off_r
        for combo in combos:
            m, fr, s, lay, shift = combo
            frames = random_frames(rng, n, h, w, lay, shift)
            rgb = rng.integers(0, 1024, (n, 3, h, w)).astype(np.uint16)
            fview.copy_(dev(frames.ravel()))
            rview.fill_(-1)
            got = to_rgb(fview, h, w, combo, out=rview, n=n)
            assert np.array_equal(got, R.yuv420_to_rgb(frames, h, w, m, fr, s, lay, shift)), (combo, off_f, off_r)
            rview.copy_(dev(rgb.view(np.int16)))
            fview.fill_(SENT)
            check_to_yuv(to_yuv(rview, combo, out=fview), rgb, combo, (off_f, off_r))
            for buf, off, size in ((fbuf, off_f, n * fb), (rbuf, off_r, n * rb)):
                guard = torch.cat([buf[:off], buf[off + size:]])
                assert bool((guard == SENT).all()), (combo, off_f, off_r)
    # the fp32 kinds: 4-byte aligned RGB
    for off_f, off_r in ((0, 4), (2, 8), (8, 12)):
        fbuf = torch.full((n * fb + 32,), SENT, dtype=torch.uint8, device=DEV)
        rbuf = torch.full((2 * n * rb + 32,), SENT, dtype=torch.uint8, device=DEV)
        fview = fbuf[off_f:off_f + n * fb]
        rview = rbuf[off_r:off_r + 2 * n * rb].view(torch.float32).view(n, 3, h, w)
        for combo in combos:
            m, fr, s, lay, shift = combo
            frames = random_frames(rng, n, h, w, lay, shift)
            fview.copy_(dev(frames.ravel()))
            got = to_rgb(fview, h, w, combo, "norm_f32", out=rview, n=n)
            want = R.normalise(R.yuv420_to_rgb(frames, h, w, m, fr, s, lay, shift), MEAN, INV_STD)
            assert np.array_equal(got, want), (combo, off_f, off_r)
            t = rng.uniform(-1.1, 1.1, (n, 3, h, w)).astype(np.float32)
            rview.copy_(dev(t))
            fview.fill_(SENT)
            check_to_yuv(to_yuv(rview, combo, out=fview), R.quantise(t), combo, (off_f, off_r))
            for buf, off, size in ((fbuf, off_f, n * fb), (rbuf, off_r, 2 * n * rb)):
                guard = torch.cat([buf[:off], buf[off + size:]])
                assert bool((guard == SENT).all()), (combo, off_f, off_r)
    # an odd address is refused
    from image_super_resolution_amd import _lib
    odd = torch.zeros(n * fb + 1, dtype=torch.uint8, device=DEV)[1:]
    with pytest.raises(_lib.IsrError, match="aligned"):
        to_rgb(odd, h, w, COMBOS[0], n=n)
    with pytest.raises(_lib.IsrError, match="aligned"):
        to_yuv(torch.zeros((n, 3, h, w), dtype=torch.int16, device=DEV), COMBOS[0], out=odd)


def test_float_kinds_on_special_values():
    """TANH input on the quantiser's special values (tests/yuv16_ref.py), laid out as an image."""
    t = R.special_tanh_values()
    h, w = 36, 40
    t = np.resize(t, (1, 3, h, w)).astype(np.float32)
    assert 3 * h * w >= len(R.special_tanh_values()) and np.isnan(t).any() and np.isinf(t).any()
    for combo in (COMBOS[0], COMBOS[-1], ("bt709", False, "center", "i420", 0), ("bt601", True, "left", "nv12", 6)):
        check_to_yuv(to_yuv(t, combo), R.quantise(t), combo, "special")
    # NORM with another mean / std: the descriptor's fp32 reciprocal
    mean, std = (0.5, 0.25, 0.0), (0.5, 0.3, 1.0)
    frames = random_frames(np.random.default_rng(1), 1, 6, 16, "i420", 0)
    got = torch.empty((1, 3, 6, 16), dtype=torch.float32, device=DEV)
    desc_call("isr_yuv420_to_rgb_16", 1, 6, 16, COMBOS[0], "norm_f32", dev(frames), got, mean, std)
    want = R.normalise(R.yuv420_to_rgb(frames, 6, 16, "bt601", False, "left"), mean, np.array(yuv.inv_std_of(std), np.float32))
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------- the video path
H, W, B = 24, 40, 2


@pytest.fixture(scope="module")
def net():
    """The 2-block synthetic net of test_gpu_yuv.py: (state_dict, eager runner)."""
    g = models.ResNet(2, 0.2, scaleRate=2)
    sd = synth_state_dict(g.state_dict(), 11)
    g.load_state_dict(sd)
    m = models.Model(g.eval())
    m.init_normalize(MEAN, STD)
    return sd, tiler.runner_for(m.fuse().eval().to(DEV), DEV)


def source_rgb(n, seed=4):
    return np.stack(list(video.SyntheticVideo(W, H, n, seed=seed))).transpose(0, 3, 1, 2)  # uint8 [n, 3, H, W]


def source_frames(n, fmt, seed=4):
    """4:2:0 frames of `fmt` of a smooth moving picture; 10-bit ones carry detail below the 8-bit step."""
    rgb = source_rgb(n, seed)
    if fmt.depth == 8:
        return Y.rgb_to_yuv420(rgb, "bt601", False, "left", fmt.layout)
    rgb10 = rgb.astype(np.int64) * 4 + np.random.default_rng(seed).integers(0, 4, rgb.shape)
    return R.rgb_to_yuv420(rgb10, "bt601", False, "left", fmt.layout, fmt.shift)


def ref_in(frames, fmt, mean=MEAN, std=STD):
    """Frames (or uint8 RGB [n, 3, h, w] with fmt None) -> what the plan is fed: uint8 RGB, or at depth 10
    the normalised fp32 image."""
    if fmt is None:
        return frames
    args = (fmt.matrix, fmt.full_range, fmt.siting, fmt.layout)
    if fmt.depth == 8:
        return Y.yuv420_to_rgb(frames, H, W, *args)
    return R.normalise(R.yuv420_to_rgb(frames, H, W, *args, fmt.shift), mean, np.array(yuv.inv_std_of(std), np.float32))


def ref_out(out, fmt):
    """The plan's output (uint8 RGB, or fp32 tanh) -> frames of fmt (None: BGR HWC)."""
    if fmt is None:
        return out[:, ::-1].transpose(0, 2, 3, 1)
    args = (fmt.matrix, fmt.full_range, fmt.siting, fmt.layout)
    if fmt.depth == 8:
        return Y.rgb_to_yuv420(out, *args)
    return R.rgb_to_yuv420(R.quantise(out), *args, fmt.shift)


def expect(gw, x, fmt_in, fmt_out, mean=MEAN, std=STD, cache={}):
    """restatement -> eager engine.make_plan(..., x_u8, out_u8, ...) -> restatement"""
    x_u8 = fmt_in is None or fmt_in.depth == 8
    out_u8 = fmt_out is None or fmt_out.depth == 8
    n = x.shape[0]
    key = (id(gw), n, x_u8, out_u8, tuple(mean), tuple(std))
    if key not in cache:
        cache[key] = (gw, engine.make_plan(gw, n, H, W, torch.device(DEV), x_u8, out_u8, mean, std))
    plan = cache[key][1]
    out = torch.empty(plan.out_shape, dtype=plan.out_dtype, device=DEV)
    plan.run(dev(ref_in(x, fmt_in, mean, std)), out)
    torch.cuda.synchronize()
    return ref_out(out.cpu().numpy(), fmt_out)


MODES = [("yuv420p10le", "yuv420p10le"), ("p010le", "p010le"), ("yuv420p", "yuv420p10le"), ("yuv420p10le", "bgr24"),
         ("rgb24", "p010le")]


@torch.no_grad()
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("pix_in,pix_out", MODES)
def test_frame_upscaler_10_bit_modes(net, pix_in, pix_out, graph):
    _, runner = net
    up = video.FrameUpscaler(runner.gw, H, W, B, MEAN, STD, DEV, graph=graph, pix_fmt_in=pix_in, pix_fmt_out=pix_out)
    shapes = {"rgb24": (H, W, 3), "yuv420p": (36, 40), "yuv420p10le": (36, 80), "p010le": (36, 80)}
    out_shapes = {"bgr24": (2 * H, 2 * W, 3), "yuv420p10le": (72, 160), "p010le": (72, 160)}
    assert up.in_frame_shape == shapes[pix_in] and up.out_frame_shape == out_shapes[pix_out]
    assert (up.graph is not None) == graph
    assert up.x.dtype == (torch.float32 if "10" in pix_in else torch.uint8)
    assert up.y.dtype == (torch.float32 if "10" in pix_out else torch.uint8)
    for n, seed in ((B, 4), (1, 9)):  # a full batch, then a ragged one through the same graph
        if pix_in == "rgb24":
            x = source_rgb(n, seed)
            fed = x.transpose(0, 2, 3, 1)
        else:
            assert up.yuv_in == yuv.YUVFormat.of_pix_fmt(pix_in, matrix="bt601")
            x = source_frames(n, up.yuv_in, seed)
            fed = x.reshape(n, *up.in_frame_shape)
        got = up(torch.from_numpy(np.ascontiguousarray(fed))).cpu().numpy()
        want = expect(runner.gw, x, up.yuv_in, up.yuv_out)
        assert got.shape == (n, *up.out_frame_shape)
        assert np.array_equal(got.reshape(n, -1), np.ascontiguousarray(want).reshape(n, -1)), (pix_in, pix_out, graph, n)
    with pytest.raises(ValueError):
        up(torch.zeros((B, 5, 5), dtype=torch.uint8))


@torch.no_grad()
def test_8_and_10_bit_output_agree(net):
    """The same 8-bit limited-range input through the 8-bit and the 10-bit output path: |Y10 - 4 Y8| <= 5
    (tests/test_yuv16_cpu.py::test_consistency_derivation_on_one_value), and the 10-bit luma uses the
    two bits the 8-bit one does not have."""
    _, runner = net
    frames = source_frames(B, yuv.YUVFormat())
    fed = torch.from_numpy(frames.reshape(B, 36, 40))
    kw = dict(graph=False, pix_fmt_in="yuv420p")
    y8 = video.FrameUpscaler(runner.gw, H, W, B, MEAN, STD, DEV, pix_fmt_out="yuv420p", **kw)(fed).cpu().numpy()
    y10 = video.FrameUpscaler(runner.gw, H, W, B, MEAN, STD, DEV, pix_fmt_out="yuv420p10le", **kw)(fed).cpu().numpy()
    luma8 = y8.reshape(B, -1)[:, :4 * H * W].astype(int)
    luma10 = np.ascontiguousarray(y10).reshape(B, -1).view("<u2")[:, :4 * H * W].astype(int)
    diff = np.abs(luma10 - 4 * luma8)
    print("max |Y10 - 4 Y8|", diff.max())
    assert diff.max() <= 5
    assert set(np.unique(luma10 % 4)) == {0, 1, 2, 3}


def write_y4m(path, frames, header):
    path.write_bytes(header + b"".join(b"FRAME\n" + f.tobytes() for f in frames))


def read_y4m(path, n, fb):
    head, _, body = path.read_bytes().partition(b"\n")
    assert len(body) == n * (fb + 6)
    out = []
    for i in range(n):
        rec = body[i * (fb + 6):(i + 1) * (fb + 6)]
        assert rec[:6] == b"FRAME\n"
        out.append(np.frombuffer(rec[6:], np.uint8))
    return head + b"\n", np.stack(out)


@torch.no_grad()
def test_10_bit_y4m_end_to_end(net, tmp_path):
    """A C420p10 file through VideoUpscaler (batches of 2, 2 and 1) and through rs.py; rs.py --out_depth 10
    on an 8-bit file writes a C420p10 file."""
    import rs
    sd, runner = net
    f10 = yuv.YUVFormat("i420", "bt601", True, "left", 10)
    frames = source_frames(5, f10)
    write_y4m(tmp_path / "in.y4m", frames, b"YUV4MPEG2 W40 H24 F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n")
    src = video.open_video(tmp_path / "in.y4m")
    assert src.yuv == yuv.YUVFormat("i420", "auto", True, "left", 10) and len(src) == 5 and src.pix_fmt == "yuv420p10le"
    up = video.FrameUpscaler(runner.gw, H, W, B, MEAN, STD, DEV, pix_fmt_in=src.pix_fmt, pix_fmt_out=src.pix_fmt,
                             yuv_in=src.yuv, yuv_out=src.yuv)
    rec = video.Y4MRecorder(tmp_path / "out.y4m", (2 * W, 2 * H), src.fps, up.yuv_out)
    assert video.VideoUpscaler(up).run(src, rec) == 5
    rec.stopRecorder()
    head, out = read_y4m(tmp_path / "out.y4m", 5, R.frame_bytes(2 * H, 2 * W))
    assert head == b"YUV4MPEG2 W80 H48 F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n"
    back = video.Y4MReader(tmp_path / "out.y4m")
    assert (back.width, back.height, back.yuv, len(back)) == (80, 48, src.yuv, 5)
    want = np.concatenate([expect(runner.gw, frames[i:i + 2], f10, f10) for i in (0, 2, 4)])
    assert np.array_equal(out, want)
    # rs.py, 10 -> 10
    torch.save(sd, tmp_path / "net.pt")
    args = ["--model", str(tmp_path / "net.pt"), "--src", str(tmp_path / "in.y4m"), "--batch_size", "2"]
    rs.runer(**vars(rs.build_parser().parse_args(args + ["--save_dir", str(tmp_path / "rs.y4m")])))
    head2, out2 = read_y4m(tmp_path / "rs.y4m", 5, R.frame_bytes(2 * H, 2 * W))
    # rs.py builds its own runner from the file and normalises by that runner's mean and std, which are the
    # model's fp32 constants (tiler.runner_for), not the doubles above: the reference does the same
    r2 = tiler.runner_for(rs.build_model(str(tmp_path / "net.pt"), 0.2, MEAN, STD), DEV)
    assert r2.mean != MEAN and np.allclose(r2.mean, MEAN)
    want2 = np.concatenate([expect(r2.gw, frames[i:i + 2], f10, f10, r2.mean, r2.std) for i in (0, 2, 4)])
    assert head2 == head and np.array_equal(out2, want2)
    # rs.py, an 8-bit center-sited file written at 10 bits: C420p10, left-sited
    f8 = yuv.YUVFormat("i420", "bt601", False, "center")
    frames8 = source_frames(3, f8)
    write_y4m(tmp_path / "in8.y4m", frames8, b"YUV4MPEG2 W40 H24 F30:1 Ip C420jpeg\n")
    rs.runer(**vars(rs.build_parser().parse_args(["--model", str(tmp_path / "net.pt"), "--src", str(tmp_path / "in8.y4m"),
                                                  "--save_dir", str(tmp_path / "rs10.y4m"), "--batch_size", "2",
                                                  "--out_depth", "10"])))
    head3, out3 = read_y4m(tmp_path / "rs10.y4m", 3, R.frame_bytes(2 * H, 2 * W))
    assert head3 == b"YUV4MPEG2 W80 H48 F30:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED\n"
    fo = yuv.YUVFormat("i420", "bt601", False, "left", 10)
    want3 = np.concatenate([expect(r2.gw, frames8[i:i + 2], f8, fo, r2.mean, r2.std) for i in (0, 2)])
    assert np.array_equal(out3, want3)
    torch.cuda.synchronize()
