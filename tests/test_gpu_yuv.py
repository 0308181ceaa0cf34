"""YUV 4:2:0 video I/O on the GPU (csrc/yuv.hip; yuv.py, video.py, rs.py): the two colour kernels
equal the numpy restatement (tests/yuv_ref.py) bit for bit over every (matrix, range, siting, layout)
on the smallest shapes that reach each path and edge; FrameUpscaler in 4:2:0 mode equals
restatement -> eager runner -> restatement, and is unchanged by default; a .y4m file streams through
VideoUpscaler into a .y4m file, and through rs.py."""
import itertools

import numpy as np
import pytest
import torch

import yuv_ref as Y
from image_super_resolution_amd import models, tiler, video, yuv
from image_super_resolution_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

COMBOS = list(itertools.product(("bt601", "bt709"), (False, True), ("left", "center"), ("i420", "nv12")))
# (h, w, batch): the smallest frames; (18, 34) the byte path with w crossing a 32-column boundary; (2, 32) and
# (6, 16) 16-byte luma with 8-byte chroma rows and a V plane that is only 8-byte aligned; (4, 64) and (10, 48)
# whole segments over several rows; (24, 80) x 3 the frame stride
SHAPES = [(2, 2, 1), (2, 4, 1), (4, 2, 1), (6, 10, 1), (18, 34, 1), (2, 32, 1), (6, 16, 1), (4, 64, 1), (10, 48, 1),
          (24, 80, 3)]


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def fmt_of(m, fr, s, lay):
    return yuv.YUVFormat(lay, m, fr, s)


def to_rgb(frames, h, w, combo):
    m, fr, s, lay = combo
    return yuv.yuv420_to_rgb(torch.from_numpy(frames).to(DEV), h, w, fmt_of(*combo)).cpu().numpy()


def to_yuv(rgb, combo):
    n = rgb.shape[0]
    return yuv.rgb_to_yuv420(torch.from_numpy(rgb).to(DEV), fmt_of(*combo)).cpu().numpy().reshape(n, -1)


@pytest.mark.parametrize("h,w,n", SHAPES)
def test_kernels_equal_the_restatement(h, w, n):
    rng = np.random.default_rng(100 * h + w)
    rgb = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    frames = rng.integers(0, 256, (n, Y.frame_bytes(h, w)), dtype=np.uint8)
    for combo in COMBOS:
        m, fr, s, lay = combo
        got = to_yuv(rgb, combo)
        want = Y.rgb_to_yuv420(rgb, m, fr, s, lay)
        assert got.shape == want.shape and np.array_equal(got, want), (combo, int((got != want).sum()))
        got = to_rgb(frames, h, w, combo)
        want = Y.yuv420_to_rgb(frames, h, w, m, fr, s, lay)
        assert got.shape == want.shape and np.array_equal(got, want), (combo, int((got != want).sum()))


@pytest.mark.parametrize("h,w", [(6, 10), (4, 64)])
def test_kernels_on_extremes(h, w):
    """Planes of 0 and 255 in every combination: the clamps of both directions run."""
    ends = np.array(list(itertools.product((0, 255), repeat=3)), dtype=np.uint8)  # [8, 3]
    rgb = np.ascontiguousarray(np.broadcast_to(ends[:, :, None, None], (8, 3, h, w)))
    q = h * w // 4
    for combo in COMBOS:
        m, fr, s, lay = combo
        planes = [np.full((8, k), 0, dtype=np.uint8) + ends[:, i:i + 1] for i, k in enumerate((h * w, q, q))]
        frames = Y.pack(planes[0].reshape(8, h, w), planes[1].reshape(8, h // 2, w // 2),
                        planes[2].reshape(8, h // 2, w // 2), lay)
        want = Y.yuv420_to_rgb(frames, h, w, m, fr, s, lay)
        assert want.min() == 0 and want.max() == 255
        assert np.array_equal(to_rgb(frames, h, w, combo), want), combo
        assert np.array_equal(to_yuv(rgb, combo), Y.rgb_to_yuv420(rgb, m, fr, s, lay)), combo


def test_kernels_at_unaligned_addresses():
    """w % 16 == 0 at addresses that are not: each plane falls back to bytes on its own."""
    h, w, n = 6, 32, 2
    rng = np.random.default_rng(5)
    fb = Y.frame_bytes(h, w)
    for off_frames, off_rgb in ((1, 0), (8, 0), (0, 3), (8, 8)):
        fbuf = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
        rbuf = torch.zeros(n * 3 * h * w + 16, dtype=torch.uint8, device=DEV)
        frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
        rgb = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
        for combo in COMBOS[:4] + COMBOS[-4:]:
            m, fr, s, lay = combo
            fview = fbuf[off_frames:off_frames + n * fb]
            rview = rbuf[off_rgb:off_rgb + n * 3 * h * w].view(n, 3, h, w)
            fview.copy_(torch.from_numpy(frames.ravel()))
            got = yuv.yuv420_to_rgb(fview, h, w, fmt_of(*combo), out=rview).cpu().numpy()
            assert np.array_equal(got, Y.yuv420_to_rgb(frames, h, w, m, fr, s, lay)), (combo, off_frames, off_rgb)
            rview.copy_(torch.from_numpy(rgb))
            got = yuv.rgb_to_yuv420(rview, fmt_of(*combo), out=fview).cpu().numpy().reshape(n, -1)
            assert np.array_equal(got, Y.rgb_to_yuv420(rgb, m, fr, s, lay)), (combo, off_frames, off_rgb)
            assert int(fbuf[:off_frames].sum()) == 0 and int(fbuf[off_frames + n * fb:].sum()) == 0
            assert int(rbuf[:off_rgb].sum()) == 0 and int(rbuf[off_rgb + n * 3 * h * w:].sum()) == 0


def test_device_refusals():
    x = torch.zeros((1, 3, 6, 9), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv420(x)
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(torch.zeros(91, dtype=torch.uint8, device=DEV), 6, 10)
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv420(torch.zeros((1, 3, 6, 10), dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------- the video path
H, W, B = 24, 40, 2


@pytest.fixture(scope="module")
def net():
    """The 2-block synthetic net of test_gpu_video.py: (state_dict, eager runner)."""
    g = models.ResNet(2, 0.2, scaleRate=2)
    sd = synth_state_dict(g.state_dict(), 11)
    g.load_state_dict(sd)
    m = models.Model(g.eval())
    m.init_normalize((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    return sd, tiler.runner_for(m.fuse().eval().to(DEV), DEV)


def upscaler(runner, **kw):
    return video.FrameUpscaler(runner.gw, H, W, B, runner.mean, runner.std, DEV, **kw)


def source_frames(n, layout="i420", seed=4):
    """4:2:0 frames of a smooth moving picture (the restatement of SyntheticVideo's RGB frames)."""
    rgb = np.stack(list(video.SyntheticVideo(W, H, n, seed=seed))).transpose(0, 3, 1, 2)
    return Y.rgb_to_yuv420(rgb, "bt601", False, "left", layout)


def expect(runner, frames, fmt_in, fmt_out):
    """restatement(yuv -> rgb) -> the eager runner -> restatement(rgb -> yuv); a format of None is RGB
    (in: [n, 3, h, w]; out: [n, 3, 2h, 2w])."""
    rgb = frames if fmt_in is None else Y.yuv420_to_rgb(frames, H, W, fmt_in.matrix, fmt_in.full_range, fmt_in.siting,
                                                        fmt_in.layout)
    out = runner(torch.from_numpy(np.ascontiguousarray(rgb)).to(DEV)).cpu().numpy()
    if fmt_out is None:
        return out
    return Y.rgb_to_yuv420(out, fmt_out.matrix, fmt_out.full_range, fmt_out.siting, fmt_out.layout)


@torch.no_grad()
def test_frame_upscaler_yuv_modes(net):
    _, runner = net
    frames = source_frames(B)
    as_in = torch.from_numpy(frames.reshape(B, 3 * H // 2, W))
    # I420 -> I420 with the defaults: limited range, left siting, bt601 at these heights on both sides
    up = upscaler(runner, pix_fmt_in="yuv420p", pix_fmt_out="yuv420p")
    assert up.in_frame_shape == (36, 40) and up.out_frame_shape == (72, 80) and up.x_hwc is None and up.bgr is None
    assert up.yuv_in == yuv.YUVFormat("i420", "bt601", False, "left") == up.yuv_out
    got = up(as_in).cpu().numpy()
    assert got.shape == (B, 72, 80)
    assert np.array_equal(got.reshape(B, -1), expect(runner, frames, up.yuv_in, up.yuv_out))
    # a second batch through the same graph, ragged
    more = source_frames(1, seed=9)
    got = up(torch.from_numpy(more.reshape(1, 36, 40))).cpu().numpy()
    assert np.array_equal(got.reshape(1, -1), expect(runner, more, up.yuv_in, up.yuv_out))
    # I420 in -> NV12 out, other formats on the two sides
    fi, fo = yuv.YUVFormat("i420", "bt709", True, "center"), yuv.YUVFormat("nv12", "bt601", False, "left")
    up = upscaler(runner, pix_fmt_in="yuv420p", pix_fmt_out="nv12", yuv_in=fi, yuv_out=fo)
    assert np.array_equal(up(as_in).cpu().numpy().reshape(B, -1), expect(runner, frames, fi, fo))
    # yuv420p in -> bgr24 out: the RGB side is today's
    up = upscaler(runner, pix_fmt_in="yuv420p")
    assert up.out_frame_shape == (48, 80, 3) and up.bgr is up.y_out and up.yuv_out is None
    want = expect(runner, frames, up.yuv_in, None)
    assert np.array_equal(up(as_in).cpu().numpy(), want[:, ::-1].transpose(0, 2, 3, 1))
    # and NV12 in -> bgr24 out
    nv = source_frames(B, "nv12")
    up = upscaler(runner, pix_fmt_in="nv12")
    assert up.out_frame_shape == (48, 80, 3) and up.bgr is up.y_out
    want = expect(runner, nv, up.yuv_in, None)
    assert np.array_equal(up(torch.from_numpy(nv.reshape(B, 36, 40))).cpu().numpy(), want[:, ::-1].transpose(0, 2, 3, 1))
    # rgb24 in -> yuv420p out
    hwc = np.stack(list(video.SyntheticVideo(W, H, B, seed=4)))
    up = upscaler(runner, pix_fmt_out="yuv420p")
    assert up.in_frame_shape == (24, 40, 3) and up.x_hwc is up.x_in
    want = expect(runner, hwc.transpose(0, 3, 1, 2), None, up.yuv_out)
    assert np.array_equal(up(torch.from_numpy(hwc)).cpu().numpy().reshape(B, -1), want)
    with pytest.raises(ValueError):
        up(as_in)  # 4:2:0 frames into an rgb24 input
    with pytest.raises(ValueError):
        upscaler(runner, pix_fmt_in="yuv444p")
    with pytest.raises(ValueError):
        upscaler(runner, pix_fmt_out="nv12", yuv_out=yuv.YUVFormat("i420"))


@torch.no_grad()
def test_default_upscaler_is_unchanged(net):
    _, runner = net
    hwc = torch.from_numpy(np.stack(list(video.SyntheticVideo(W, H, B, seed=2))))
    a = video.FrameUpscaler(runner.gw, H, W, B, runner.mean, runner.std, DEV)
    b = upscaler(runner, pix_fmt_in="rgb24", pix_fmt_out="bgr24", yuv_in=None, yuv_out=None)
    assert a.x_hwc is a.x_in and a.bgr is a.y_out and a.yuv_in is None and a.yuv_out is None
    assert tuple(a.x_hwc.shape) == (B, H, W, 3) and tuple(a.bgr.shape) == (B, 2 * H, 2 * W, 3)
    got = a(hwc).cpu()
    assert torch.equal(got, b(hwc).cpu())
    eager = runner(hwc.permute(0, 3, 1, 2).contiguous().to(DEV)).cpu()
    assert torch.equal(got, eager.flip(1).permute(0, 2, 3, 1))


def write_y4m(path, frames, header=b"YUV4MPEG2 W40 H24 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"):
    path.write_bytes(header + b"".join(b"FRAME\n" + f.tobytes() for f in frames))


def read_y4m(path, n, h, w):
    data = path.read_bytes()
    head, _, body = data.partition(b"\n")
    fb = Y.frame_bytes(h, w)
    assert len(body) == n * (fb + 6)
    out = []
    for i in range(n):
        rec = body[i * (fb + 6):(i + 1) * (fb + 6)]
        assert rec[:6] == b"FRAME\n"
        out.append(np.frombuffer(rec[6:], np.uint8))
    return head + b"\n", np.stack(out)


@torch.no_grad()
def test_y4m_streams_through_the_pipeline(net, tmp_path):
    _, runner = net
    frames = source_frames(5)
    write_y4m(tmp_path / "in.y4m", frames)
    src = video.open_video(tmp_path / "in.y4m")
    assert src.yuv == yuv.YUVFormat("i420", "auto", True, "center") and len(src) == 5
    up = upscaler(runner, pix_fmt_in="yuv420p", pix_fmt_out="yuv420p", yuv_in=src.yuv, yuv_out=src.yuv)
    rec = video.Y4MRecorder(tmp_path / "out.y4m", (2 * W, 2 * H), src.fps, up.yuv_out)
    assert video.VideoUpscaler(up).run(src, rec) == 5  # batches of 2, 2 and 1
    rec.stopRecorder()
    head, out = read_y4m(tmp_path / "out.y4m", 5, 2 * H, 2 * W)
    assert head == b"YUV4MPEG2 W80 H48 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    back = video.Y4MReader(tmp_path / "out.y4m")
    assert (back.width, back.height, back.fps, back.yuv) == (80, 48, 25.0, src.yuv) and len(back) == 5
    for i in range(5):
        assert np.array_equal(out[i:i + 1], expect(runner, frames[i:i + 1], up.yuv_in, up.yuv_out)), f"frame {i}"


@torch.no_grad()
def test_rs_y4m_to_y4m(net, tmp_path):
    """rs.py's video branch, .y4m in and .y4m out, on the same net saved as a bare state_dict."""
    import rs
    sd, _ = net
    torch.save(sd, tmp_path / "net.pt")
    frames = source_frames(3)
    write_y4m(tmp_path / "in.y4m", frames, b"YUV4MPEG2 W40 H24 F30:1 Ip C420mpeg2\n")
    kw = vars(rs.build_parser().parse_args(["--model", str(tmp_path / "net.pt"), "--src", str(tmp_path / "in.y4m"),
                                            "--save_dir", str(tmp_path / "out.y4m"), "--batch_size", "2"]))
    rs.runer(**kw)
    head, out = read_y4m(tmp_path / "out.y4m", 3, 2 * H, 2 * W)
    assert head == b"YUV4MPEG2 W80 H48 F30:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n"
    runner = tiler.runner_for(rs.build_model(str(tmp_path / "net.pt"), 0.2, kw["mean"], kw["std"]), DEV)
    fmt = yuv.YUVFormat("i420", "bt601", False, "left")
    assert np.array_equal(out, expect(runner, frames, fmt, fmt))
    # the flags override the header, and a .nv12 save_dir is headerless NV12
    rs.runer(**dict(kw, save_dir=str(tmp_path / "out.nv12"), yuv_matrix="bt709", yuv_range="full", yuv_siting="center"))
    fmt = yuv.YUVFormat("i420", "bt709", True, "center")
    got = np.frombuffer((tmp_path / "out.nv12").read_bytes(), np.uint8).reshape(3, -1)
    assert np.array_equal(got, expect(runner, frames, fmt, yuv.YUVFormat("nv12", "bt709", True, "center")))
    torch.cuda.synchronize()
