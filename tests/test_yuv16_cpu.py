"""10-bit YUV 4:2:0 video I/O, the parts that need no GPU: libisr's coefficient builder at a depth
(isr_yuv_coeffs_depth) against isr_yuv_coeffs and the numpy restatement (tests/yuv16_ref.py), the integer
restatement against fp64 with bounds derived from the tables, the int32 overflow the GPU extremes test
relies on, flat-colour round trips, the tanh quantiser against rational arithmetic, the 10-bit Y4M
header, readers and recorder, YUVFormat at both depths, rs.py's flags, the ffmpeg argv and the
descriptor's layout against C (every refusal of the two entry points: tests/test_capi_refusals.py)."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest
import torch

import yuv16_ref as R
import yuv_ref as Y
from conftest import ROOT
from image_super_resolution_amd import _lib, video, yuv

PAIRS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]
COMBOS = [(m, fr, s) for m, fr in PAIRS for s in ("left", "center")]
TOP = 1023


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def random_rgb(n, h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 1024, (n, 3, h, w)).astype(np.uint16)


def random_frames(n, h, w, shift=0, seed=0):
    words = np.random.default_rng(seed + 1000 * h + w).integers(0, 1024, (n, 3 * h * w // 2)).astype("<u2") << shift
    return words.astype("<u2").view(np.uint8).reshape(n, -1)


def extreme_frames(h, w, layout="i420", shift=0):
    """Planes of 0 and 1023 in all eight combinations: [8, 3 h w] bytes and the [8, 3] plane values."""
    ends = np.array(list(itertools.product((0, TOP), repeat=3)), dtype=np.int64)
    planes = [np.broadcast_to(ends[:, i, None, None], (8, h >> (i > 0), w >> (i > 0))) for i in range(3)]
    return R.pack(*planes, layout, shift), ends


# ------------------------------------------------------------------------------- coefficients
def test_depth_8_equals_the_8_bit_builder():
    for m, fr in PAIRS:
        f8, i8 = yuv.coeffs(m, fr)
        fd, idp = yuv.coeffs(m, fr, 8)
        lib = _lib.load()
        fwd, inv = np.zeros(9, dtype=np.int32), np.zeros(5, dtype=np.int32)
        assert lib.isr_yuv_coeffs_depth(yuv.MATRICES.index(m), int(fr), 8, fwd.ctypes.data, inv.ctypes.data) == 0
        assert np.array_equal(fwd.reshape(3, 3), f8) and np.array_equal(inv, i8), (m, fr)
        assert np.array_equal(fd, f8) and np.array_equal(idp, i8)
        assert np.array_equal(R.coeffs(m, fr, 8)[0], Y.coeffs(m, fr)[0]) and np.array_equal(R.coeffs(m, fr, 8)[1], Y.coeffs(m, fr)[1])


def test_depth_10_equals_the_restatement():
    for m, fr in PAIRS:
        fwd, inv = yuv.coeffs(m, fr, 10)
        rf, ri = R.coeffs(m, fr, 10)
        assert fwd.dtype == np.int32 and np.array_equal(fwd, rf) and np.array_equal(inv, ri), (m, fr, fwd - rf, inv - ri)
        sy = R.scales(fr, 10)[0]
        assert int(fwd[0].sum()) == R.fix(sy) and int(fwd[1].sum()) == 0 and int(fwd[2].sum()) == 0
        real, _ = R.real_coeffs(m, fr, 10)
        assert np.abs(fwd - real * 65536).max() <= 1.5
    assert R.scales(False, 10) == (876.0 / 1023.0, 896.0 / 1023.0, 64)
    lib = _lib.load()
    fwd, inv = np.full(9, -7, dtype=np.int32), np.full(5, -7, dtype=np.int32)
    for depth in (0, 7, 9, 12, 16):
        assert lib.isr_yuv_coeffs_depth(0, 0, depth, fwd.ctypes.data, inv.ctypes.data) == -2
        assert b"depth" in lib.isr_last_error()
    assert lib.isr_yuv_coeffs_depth(2, 0, 10, fwd.ctypes.data, inv.ctypes.data) == -2 and b"matrix" in lib.isr_last_error()
    assert (fwd == -7).all() and (inv == -7).all()
    assert lib.isr_yuv_coeffs_depth(0, 0, 10, None, inv.ctypes.data) == -1 and b"null" in lib.isr_last_error()


def test_greys_give_mid_chroma():
    greys = np.broadcast_to(np.arange(1024, dtype=np.uint16)[:, None, None, None], (1024, 3, 2, 4))
    for m, fr, s in COMBOS:
        y, u, v = R.unpack(R.rgb_to_yuv420(greys, m, fr, s), 2, 4, "i420")
        assert (u == 512).all() and (v == 512).all(), (m, fr, s)
        if fr:
            assert np.array_equal(y, greys[:, 0])
        else:
            assert (y[0] == 64).all() and (y[1023] == 940).all()


# ------------------------------------------------------------------------------- arithmetic
def table_bounds(m, fr):
    """(forward, inverse per channel): 0.5 for the one rounding plus, coefficient by coefficient, the
    table's error times its operand's range: 1023 for R, G, B, S / D and Y - oy, 512 for a centred chroma."""
    fwd, inv = R.coeffs(m, fr)
    rf, ri = R.real_coeffs(m, fr)
    ef = 0.5 + (np.abs(fwd / 65536.0 - rf).sum(axis=1) * 1023).max()
    d = np.abs(inv / 65536.0 - np.array(ri))
    ei = 0.5 + d[0] * 1023 + 512 * np.array([d[1], d[3] + d[4], d[2]])
    return ef + 1e-9, ei + 1e-9


def test_restatement_against_exact():
    """|integer - exact| before the clamp is within the bound of table_bounds, both directions, over
    random and extreme frames.  The exact value is clipped like the integer one: clipping is 1-Lipschitz."""
    worst_f = worst_i = 0.0
    for m, fr, s in COMBOS:
        ef, ei = table_bounds(m, fr)
        assert ef < 0.55 and ei.max() < 0.55  # the tables are good to 2^-17 each: far from a second unit
        for h, w in ((2, 2), (6, 10), (18, 34)):
            cases = [random_rgb(2, h, w)] + [np.broadcast_to(np.array(e, dtype=np.uint16)[None, :, None, None], (1, 3, h, w))
                                             for e in itertools.product((0, TOP), repeat=3)]
            for rgb in cases:
                got = R.unpack(R.rgb_to_yuv420(rgb, m, fr, s), h, w, "i420")
                for g, e in zip(got, R.rgb_to_yuv420_exact(rgb, m, fr, s)):
                    err = np.abs(g - np.clip(e, 0, TOP)).max()
                    worst_f = max(worst_f, err)
                    assert err <= ef, (m, fr, s, h, w, err, ef)
            for frames in (random_frames(2, h, w), extreme_frames(h, w)[0]):
                back = R.yuv420_to_rgb(frames, h, w, m, fr, s).astype(np.float64)
                exact = np.clip(R.yuv420_to_rgb_exact(frames, h, w, m, fr, s), 0, TOP)
                err = np.abs(back - exact).max(axis=(0, 2, 3))
                worst_i = max(worst_i, err.max())
                assert (err <= ei).all(), (m, fr, s, h, w, err, ei)
    print(f"worst |integer - exact|: rgb -> yuv {worst_f:.4f}, yuv -> rgb {worst_i:.4f}")


def test_overflow_premise():
    """The blue sum of limited-range bt709 at center siting passes int32 on planes of 1023 (so the GPU
    extremes test exercises the 64-bit sums); full range stays inside, and so does every forward sum."""
    for h, w in ((6, 10), (4, 32)):
        frames, _ = extreme_frames(h, w)
        peak = []
        R.yuv420_to_rgb(frames, h, w, "bt709", False, "center", peak=peak)
        assert peak[0] > 2 ** 31 - 1 and peak[0] < 2.32e9, peak
        peak = []
        R.yuv420_to_rgb(frames, h, w, "bt709", True, "center", peak=peak)
        assert peak[0] <= 2 ** 31 - 1, peak
    ends = np.array(list(itertools.product((0, TOP), repeat=3)), dtype=np.uint16)
    for m, fr, s in COMBOS:
        peak = []
        R.rgb_to_yuv420(np.broadcast_to(ends[:, :, None, None], (8, 3, 2, 4)), m, fr, s, peak=peak)
        assert peak[0] < 5.4e8, (m, fr, s, peak)
        # each term of the inverse fits int32 on its own, and the green sum does (include/isr.h)
        _, (cy, crv, cbu, cgu, cgv) = R.coeffs(m, fr)
        oy = R.scales(fr)[2]
        assert cy * 16 * (TOP - oy) + 32768 * 16 < 1.18e9 and max(crv, cbu) * 8192 < 1.14e9
        assert cy * 16 * (TOP - oy) + 32768 * 16 - 8192 * (cgu + cgv) < 1.84e9
        assert -cy * 16 * oy + 8176 * (cgu + cgv) > -7.4e8


def test_flat_colours_round_trip():
    """rgb10 -> yuv10 -> rgb10 of flat images of a 12^3 lattice.  The stored Y, Cb, Cr are each within
    ef of the exact ones (table_bounds), the exact inverse turns that into at most cy ef + (|cgu| + |cgv|
    or crv or cbu) ef, and the integer inverse adds its own ei; both ends are integers, so the
    difference is at most the floor of the sum.  Flat images: the filters pass a constant through."""
    lattice = np.array(list(itertools.product(range(0, 1024, 93), repeat=3)), dtype=np.uint16)
    assert lattice.shape == (1728, 3) and lattice.max() == TOP
    flat = np.broadcast_to(lattice[:, :, None, None], (1728, 3, 2, 4))
    for m, fr, s in COMBOS:
        ef, ei = table_bounds(m, fr)
        cy, crv, cbu, cgu, cgv = R.real_coeffs(m, fr)[1]
        bound = np.floor(ef * (cy + np.array([crv, abs(cgu) + abs(cgv), cbu])) + ei).astype(int)
        assert bound.max() <= 2
        back = R.yuv420_to_rgb(R.rgb_to_yuv420(flat, m, fr, s), 2, 4, m, fr, s)
        worst = np.abs(back.astype(int) - flat).max(axis=(0, 2, 3))
        print(m, fr, s, "worst", worst.tolist(), "bound", bound.tolist())
        assert (worst <= bound).all(), (m, fr, s, worst, bound)


def test_tanh_quantiser_against_rational_arithmetic():
    t = R.special_tanh_values()
    assert t.dtype == np.float32 and len(t) > 4000
    got = R.quantise(t)
    want = np.array([R.quantise_exact(v) for v in t])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert np.array_equal(got[:1024], np.arange(1024))  # the level centres
    for v, q in ((1.0, TOP), (-1.0, 0), (0.0, 512), (-0.0, 512), (1.5, TOP), (-1.5, 0), (np.inf, TOP), (-np.inf, 0),
                 (np.nan, 0)):
        assert R.quantise(np.float32(v)) == q, v
    # 0 is a half-way point (511.5): half-even takes it up to 512; so does a t that t + 1 rounds to 1; the
    # first t below whose t + 1 is below 1 goes down
    assert R.quantise(np.nextafter(np.float32(0), np.float32(-1))) == 512 and R.quantise(np.float32(-2.0 ** -24)) == 511


def test_consistency_derivation_on_one_value():
    """The GPU consistency case's |Y10 - 4 Y8| <= 5 from one fp32 t, grey, limited range: quantising t to
    8 bits moves each of R, G, B by at most 0.5 of 255, worth 0.5 sy 4 = 1.72 of a 10-bit luma step; the
    8-bit luma rounding 0.5 x 4 = 2; the 10-bit path's own two roundings 0.5 sy10 + 0.5 = 0.93."""
    sy8, sy10 = 219.0 / 255.0, 876.0 / 1023.0
    assert 0.5 * sy8 * 4 <= 1.72 and 0.5 * sy10 + 0.5 <= 0.93 and 1.72 + 2 + 0.93 <= 5
    rng = np.random.default_rng(3)
    t = rng.uniform(-1, 1, (64, 1, 2, 4)).astype(np.float32)
    t = np.broadcast_to(t, (64, 3, 2, 4))
    q8 = np.clip(np.rint((t + np.float32(1)) / np.float32(2) * np.float32(255)), 0, 255).astype(np.uint8)
    y8 = Y.unpack(Y.rgb_to_yuv420(q8, "bt601", False, "left"), 2, 4, "i420")[0].astype(int)
    y10 = R.unpack(R.rgb_to_yuv420(R.quantise(t), "bt601", False, "left"), 2, 4, "i420")[0]
    assert np.abs(y10 - 4 * y8).max() <= 5


# ------------------------------------------------------------------------------- formats and files
def test_format_at_both_depths():
    assert yuv.YUVFormat("i420", "auto", True, "center") == yuv.YUVFormat("i420", "auto", True, "center", 8)
    assert yuv.YUVFormat("i420", "auto", True, "center") != yuv.YUVFormat("i420", "auto", True, "center", 10)
    assert yuv.YUVFormat().depth == 8 and yuv.YUVFormat().shift == 0
    for name, layout, depth, shift in (("yuv420p", "i420", 8, 0), ("nv12", "nv12", 8, 0), ("yuv420p10le", "i420", 10, 0),
                                       ("p010le", "nv12", 10, 6)):
        f = yuv.YUVFormat.of_pix_fmt(name)
        assert (f.layout, f.depth, f.pix_fmt, f.shift) == (layout, depth, name, shift)
        assert f.resolved(1080) == yuv.YUVFormat(layout, "bt709", False, "left", depth)
    assert set(yuv.PIX_FMTS) == {"yuv420p", "nv12", "yuv420p10le", "p010le"}
    for bad in (9, 12, 16, "10"):
        with pytest.raises(ValueError):
            yuv.YUVFormat(depth=bad)
    with pytest.raises(ValueError):
        yuv.YUVFormat(matrix="bt2020", depth=10)
    assert yuv.frame_bytes(6, 10) == 90 and yuv.frame_bytes(6, 10, 8) == 90 and yuv.frame_bytes(6, 10, depth=10) == 180
    assert yuv.frame_bytes(6, 10, 10) == R.frame_bytes(6, 10)
    for h, w, d in ((5, 10, 10), (6, 9, 10), (6, 10, 12)):
        with pytest.raises(ValueError):
            yuv.frame_bytes(h, w, d)
    with pytest.raises(RuntimeError, match="HIP"):
        yuv.yuv420_to_rgb(torch.zeros(180, dtype=torch.uint8), 6, 10, yuv.YUVFormat(depth=10))
    with pytest.raises(RuntimeError, match="HIP"):
        yuv.rgb_to_yuv420(torch.zeros((1, 3, 6, 10), dtype=torch.float32), yuv.YUVFormat(depth=10))


def test_y4m_10_bit_header():
    for fr in (False, True):
        fmt = yuv.YUVFormat("i420", "auto", fr, "left", 10)
        head = video.y4m_header(40, 24, 25, fmt)
        assert head.startswith(b"YUV4MPEG2 W40 H24 F25:1 Ip ") and head.endswith(b"\n")
        assert b"C420p10" in head.split() and b"XYSCSS=420P10" in head.split()
        assert (b"XCOLORRANGE=FULL" if fr else b"XCOLORRANGE=LIMITED") in head.split()
        meta = video.parse_y4m_header(head, depths=(8, 10))
        assert (meta["width"], meta["height"], meta["fps"], meta["yuv"]) == (40, 24, 25.0, fmt)
        with pytest.raises(ValueError, match="C420p10"):
            video.parse_y4m_header(head)
        with pytest.raises(ValueError, match="C420p10"):
            video.parse_y4m_header(head, depths=(8,))
    with pytest.raises(ValueError, match="center"):
        video.y4m_header(40, 24, 25, yuv.YUVFormat("i420", "auto", False, "center", 10))
    with pytest.raises(ValueError):
        video.y4m_header(40, 24, 25, yuv.YUVFormat("nv12", depth=10))
    # the 8-bit tags are read as before with the keyword, and other depths stay refused
    meta = video.parse_y4m_header(b"YUV4MPEG2 W8 H6 F30:1 Ip C420mpeg2\n", depths=(8, 10))
    assert meta["yuv"] == yuv.YUVFormat("i420", "auto", False, "left")
    for bad in ("C420p12", "C422p10", "C444p10", "C420p16"):
        with pytest.raises(ValueError, match=bad):
            video.parse_y4m_header(f"YUV4MPEG2 W8 H6 F30:1 {bad}\n".encode(), depths=(8, 10))


def test_y4m_10_bit_reader_and_recorder(tmp_path):
    h, w = 6, 10
    frames = random_frames(3, h, w)
    assert frames.shape == (3, 180)
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 W10 H6 F24:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n" +
                    b"".join(b"FRAME\n" + f.tobytes() for f in frames))
    rd = video.open_video(src)
    assert isinstance(rd, video.Y4MReader) and len(rd) == 3
    assert (rd.width, rd.height, rd.fps, rd.pix_fmt, rd.frame_shape) == (w, h, 24.0, "yuv420p10le", (9, 20))
    assert rd.yuv == yuv.YUVFormat("i420", "auto", True, "left", 10)
    got = list(rd)
    assert len(got) == 3 and all(g.shape == (9, 20) and g.dtype == np.uint8 for g in got)
    for g, f in zip(got, frames):
        y, u, v = R.unpack(g, h, w, "i420")
        words = f.view("<u2")
        assert np.array_equal(g.ravel(), f) and np.array_equal(y[0], words[:60].reshape(6, 10))
        assert np.array_equal(u[0], words[60:75].reshape(3, 5)) and np.array_equal(v[0], words[75:].reshape(3, 5))
    (tmp_path / "cut.y4m").write_bytes(src.read_bytes()[:-7])
    cut = video.Y4MReader(tmp_path / "cut.y4m")
    assert len(list(cut)) == 2
    rec = video.Y4MRecorder(tmp_path / "out.y4m", (w, h), 24, rd.yuv)
    for g in got:
        rec.writeFrame(g)
    rec.stopRecorder()
    assert (tmp_path / "out.y4m").read_bytes() == src.read_bytes()
    with pytest.raises(ValueError):  # an 8-bit frame into a 10-bit file
        video.Y4MRecorder(tmp_path / "bad.y4m", (w, h), 24, rd.yuv).writeFrame(np.zeros((9, 10), np.uint8))
    # an 8-bit file is read as before
    (tmp_path / "in8.y4m").write_bytes(b"YUV4MPEG2 W10 H6 F24:1 Ip C420mpeg2\n" + b"FRAME\n" + bytes(90))
    r8 = video.Y4MReader(tmp_path / "in8.y4m")
    assert (r8.pix_fmt, r8.frame_shape, len(r8), r8.yuv.depth) == ("yuv420p", (9, 10), 1, 8)
    # headerless words: --pix_fmt gives the depth
    for suffix, layout, pix in ((".yuv", "i420", "yuv420p10le"), (".i420", "i420", "yuv420p10le"), (".nv12", "nv12", "p010le")):
        raw = tmp_path / f"in{suffix}"
        raw.write_bytes(frames.tobytes())
        rr = video.open_video(raw, w, h, 25.0, pix)
        assert isinstance(rr, video.RawYUVReader) and len(rr) == 3 and rr.frame_shape == (9, 20)
        assert rr.yuv == yuv.YUVFormat(layout, depth=10) and rr.pix_fmt == pix
        assert all(np.array_equal(a.ravel(), f) for a, f in zip(rr, frames))
        assert len(video.open_video(raw, w, h, 25.0)) == 6  # the same bytes as 8-bit frames
    assert len(video.RawYUVReader(tmp_path / "in.yuv", w, h, depth=10)) == 3
    (tmp_path / "odd.yuv").write_bytes(b"\0" * 270)
    with pytest.raises(ValueError):
        video.RawYUVReader(tmp_path / "odd.yuv", w, h, depth=10)


def test_recorder_and_reader_argv_10_bit():
    for pix, layout in (("yuv420p10le", "i420"), ("p010le", "nv12")):
        r = video.FFMPEG_recorder("x.mp4", (3840, 2160), 30, codec="libx264", dry_run=True, pix_fmt=pix)
        i = r.cmd.index("-i")
        source, sink = r.cmd[:i], r.cmd[i:]
        assert source[source.index("-pixel_format") + 1] == pix and r.yuv == yuv.YUVFormat(layout, "bt709", False, "left", 10)
        for part in (source, sink):
            assert part[part.index("-colorspace") + 1] == "bt709" and part[part.index("-color_range") + 1] == "tv"
        assert sink[sink.index("-pix_fmt") + 1] == "yuv420p10le" and r.cmd[-1] == "x.mp4"
        cmd = video.ffmpeg_reader_cmd("clip.mkv", pix)
        assert cmd == ["ffmpeg", "-v", "quiet", "-i", "clip.mkv", "-f", "rawvideo", "-pix_fmt", pix, "pipe:"]
        rd = video.FFmpegVideoReader("clip.mkv", pix, meta=dict(width=1920, height=1080, fps=25.0, frames=7))
        assert rd.cmd == cmd and rd.frame_shape == (1620, 3840) and rd.yuv == yuv.YUVFormat(layout, depth=10)
    r = video.FFMPEG_recorder("x.mp4", (640, 480), 30, codec="libx264", dry_run=True, pix_fmt="yuv420p")
    assert r.cmd[r.cmd.index("-pix_fmt") + 1] == "yuv420p"
    with pytest.raises(ValueError):  # the pipe's name and the format's depth disagree
        video.FFMPEG_recorder("x.mp4", (640, 480), 30, codec="libx264", dry_run=True, pix_fmt="yuv420p10le",
                              yuv=yuv.YUVFormat("i420"))


def test_rs_out_depth(tmp_path):
    import rs
    opt = rs.build_parser().parse_args([])
    assert opt.out_depth is None and opt.pix_fmt == "rgb24"
    for pix in ("yuv420p10le", "p010le"):
        assert rs.build_parser().parse_args(["--pix_fmt", pix, "--out_depth", "8"]).pix_fmt == pix
    assert rs.build_parser().parse_args(["--out_depth", "10"]).out_depth == 10
    for bad in (["--out_depth", "12"], ["--out_depth", "ten"], ["--pix_fmt", "yuv422p10le"]):
        with pytest.raises(SystemExit):
            rs.build_parser().parse_args(bad)

    class Src:
        def __init__(self, fmt=None):
            self.yuv, self.pix_fmt = fmt, (fmt.pix_fmt if fmt else "rgb24")

    none = dict(pix_fmt="rgb24", yuv_matrix=None, yuv_range=None, yuv_siting=None)  # no out_depth key: today's call
    h8, h10 = yuv.YUVFormat("i420", "auto", True, "center"), yuv.YUVFormat("i420", "auto", True, "left", 10)
    assert rs.video_formats(none, Src(h8), tmp_path / "o.y4m") == ("yuv420p", h8, "yuv420p", h8)
    assert rs.video_formats(dict(none, out_depth=None), Src(h8), tmp_path / "o.y4m") == ("yuv420p", h8, "yuv420p", h8)
    # 10 in -> 10 out by default, every suffix
    assert rs.video_formats(none, Src(h10), tmp_path / "o.y4m") == ("yuv420p10le", h10, "yuv420p10le", h10)
    assert rs.video_formats(none, Src(h10), tmp_path / "o.nv12")[2:] == ("p010le", yuv.YUVFormat("nv12", "auto", True, "left", 10))
    assert rs.video_formats(none, Src(h10), tmp_path / "o.bgr")[2:] == ("bgr24", None)
    # 10 -> 8 and 8 -> 10; a 10-bit .y4m of a center-sited source is left-sited unless the flag says otherwise
    assert rs.video_formats(dict(none, out_depth=8), Src(h10), tmp_path / "o.yuv")[2:] == ("yuv420p", yuv.YUVFormat("i420", "auto", True, "left"))
    assert rs.video_formats(dict(none, out_depth=10), Src(h8), tmp_path / "o.y4m") == ("yuv420p", h8, "yuv420p10le", h10)
    assert rs.video_formats(dict(none, out_depth=10), Src(h8), tmp_path / "o.yuv")[3] == yuv.YUVFormat("i420", "auto", True, "center", 10)
    assert rs.video_formats(dict(none, out_depth=10), Src(), tmp_path / "o.nv12")[2:] == ("p010le", yuv.YUVFormat("nv12", depth=10))
    # a container follows --pix_fmt, and --out_depth still wins
    p10 = yuv.YUVFormat("nv12", depth=10)
    assert rs.video_formats(dict(none, pix_fmt="p010le"), Src(p10), tmp_path / "o.mp4") == ("p010le", p10, "p010le", p10)
    assert rs.video_formats(dict(none, pix_fmt="p010le", out_depth=8), Src(p10), tmp_path / "o.mp4")[2:] == ("nv12", yuv.YUVFormat("nv12"))


# ------------------------------------------------------------------------------- ABI and refusals
PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "isr.h"
#define F(m) printf(#m " %zu\n", offsetof(isr_yuv16_desc, m))
int main(void) {
  printf("size %zu\n", sizeof(isr_yuv16_desc));
  F(n); F(h); F(w); F(layout); F(siting); F(full_range); F(depth); F(shift); F(rgb_kind); F(fwd); F(inv); F(mean);
  F(inv_std); F(src); F(dst);
  printf("consts %d %d %d\n", ISR_RGB_U16, ISR_RGB_NORM_F32, ISR_RGB_TANH_F32);
  return 0;
}
"""


def test_desc_layout_matches_c(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                   check=True)
    lines = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines()
    c = {ln.split()[0]: ln.split()[1:] for ln in lines}
    assert int(c["size"][0]) == ctypes.sizeof(_lib.IsrYuv16Desc)
    names = [name for name, _ in _lib.IsrYuv16Desc._fields_]
    assert names == ["n", "h", "w", "layout", "siting", "full_range", "depth", "shift", "rgb_kind", "fwd", "inv", "mean",
                     "inv_std", "src", "dst"]
    for name in names:
        assert getattr(_lib.IsrYuv16Desc, name).offset == int(c[name][0]), name
    assert [int(v) for v in c["consts"]] == [0, 1, 2] == [yuv.RGB_KINDS.index(k) for k in ("u16", "norm_f32", "tanh_f32")]
