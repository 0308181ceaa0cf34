"""YUV 4:2:0 video I/O, the parts that need no GPU: libisr's host-side coefficient builder
(isr_yuv_coeffs) against the numpy restatement (tests/yuv_ref.py) as integers, its properties and
refusals, the builder as a stand-alone program under the address and undefined-behaviour
sanitizers, the integer restatement against the same filters and matrices in fp64 (the derived
bound), greys, range end points and flat-colour round trips, the Y4M header and reader, the ffmpeg
argv of the recorder and the reader, rs.py's flags, yuv.py's refusal of CPU tensors and the
descriptor's layout against C (what the two entry points refuse: tests/test_capi_refusals.py)."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest
import torch

import host_program
import yuv_ref as Y
from conftest import ROOT
from image_super_resolution_amd import _lib, video, yuv

PAIRS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]
COMBOS = [(m, fr, s) for m, fr in PAIRS for s in ("left", "center")]


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def random_rgb(n, h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (n, 3, h, w), dtype=np.uint8)


def random_frames(n, h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (n, Y.frame_bytes(h, w)), dtype=np.uint8)


# ------------------------------------------------------------------------------- coefficients
def test_coeff_builder_equals_the_restatement():
    for m, fr in PAIRS:
        fwd, inv = yuv.coeffs(m, fr)
        rf, ri = Y.coeffs(m, fr)
        assert fwd.dtype == np.int32 and fwd.shape == (3, 3) and inv.shape == (5,)
        assert np.array_equal(fwd, rf) and np.array_equal(inv, ri), (m, fr, fwd - rf, inv - ri)
        sy = Y.scales(fr)[0]
        assert int(fwd[0].sum()) == Y.fix(sy) and int(fwd[1].sum()) == 0 and int(fwd[2].sum()) == 0
        # the G entry moved by at most 1.5 units from its own rounding
        real, _ = Y.real_coeffs(m, fr)
        assert np.abs(fwd - real * 65536).max() <= 1.5
    assert Y.fix(219.0 / 255.0) == 56284


def test_coeff_builder_refusals():
    lib = _lib.load()
    fwd, inv = np.full(9, -7, dtype=np.int32), np.full(5, -7, dtype=np.int32)
    for bad in (-1, 2, 99):
        assert lib.isr_yuv_coeffs(bad, 0, fwd.ctypes.data, inv.ctypes.data) == -2
        assert b"matrix" in lib.isr_last_error()
    assert (fwd == -7).all() and (inv == -7).all()
    assert lib.isr_yuv_coeffs(0, 0, None, inv.ctypes.data) == -1 and b"null" in lib.isr_last_error()
    assert lib.isr_yuv_coeffs(0, 0, fwd.ctypes.data, None) == -1 and b"null" in lib.isr_last_error()
    assert lib.isr_yuv_coeffs(1, 1, fwd.ctypes.data, inv.ctypes.data) == 0
    with pytest.raises(ValueError):
        yuv.coeffs("bt2020")


@pytest.mark.skipif(host_program.GXX is None, reason="needs g++")
def test_coeff_builder_standalone_under_sanitizers(tmp_path):
    """csrc/yuv_coeffs.h in a program of its own (tests/yuv_coeffs_main.cpp), plain and with
    -fsanitize=address,undefined (tests/host_program.py): both run clean over every matrix id, range
    and refusal, print the same lines, and those are the integers libisr hands to Python."""
    (out,) = host_program.run_plain_and_sanitized(ROOT / "tests" / "yuv_coeffs_main.cpp", tmp_path,
                                                  extra_flags=("-ffp-contract=off",))
    rows = [[int(v) for v in line.split()] for line in out.splitlines()]
    assert len(rows) == 12 and {r[2] for r in rows} == {0, 1}
    made = 0
    for matrix, full, code, *vals in rows:
        assert (code == 0) == (matrix in (0, 1))
        if code:
            continue
        fwd, inv = yuv.coeffs(yuv.MATRICES[matrix], bool(full))
        assert vals == fwd.ravel().tolist() + inv.tolist(), (matrix, full)
        made += 1
    assert made == 6


# ------------------------------------------------------------------------------- arithmetic
def test_restatement_against_exact():
    """|integer - exact| <= 0.52 before the clamp, both directions: 0.5 for the one rounding, plus the
    coefficient error, at most three terms x 2^-17 x 255 and the G fix-up of 1.5 x 2^-16 x 255, under
    0.02 together.  The exact value is clipped to [0, 255] like the integer one: clipping is
    1-Lipschitz, so it can only bring the two closer."""
    assert 3 * 2.0 ** -17 * 255 + 1.5 * 2.0 ** -16 * 255 < 0.02
    for (m, fr, s), (h, w) in itertools.product(COMBOS, ((2, 2), (6, 10), (18, 34))):
        rgb = random_rgb(2, h, w)
        got = Y.unpack(Y.rgb_to_yuv420(rgb, m, fr, s, "i420"), h, w, "i420")
        for g, e in zip(got, Y.rgb_to_yuv420_exact(rgb, m, fr, s)):
            assert np.abs(g - np.clip(e, 0, 255)).max() <= 0.52, (m, fr, s, h, w)
        assert np.array_equal(Y.unpack(Y.rgb_to_yuv420(rgb, m, fr, s, "nv12"), h, w, "nv12")[2], got[2])
        frames = random_frames(2, h, w)
        back = Y.yuv420_to_rgb(frames, h, w, m, fr, s).astype(np.float64)
        exact = Y.yuv420_to_rgb_exact(frames, h, w, m, fr, s)
        assert np.abs(back - np.clip(exact, 0, 255)).max() <= 0.52, (m, fr, s, h, w)


def test_greys_and_range_ends():
    greys = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 3, 4, 4))
    for m, fr, s in COMBOS:
        y, u, v = Y.unpack(Y.rgb_to_yuv420(greys, m, fr, s), 4, 4, "i420")
        assert (u == 128).all() and (v == 128).all(), (m, fr, s)
        if fr:
            assert np.array_equal(y, greys[:, 0])
            assert np.array_equal(Y.yuv420_to_rgb(Y.pack(y, u, v, "i420"), 4, 4, m, fr, s), greys)
        else:
            assert (y[0] == 16).all() and (y[255] == 235).all()
            back = Y.yuv420_to_rgb(Y.pack(y, u, v, "i420"), 4, 4, m, fr, s)
            assert (back[0] == 0).all() and (back[255] == 255).all()
            assert np.abs(back.astype(int) - greys).max() <= 1  # 0.5 cy = 0.58 of a value, rounded once more


def test_flat_colours_round_trip_within_2():
    """A flat image of every colour of a 16^3 lattice comes back within 2 per channel, all eight
    (matrix, range, siting): the stored Y, Cb, Cr are each off by at most 0.5, which the inverse turns
    into at most 0.5 cy + 0.5 cbu <= 0.58 + 1.06 (B, BT.709 limited: the largest), rounded once more.
    Flat images: the filters pass a constant through exactly (weights sum to D)."""
    lattice = np.array(list(itertools.product(range(0, 256, 17), repeat=3)), dtype=np.uint8)
    assert lattice.shape == (4096, 3)
    flat = np.broadcast_to(lattice[:, :, None, None], (4096, 3, 2, 4))
    for m, fr, s in COMBOS:
        back = Y.yuv420_to_rgb(Y.rgb_to_yuv420(flat, m, fr, s), 2, 4, m, fr, s)
        worst = int(np.abs(back.astype(int) - flat).max())
        print(m, fr, s, "worst", worst)
        assert worst <= 2, (m, fr, s, worst)


# ------------------------------------------------------------------------------- Y4M
def test_y4m_header_round_trip():
    for siting, tag in (("left", "C420mpeg2"), ("center", "C420jpeg")):
        for fr in (False, True):
            fmt = yuv.YUVFormat("i420", "auto", fr, siting)
            head = video.y4m_header(40, 24, 25, fmt)
            assert head.startswith(b"YUV4MPEG2 W40 H24 F25:1 Ip ") and head.endswith(b"\n")
            assert tag.encode() in head.split() and (b"XCOLORRANGE=FULL" if fr else b"XCOLORRANGE=LIMITED") in head.split()
            meta = video.parse_y4m_header(head)
            assert (meta["width"], meta["height"], meta["fps"], meta["yuv"]) == (40, 24, 25.0, fmt)
    assert video.parse_y4m_header(video.y4m_header(8, 8, 30000 / 1001, yuv.YUVFormat()))["fps"] == pytest.approx(29.97, abs=1e-3)
    for tag, siting in (("C420jpeg", "center"), ("C420", "center"), ("", "center"), ("C420mpeg2", "left")):
        meta = video.parse_y4m_header(f"YUV4MPEG2 W8 H6 F30:1 I? {tag}\n".encode())
        assert meta["yuv"].siting == siting and not meta["yuv"].full_range
    for bad in ("C422", "C444", "C420p10", "C420paldv", "Cmono", "Ii", "It"):
        with pytest.raises(ValueError, match=bad):
            video.parse_y4m_header(f"YUV4MPEG2 W8 H6 F30:1 {bad}\n".encode())
    for w, h in ((7, 6), (8, 5), (0, 2)):
        with pytest.raises(ValueError):
            video.parse_y4m_header(f"YUV4MPEG2 W{w} H{h} F30:1 Ip\n".encode())
        with pytest.raises(ValueError):
            video.y4m_header(w, h, 30, yuv.YUVFormat())
    with pytest.raises(ValueError):
        video.parse_y4m_header(b"RIFF W8 H6\n")
    with pytest.raises(ValueError):
        video.y4m_header(8, 6, 30, yuv.YUVFormat("nv12"))


def test_y4m_reader_and_recorder(tmp_path):
    h, w = 6, 10
    frames = random_frames(3, h, w)
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 W10 H6 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL\n" +
                    b"".join(b"FRAME\n" + f.tobytes() for f in frames))
    rd = video.open_video(src)
    assert isinstance(rd, video.Y4MReader) and len(rd) == 3
    assert (rd.width, rd.height, rd.fps, rd.pix_fmt) == (w, h, 24.0, "yuv420p")
    assert rd.yuv == yuv.YUVFormat("i420", "auto", True, "left")
    got = list(rd)
    assert len(got) == 3 and all(g.shape == (9, 10) and g.dtype == np.uint8 for g in got)
    for g, f in zip(got, frames):
        y, u, v = Y.unpack(g.reshape(1, -1), h, w, "i420")
        assert np.array_equal(g.ravel(), f) and np.array_equal(y[0], f[:60].reshape(6, 10))
        assert np.array_equal(u[0], f[60:75].reshape(3, 5)) and np.array_equal(v[0], f[75:].reshape(3, 5))
    # a truncated last frame ends the stream; so does a missing FRAME line
    (tmp_path / "cut.y4m").write_bytes(src.read_bytes()[:-7])
    assert len(list(video.Y4MReader(tmp_path / "cut.y4m"))) == 2
    # the recorder writes a file the reader gives back
    rec = video.Y4MRecorder(tmp_path / "out.y4m", (w, h), 24, rd.yuv)
    for g in got:
        rec.writeFrame(g)
    rec.stopRecorder()
    assert (tmp_path / "out.y4m").read_bytes() == src.read_bytes()
    with pytest.raises(ValueError):
        video.Y4MRecorder(tmp_path / "bad.y4m", (w, h), 24).writeFrame(np.zeros((6, 10, 3), np.uint8))
    # headerless I420 / NV12
    for suffix, layout in ((".yuv", "i420"), (".i420", "i420"), (".nv12", "nv12")):
        raw = tmp_path / f"in{suffix}"
        raw.write_bytes(frames.tobytes())
        rr = video.open_video(raw, w, h, 25.0)
        assert isinstance(rr, video.RawYUVReader) and len(rr) == 3 and rr.yuv.layout == layout
        assert rr.pix_fmt == ("nv12" if layout == "nv12" else "yuv420p")
        assert all(np.array_equal(a.ravel(), f) for a, f in zip(rr, frames))
        with pytest.raises(ValueError):
            video.open_video(raw)
    (tmp_path / "odd.yuv").write_bytes(b"\0" * 91)
    with pytest.raises(ValueError):
        video.RawYUVReader(tmp_path / "odd.yuv", w, h)


# ------------------------------------------------------------------------------- ffmpeg argv
def test_recorder_and_reader_argv():
    r = video.FFMPEG_recorder("out dir/x.mp4", (3840, 2160), 30, codec="libx264", dry_run=True)
    assert r.cmd == ["ffmpeg", "-v", "quiet", "-y", "-s", "3840x2160", "-pixel_format", "bgr24", "-f", "rawvideo",
                     "-r", "30", "-i", "pipe:", "-vcodec", "libx264", "-pix_fmt", "yuv420p", "-b:v", "20.0M",
                     "out_dir/x.mp4"]
    for pix in ("nv12", "yuv420p"):
        r = video.FFMPEG_recorder("x.mp4", (3840, 2160), 30, codec="libx264", dry_run=True, pix_fmt=pix)
        i = r.cmd.index("-i")
        source, sink = r.cmd[:i], r.cmd[i:]
        assert source[source.index("-pixel_format") + 1] == pix
        for part in (source, sink):
            assert part[part.index("-colorspace") + 1] == "bt709"
            assert part[part.index("-color_range") + 1] == "tv"
            assert part[part.index("-chroma_sample_location") + 1] == "left"
        assert sink[sink.index("-pix_fmt") + 1] == "yuv420p" and r.cmd[-1] == "x.mp4"
    r = video.FFMPEG_recorder("x.mp4", (640, 480), 30, codec="libx264", dry_run=True, pix_fmt="yuv420p",
                              yuv=yuv.YUVFormat("i420", "auto", True, "center"))
    assert r.cmd[r.cmd.index("-colorspace") + 1] == "smpte170m" and r.cmd[r.cmd.index("-color_range") + 1] == "pc"
    assert r.cmd[r.cmd.index("-chroma_sample_location") + 1] == "center"
    with pytest.raises(ValueError):
        video.FFMPEG_recorder("x.mp4", (640, 480), 30, codec="libx264", dry_run=True, pix_fmt="nv12",
                              yuv=yuv.YUVFormat("i420"))
    with pytest.raises(ValueError):
        video.FFMPEG_recorder("x.mp4", (640, 480), 30, codec="libx264", dry_run=True, pix_fmt="yuv444p")
    assert video.ffmpeg_reader_cmd("a b/clip.mp4") == ["ffmpeg", "-v", "quiet", "-i", "a b/clip.mp4", "-f", "rawvideo",
                                                      "-pix_fmt", "rgb24", "pipe:"]
    cmd = video.ffmpeg_reader_cmd("clip.mp4", "nv12")
    assert cmd[cmd.index("-pix_fmt") + 1] == "nv12" and cmd[-1] == "pipe:"
    with pytest.raises(ValueError):
        video.ffmpeg_reader_cmd("clip.mp4", "yuv422p")
    # the reader itself, made without the binaries from given stream properties
    meta = dict(width=1920, height=1080, fps=25.0, frames=7)
    rd = video.FFmpegVideoReader("clip.mp4", "nv12", meta=meta)
    assert rd.cmd == cmd and rd.frame_shape == (1620, 1920) and rd.yuv == yuv.YUVFormat("nv12")
    assert (rd.width, rd.height, rd.fps, len(rd), rd.pix_fmt) == (1920, 1080, 25.0, 7, "nv12")
    rd = video.FFmpegVideoReader("a b/clip.mp4", meta=meta)
    assert rd.cmd == video.ffmpeg_reader_cmd("a b/clip.mp4") and rd.frame_shape == (1080, 1920, 3) and rd.yuv is None
    with pytest.raises(ValueError):
        video.FFmpegVideoReader("clip.mp4", "yuv420p", meta=dict(width=1919, height=1080))


# ------------------------------------------------------------------------------- rs.py, yuv.py, ABI
def test_rs_flags_and_formats(tmp_path):
    import rs
    opt = rs.build_parser().parse_args([])
    assert (opt.pix_fmt, opt.yuv_matrix, opt.yuv_range, opt.yuv_siting) == ("rgb24", None, None, None)
    opt = rs.build_parser().parse_args(["--pix_fmt", "nv12", "--yuv_matrix", "bt601", "--yuv_range", "full",
                                        "--yuv_siting", "center"])
    assert (opt.pix_fmt, opt.yuv_matrix, opt.yuv_range, opt.yuv_siting) == ("nv12", "bt601", "full", "center")
    for bad in (["--pix_fmt", "yuv444p"], ["--yuv_matrix", "bt2020"], ["--yuv_range", "tv"], ["--yuv_siting", "top"]):
        with pytest.raises(SystemExit):
            rs.build_parser().parse_args(bad)

    class Src:
        def __init__(self, fmt=None):
            self.yuv, self.pix_fmt = fmt, (fmt.pix_fmt if fmt else "rgb24")

    none = dict(pix_fmt="rgb24", yuv_matrix=None, yuv_range=None, yuv_siting=None)
    header = yuv.YUVFormat("i420", "auto", True, "center")
    # rgb in, bgr out: today's path
    assert rs.video_formats(none, Src(), tmp_path / "o.bgr") == ("rgb24", None, "bgr24", None)
    assert rs.video_formats(none, Src(), tmp_path / "o.mp4") == ("rgb24", None, "bgr24", None)
    # the .y4m header wins, and the output inherits it
    assert rs.video_formats(none, Src(header), tmp_path / "o.y4m") == ("yuv420p", header, "yuv420p", header)
    got = rs.video_formats(none, Src(header), tmp_path / "o.nv12")
    assert got[2:] == ("nv12", yuv.YUVFormat("nv12", "auto", True, "center"))
    assert rs.video_formats(none, Src(header), tmp_path / "o.raw")[2:] == ("bgr24", None)
    # ... unless a flag is given
    flags = dict(none, yuv_matrix="bt601", yuv_range="limited", yuv_siting="left")
    want = yuv.YUVFormat("i420", "bt601", False, "left")
    assert rs.video_formats(flags, Src(header), tmp_path / "o.yuv") == ("yuv420p", want, "yuv420p", want)
    # a container follows --pix_fmt
    got = rs.video_formats(dict(none, pix_fmt="nv12"), Src(yuv.YUVFormat("nv12")), tmp_path / "o.mp4")
    assert got == ("nv12", yuv.YUVFormat("nv12"), "nv12", yuv.YUVFormat("nv12"))
    assert rs.video_formats(none, Src(), tmp_path / "o.y4m")[2:] == ("yuv420p", yuv.YUVFormat("i420"))


def test_format_and_cpu_tensors_refused():
    auto = yuv.YUVFormat()
    assert (auto.layout, auto.matrix, auto.full_range, auto.siting, auto.pix_fmt) == ("i420", "auto", False, "left", "yuv420p")
    assert auto.resolved(720).matrix == "bt709" and auto.resolved(718).matrix == "bt601"
    assert yuv.YUVFormat(matrix="bt601").resolved(2160).matrix == "bt601"
    assert yuv.YUVFormat.of_pix_fmt("nv12").layout == "nv12"
    for kw in (dict(layout="yv12"), dict(matrix="bt2020"), dict(siting="top")):
        with pytest.raises(ValueError):
            yuv.YUVFormat(**kw)
    assert yuv.frame_bytes(6, 10) == 90 == Y.frame_bytes(6, 10)
    for h, w in ((5, 10), (6, 9), (0, 2)):
        with pytest.raises(ValueError):
            yuv.frame_bytes(h, w)
    with pytest.raises(RuntimeError, match="HIP"):
        yuv.yuv420_to_rgb(torch.zeros(90, dtype=torch.uint8), 6, 10)
    with pytest.raises(RuntimeError, match="HIP"):
        yuv.rgb_to_yuv420(torch.zeros((1, 3, 6, 10), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP"):
        yuv.rgb_to_yuv420(np.zeros((1, 3, 6, 10), dtype=np.uint8))


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "isr.h"
#define F(m) printf(#m " %zu\n", offsetof(isr_yuv_desc, m))
int main(void) {
  printf("size %zu\n", sizeof(isr_yuv_desc));
  F(n); F(h); F(w); F(layout); F(siting); F(full_range); F(fwd); F(inv); F(src); F(dst);
  printf("consts %d %d %d %d %d %d %d\n", ISR_YUV_BITS, ISR_YUV_BT601, ISR_YUV_BT709, ISR_YUV_I420, ISR_YUV_NV12,
         ISR_YUV_SITING_LEFT, ISR_YUV_SITING_CENTER);
  return 0;
}
"""


def test_desc_layout_matches_c(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                   check=True)
    lines = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines()
    c = {ln.split()[0]: ln.split()[1:] for ln in lines}
    assert int(c["size"][0]) == ctypes.sizeof(_lib.IsrYuvDesc)
    assert [name for name, _ in _lib.IsrYuvDesc._fields_] == ["n", "h", "w", "layout", "siting", "full_range", "fwd",
                                                              "inv", "src", "dst"]
    for name, _ in _lib.IsrYuvDesc._fields_:
        assert getattr(_lib.IsrYuvDesc, name).offset == int(c[name][0]), name
    assert [int(v) for v in c["consts"]] == [Y.BITS, 0, 1, 0, 1, 0, 1]
    assert (yuv.MATRICES, yuv.LAYOUTS, yuv.SITINGS) == (tuple(Y.MATRICES), Y.LAYOUTS, Y.SITINGS)
