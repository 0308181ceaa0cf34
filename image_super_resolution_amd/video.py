"""Video super-resolution path (BASELINE configs[4]).

Mirrors the reference's video branch — rs.py:54-76 (decode → Normalize → model
→ TanhToArrayImage → RGB2BGR → FFMPEG_recorder), utils/datasets.py:431-463
(`dataset_for_inference`: frames as uint8 CHW, fps from the container) and
utils/ffmpeg.py:28-140 (`FFMPEG_recorder`: raw bgr24 frames piped to an ffmpeg
encoder, bitrate ∝ output megapixels) — rebuilt around the MI355X path:

* the per-batch forward (uint8 HWC RGB in → Normalize fused into the head
  kernel → RRDB trunk → tail + TanhToArrayImage fused → BGR HWC uint8 out) is
  one `GeneratorPlan` whose ~245 kernel launches, plus the layout copies on
  either side, are captured once into a HIP graph and replayed per batch
  (torch.cuda.CUDAGraph over the HIP stream: no per-frame CPU launch cost);
* frames are staged through pinned host buffers, two output slots deep, so the
  device→host copy of batch i and the encoder write of batch i-1 overlap the
  forward of batch i+1; encoding runs on a writer thread;
* decode / encode use the ffmpeg binary through raw pipes when it is installed
  (as the reference does); `RawVideoReader` / `RawRecorder` read and write
  headerless rgb24 / bgr24 files and `SyntheticVideo` generates frames, so the
  pipeline is testable and benchmarkable on a machine without ffmpeg;
* opt-in, frames cross the host boundary as 8-bit YUV 4:2:0 (`pix_fmt_in` / `pix_fmt_out` of
  yuv420p or nv12: half the bytes of rgb24 / bgr24, what decoders produce and encoders take) and the
  colour conversion runs in the captured graph (yuv.py, csrc/yuv.hip) in place of the layout copies;
  `Y4MReader` / `Y4MRecorder` read and write YUV4MPEG2 (.y4m) files, `RawYUVReader` headerless
  I420 / NV12, again without ffmpeg;
* a side whose pix_fmt is yuv420p10le or p010le carries 10-bit samples in 16-bit words (what HEVC Main10
  and AV1 decoders hand over): its frames convert straight to the head's normalised fp32 input and
  straight from the tail's fp32 tanh (csrc/yuv16.hip), in the same graph, with no 8-bit step between.

Reference bugs deliberately not reproduced: the frame is
normalised once (rs.py:63 normalises before a TorchScript Model that normalises
again) and quantised to uint8 once (rs.py:65 re-applies TanhToArrayImage to
the model's uint8 output); frames are read in order (the reference's
DataLoader uses shuffle=True but `__getitem__` ignores the index).
"""
from __future__ import annotations

import ctypes
import math
import platform
import queue
import shutil
import subprocess
import threading
from pathlib import Path
from fractions import Fraction
from typing import Iterator

import numpy as np
import torch

from . import _lib, engine, yuv as yuvmod
from .yuv import YUVFormat

RGB_FORMATS = (".rgb", ".raw", ".rgb24")       # headerless rgb24 input
YUV_FORMATS = (".y4m", ".yuv", ".i420", ".nv12")  # YUV4MPEG2 and headerless I420 / NV12 input
VID_FORMATS = ('.mp4', '.avi', '.mkv', '.mov', '.wmv', '.flv', '.webm', '.mpeg', '.mpg', '.m4v', '.ts')


def have_ffmpeg() -> bool:
    return shutil.which("ffmpeg") is not None and shutil.which("ffprobe") is not None


# ----------------------------------------------------------------------------- sources
def ffmpeg_reader_cmd(src: str | Path, pix_fmt: str = "rgb24") -> list[str]:
    """FFmpegVideoReader's decoder argv: raw frames of `pix_fmt` (rgb24, yuv420p, nv12, yuv420p10le or
    p010le) to a pipe."""
    if pix_fmt != "rgb24" and pix_fmt not in yuvmod.PIX_FMTS:
        raise ValueError(f"unknown pix_fmt {pix_fmt!r}; rgb24, {', '.join(yuvmod.PIX_FMTS)}")
    return ["ffmpeg", "-v", "quiet", "-i", Path(src).as_posix(), "-f", "rawvideo", "-pix_fmt", pix_fmt, "pipe:"]


class FFmpegVideoReader:
    """Decoded uint8 HWC RGB frames of a video file via an ffmpeg rawvideo pipe
    (the role of torchvision's VideoReader in utils/datasets.py:431-453)."""

    def __init__(self, src: str | Path, pix_fmt: str = "rgb24", meta: dict | None = None):
        """`meta` (width, height and optionally fps, frames) stands in for the ffprobe call: the reader
        is then made without the binaries, which only iterating needs."""
        self.cmd = ffmpeg_reader_cmd(src, pix_fmt)
        self.pix_fmt = pix_fmt
        src = Path(src)
        if meta is not None:
            self.width, self.height = int(meta["width"]), int(meta["height"])
            self.fps, self.total_frame = float(meta.get("fps", 30.0)), int(meta.get("frames", 0))
        else:
            self._probe(src)
        self.src = src
        self.yuv = None
        self.frame_shape = (self.height, self.width, 3)
        if pix_fmt != "rgb24":  # frames as [3h/2, w] bytes; the stream's own tags are not read: YUVFormat's defaults
            self.yuv = YUVFormat.of_pix_fmt(pix_fmt)
            self.frame_shape = yuvmod.frame_shape(self.height, self.width, self.yuv.depth)  # 10 bits: [3h/2, 2w]

    def _probe(self, src: Path) -> None:
        if not have_ffmpeg():
            raise RuntimeError("FFmpegVideoReader needs the ffmpeg and ffprobe binaries")
        probe = subprocess.run(["ffprobe", "-v", "error", "-select_streams", "v:0", "-show_entries",
                                "stream=width,height,r_frame_rate,nb_frames,duration", "-of",
                                "default=noprint_wrappers=1", src.as_posix()],
                               capture_output=True, text=True, check=True).stdout
        meta = dict(line.split("=", 1) for line in probe.strip().splitlines() if "=" in line)
        self.width, self.height = int(meta["width"]), int(meta["height"])
        num, den = (meta.get("r_frame_rate", "30/1").split("/") + ["1"])[:2]
        self.fps = float(num) / float(den or 1)
        nb = meta.get("nb_frames", "N/A")
        dur = meta.get("duration", "N/A")
        self.total_frame = int(nb) if nb.isdigit() else (int(self.fps * float(dur)) if dur != "N/A" else 0)

    def __len__(self):
        return self.total_frame

    def __iter__(self) -> Iterator[np.ndarray]:
        proc = subprocess.Popen(self.cmd, stdout=subprocess.PIPE)
        n = math.prod(self.frame_shape)
        try:
            while True:
                buf = proc.stdout.read(n)
                if len(buf) < n:
                    break
                yield np.frombuffer(buf, np.uint8).reshape(self.frame_shape)
        finally:
            proc.stdout.close()
            proc.wait()


class RawVideoReader:
    """Headerless rgb24 frames (H x W x 3 uint8, back to back) from a file."""

    def __init__(self, src: str | Path, width: int, height: int, fps: float = 30.0):
        self.src, self.width, self.height, self.fps = Path(src), width, height, fps
        size = self.src.stat().st_size
        fb = width * height * 3
        if size % fb:
            raise ValueError(f"{src}: {size} bytes is not a whole number of {width}x{height} rgb24 frames")
        self.total_frame = size // fb

    def __len__(self):
        return self.total_frame

    def __iter__(self) -> Iterator[np.ndarray]:
        mm = np.memmap(self.src, np.uint8, "r", shape=(self.total_frame, self.height, self.width, 3))
        for i in range(self.total_frame):
            yield np.asarray(mm[i])


Y4M_MAGIC = b"YUV4MPEG2"
Y4M_SITING = {"420jpeg": "center", "420": "center", "420mpeg2": "left"}  # the C tag's value -> chroma siting
Y4M_TAG = {"center": "420jpeg", "left": "420mpeg2"}


def y4m_header(width: int, height: int, fps, yuv: YUVFormat) -> bytes:
    """The YUV4MPEG2 stream header of progressive 4:2:0 frames in `yuv`'s siting and range.  10-bit frames
    are tagged C420p10 (with ffmpeg's XYSCSS=420P10), which names no siting and is read as left: a
    center-sited 10-bit format is refused."""
    yuvmod.check_size(height, width)
    if yuv.layout != "i420":
        raise ValueError("a .y4m file holds planar I420 frames, not NV12")
    rate = Fraction(fps).limit_denominator(1001)
    rng = "FULL" if yuv.full_range else "LIMITED"
    if yuv.depth == 10:
        if yuv.siting != "left":
            raise ValueError("a 10-bit .y4m file (C420p10) has no tag for center chroma siting: use siting 'left'")
        tag = "420p10 XYSCSS=420P10"
    else:
        tag = Y4M_TAG[yuv.siting]
    return (f"YUV4MPEG2 W{width} H{height} F{rate.numerator}:{rate.denominator} Ip A1:1 C{tag} "
            f"XCOLORRANGE={rng}\n").encode("ascii")


def parse_y4m_header(line: bytes, depths=(8,)) -> dict:
    """width, height, fps and yuv (a YUVFormat, matrix "auto") of a YUV4MPEG2 header line.  8-bit
    progressive 4:2:0 only: any other C or I tag raises a ValueError naming it.  With 10 among `depths`,
    C420p10 is taken too: depth 10, siting left."""
    tags = line.decode("ascii", "replace").split()
    if not tags or tags[0] != Y4M_MAGIC.decode():
        raise ValueError("not a YUV4MPEG2 stream (no YUV4MPEG2 magic)")
    w = h = None
    fps, siting, full, depth = 30.0, "center", False, 8
    for t in tags[1:]:
        k, v = t[0], t[1:]
        if k == "W":
            w = int(v)
        elif k == "H":
            h = int(v)
        elif k == "F":
            num, _, den = v.partition(":")
            fps = float(num) / float(den or 1) if float(den or 1) else 30.0
        elif k == "I":
            if v not in ("p", "?"):
                raise ValueError(f"y4m: interlacing tag {t!r} is not supported (progressive Ip / I? only)")
        elif k == "C":
            if v == "420p10" and 10 in depths:
                siting, depth = "left", 10
            elif v not in Y4M_SITING or 8 not in depths:
                raise ValueError(f"y4m: chroma tag {t!r} is not supported (8-bit C420jpeg, C420, C420mpeg2 only)")
            else:
                siting, depth = Y4M_SITING[v], 8
        elif t.startswith("XCOLORRANGE="):
            full = t.split("=", 1)[1].upper() == "FULL"
    if w is None or h is None:
        raise ValueError("y4m: the header has no W / H tag")
    yuvmod.check_size(h, w)
    return {"width": w, "height": h, "fps": fps, "yuv": YUVFormat("i420", "auto", full, siting, depth)}


class Y4MReader:
    """The frames of a YUV4MPEG2 (.y4m) file as uint8 [3h/2, w] arrays (a frame's bytes in order: the Y
    plane's rows, then U, then V).  `yuv` holds the header's siting and range; a truncated last frame
    ends the stream.  A C420p10 file: frames of [3h/2, 2w] bytes, little-endian 16-bit words, `yuv.depth`
    10 and `pix_fmt` yuv420p10le."""
    pix_fmt = "yuv420p"

    def __init__(self, src: str | Path):
        self.src = Path(src)
        with open(self.src, "rb") as f:
            line = f.readline(4096)
            self._data0 = f.tell()
        meta = parse_y4m_header(line, depths=(8, 10))
        self.width, self.height, self.fps, self.yuv = meta["width"], meta["height"], meta["fps"], meta["yuv"]
        self.pix_fmt = self.yuv.pix_fmt
        self.frame_shape = yuvmod.frame_shape(self.height, self.width, self.yuv.depth)
        # "FRAME\n" carries no parameters in the files encoders write: the count is exact for those
        self.total_frame = (self.src.stat().st_size - self._data0) // (math.prod(self.frame_shape) + 6)

    def __len__(self):
        return self.total_frame

    def __iter__(self) -> Iterator[np.ndarray]:
        n = math.prod(self.frame_shape)
        with open(self.src, "rb") as f:
            f.seek(self._data0)
            while True:
                head = f.readline(4096)
                if not head.startswith(b"FRAME"):
                    break
                buf = f.read(n)
                if len(buf) < n:
                    break
                yield np.frombuffer(buf, np.uint8).reshape(self.frame_shape)


class RawYUVReader:
    """Headerless 4:2:0 frames (I420 or NV12, 3 h w / 2 bytes each, back to back) from a file, as uint8
    [3h/2, w] arrays; with depth 10 (yuv420p10le / p010le words) 3 h w bytes each, as [3h/2, 2w]."""

    def __init__(self, src: str | Path, width: int, height: int, fps: float = 30.0, layout: str = "i420",
                 depth: int = 8):
        self.src, self.width, self.height, self.fps = Path(src), width, height, fps
        self.yuv = YUVFormat(layout, depth=depth)
        self.pix_fmt = self.yuv.pix_fmt
        fb = yuvmod.frame_bytes(height, width, depth)
        size = self.src.stat().st_size
        if size % fb:
            raise ValueError(f"{src}: {size} bytes is not a whole number of {width}x{height} 4:2:0 frames"
                             + (f" of {depth} bits" if depth != 8 else ""))
        self.total_frame = size // fb
        self.frame_shape = yuvmod.frame_shape(height, width, depth)

    def __len__(self):
        return self.total_frame

    def __iter__(self) -> Iterator[np.ndarray]:
        mm = np.memmap(self.src, np.uint8, "r", shape=(self.total_frame, *self.frame_shape))
        for i in range(self.total_frame):
            yield np.asarray(mm[i])


class SyntheticVideo:
    """`frames` smooth moving uint8 RGB frames (benchmarks / tests; no decoder)."""

    def __init__(self, width: int, height: int, frames: int, fps: float = 30.0, seed: int = 0):
        self.width, self.height, self.total_frame, self.fps = width, height, frames, fps
        g = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
        self._base = [(np.sin(xx / (17 + 9 * c) + c) * np.cos(yy / (13 + 7 * c)) + 1) * 100 for c in range(3)]
        self._noise = g.integers(0, 40, size=(height, width, 3), dtype=np.uint8)

    def __len__(self):
        return self.total_frame

    def __iter__(self) -> Iterator[np.ndarray]:
        for i in range(self.total_frame):
            s = i % 32
            f = np.stack([np.roll(b, s, axis=1) for b in self._base], axis=-1).astype(np.uint8)
            yield f + self._noise


def open_video(src: str | Path, width: int | None = None, height: int | None = None, fps: float = 30.0,
               pix_fmt: str = "rgb24"):
    """`dataset_for_inference` equivalent: ffmpeg for container formats (decoding to `pix_fmt`), raw for
    .rgb/.raw, YUV4MPEG2 for .y4m, headerless I420 for .yuv/.i420 and NV12 for .nv12 (of 10-bit words when
    `pix_fmt` is yuv420p10le or p010le)."""
    src = Path(src)
    suffix = src.suffix.lower()
    if suffix in RGB_FORMATS:
        if not (width and height):
            raise ValueError("raw rgb24 input needs --video_size WxH")
        return RawVideoReader(src, width, height, fps)
    if suffix == ".y4m":
        return Y4MReader(src)
    if suffix in YUV_FORMATS:
        if not (width and height):
            raise ValueError("raw 4:2:0 input needs --video_size WxH")
        return RawYUVReader(src, width, height, fps, "nv12" if suffix == ".nv12" else "i420",
                            yuvmod.PIX_FMT_DEPTH.get(pix_fmt, 8))
    return FFmpegVideoReader(src, pix_fmt)


# ----------------------------------------------------------------------------- sinks
def _gpu_vendor() -> str:
    try:
        return "AMD" if torch.version.hip else ("NVIDIA" if torch.cuda.is_available() else "")
    except Exception:  # noqa: BLE001
        return ""


def _bitrate_mbps(dims, fps) -> float:
    """Target bitrate in Mbit/s (utils/ffmpeg.py:59-61): 20 Mbit/s for a 4K frame at 30 fps, scaled
    by the frame area and by the frame-rate ratio, which is never taken below 1."""
    rate_factor = round(fps / 30, 3)
    if rate_factor < 1:
        rate_factor = 1
    return round(20 * (math.prod(dims) / (3840 * 2160)) * rate_factor, 3)


def _srt_entry(index: int, t0: str, t1: str, text: str) -> str:
    return f"{index}\n{t0} --> {t1}\n{text}\n\n"


class FFMPEG_recorder:  # noqa: N801  (reference class name, utils/ffmpeg.py:28)
    """utils/ffmpeg.py:28-140: raw bgr24 frames piped into an ffmpeg encoder process.

    The public surface is the reference's (constructor arguments, `bitRate`, `cmd`,
    `subtitleContent`, writeFrame / writeSubtitle / addSubtitle / addAudio / stopRecorder) and so is
    what ffmpeg receives (tests/test_video_cpu.py pins the argv, bitrate and timecodes).  The encoder
    is hevc_vaapi on a Linux host with an AMD GPU when ffmpeg offers it (the reference's preference
    for that platform), else libx264."""

    def __init__(self, save_path=None, videoDimensions=(1280, 720), fps=30, codec: str | None = None,
                 dry_run: bool = False, pix_fmt: str = "bgr24", yuv: YUVFormat | None = None):
        self.save_path = save_path
        self.dimension = videoDimensions
        self.fps = fps
        if codec is None:
            amd_linux = platform.uname().system == "Linux" and _gpu_vendor() == "AMD"
            codec = "hevc_vaapi" if amd_linux and _has_encoder("hevc_vaapi") else "libx264"
        self.codec = codec
        out_path = save_path.replace(" ", "_") if save_path else save_path  # ffmpeg target without spaces
        self.countFrame = 0
        self.startTime = 0.
        self.bitRate = _bitrate_mbps(self.dimension, self.fps)
        self.subtitleContent = ''
        width, height = self.dimension
        if pix_fmt != "bgr24" and pix_fmt not in yuvmod.PIX_FMTS:
            raise ValueError(f"FFMPEG_recorder: pix_fmt {pix_fmt!r}: bgr24, {', '.join(yuvmod.PIX_FMTS)}")
        self.pix_fmt, self.yuv = pix_fmt, None
        tags = []
        if pix_fmt != "bgr24":  # 4:2:0 frames through the pipe: ffmpeg converts nothing, so tell it what they are
            self.yuv = (yuv or YUVFormat.of_pix_fmt(pix_fmt)).resolved(height)
            if self.yuv.pix_fmt != pix_fmt:
                raise ValueError(f"FFMPEG_recorder: pix_fmt {pix_fmt!r} with a {self.yuv.pix_fmt} YUVFormat")
            tags = ['-colorspace', 'bt709' if self.yuv.matrix == 'bt709' else 'smpte170m',
                    '-color_range', 'pc' if self.yuv.full_range else 'tv',
                    '-chroma_sample_location', self.yuv.siting]
        source = ['-s', f'{width}x{height}', '-pixel_format', pix_fmt, *tags, '-f', 'rawvideo', '-r', f'{self.fps}',
                  '-i', 'pipe:']
        # a 10-bit pipe is encoded at 10 bits: the samples the network made are not rounded to 8 again
        sink_fmt = 'yuv420p10le' if self.yuv is not None and self.yuv.depth == 10 else 'yuv420p'
        sink = ['-vcodec', f'{self.codec}', '-pix_fmt', sink_fmt, *tags, '-b:v', f'{self.bitRate}M', f'{out_path}']
        self.cmd = ['ffmpeg', '-v', 'quiet', '-y', *source, *sink]
        self.process = None
        if dry_run:
            return
        if shutil.which("ffmpeg") is None:
            raise RuntimeError("FFMPEG_recorder needs the ffmpeg binary (use RawRecorder without it)")
        self.process = subprocess.Popen(self.cmd, stdin=subprocess.PIPE)

    def writeFrame(self, image=None):  # noqa: N802
        """image: ndarray uint8 HWC BGR (or the [3h/2, w] bytes of a 4:2:0 frame of `pix_fmt`)."""
        self.process.stdin.write(np.ascontiguousarray(image).tobytes())

    @staticmethod
    def second_to_timecode(x=0.) -> str:
        """SubRip timecode HH:MM:SS,mmm of x seconds, milliseconds truncated (utils/ffmpeg.py:81-89;
        float divmod is exact, so x mod 1 equals the reference's chained remainders)."""
        whole, frac = divmod(x, 1)
        hours, rest = divmod(int(whole), 3600)
        minutes, seconds = divmod(rest, 60)
        return f"{hours:02d}:{minutes:02d}:{seconds:02d},{int(frac * 1000.):03d}"

    def writeSubtitle(self, title='', fps=30):  # noqa: N802
        """One SubRip cue of 1/fps seconds at the running clock (utils/ffmpeg.py:91-100)."""
        t0 = self.startTime
        self.startTime = t0 + 1 / fps
        self.subtitleContent += _srt_entry(self.countFrame, self.second_to_timecode(t0),
                                           self.second_to_timecode(self.startTime), title or "UTC2")
        self.countFrame += 1

    def addSubtitle(self, hardSubtitle=False):  # noqa: N802,N803
        """Mux (or burn in, hardSubtitle) the collected cues into '<name>with_sub.mp4'."""
        muxed = self.save_path.replace('.mp4', 'with_sub.mp4')
        srt = muxed.replace('.mp4', '.srt')
        Path(srt).write_text(self.subtitleContent)
        head = ["ffmpeg", "-hide_banner", "-i", self.save_path]
        if hardSubtitle:
            tail = ["-c:v", "copy", "-vf", f"subtitles={srt}"]
        else:
            tail = ["-i", srt, "-c:v", "copy", "-c:s", "mov_text", "-metadata:s:s:0", "language=eng"]
        return subprocess.run([*head, *tail, muxed])

    def addAudio(self, audio_src):  # noqa: N802
        """Copy the video stream and take the audio of `audio_src` into '<name>_audio.mp4'; 0 when
        there is no such file, else 1."""
        src = Path(audio_src)
        if not src.is_file():
            return 0
        target = self.save_path.replace(".mp4", "_audio.mp4")
        streams = ["-c:v", "copy", "-map", "0:v", "-map", "1:a"]
        subprocess.run(["ffmpeg", "-i", self.save_path, "-i", src.as_posix(), *streams, "-y", target])
        return 1

    def stopRecorder(self):  # noqa: N802
        if self.process is None:
            return
        self.process.stdin.close()
        self.process.wait()


def _has_encoder(name: str) -> bool:
    if shutil.which("ffmpeg") is None:
        return False
    try:
        out = subprocess.run(["ffmpeg", "-hide_banner", "-encoders"], capture_output=True, text=True, timeout=10).stdout
    except Exception:  # noqa: BLE001
        return False
    return f" {name} " in out


class RawRecorder:
    """Writes headerless bgr24 frames to a file (FFMPEG_recorder's pipe payload)."""

    def __init__(self, save_path, videoDimensions=(1280, 720), fps=30):  # noqa: N803
        self.save_path, self.dimension, self.fps = str(save_path), videoDimensions, fps
        self._f = open(self.save_path, "wb")
        self.frames = 0

    def writeFrame(self, image):  # noqa: N802
        self._f.write(np.ascontiguousarray(image).tobytes())
        self.frames += 1

    def stopRecorder(self):  # noqa: N802
        self._f.close()

    def addAudio(self, audio_src):  # noqa: N802
        return 0


class Y4MRecorder:
    """Writes 4:2:0 I420 frames to a YUV4MPEG2 (.y4m) file, which ffmpeg, x264, x265, SVT-AV1 and aomenc
    read: the header (size, rate, the C tag of `yuv`'s siting, XCOLORRANGE), then FRAME + the frame's
    bytes."""

    def __init__(self, save_path, videoDimensions=(1280, 720), fps=30, yuv: YUVFormat | None = None):  # noqa: N803
        self.save_path, self.dimension, self.fps = str(save_path), videoDimensions, fps
        self.yuv = yuv or YUVFormat()
        width, height = videoDimensions
        header = y4m_header(width, height, fps, self.yuv)
        self._bytes = yuvmod.frame_bytes(height, width, self.yuv.depth)
        self._f = open(self.save_path, "wb")
        self._f.write(header)
        self.frames = 0

    def writeFrame(self, image):  # noqa: N802
        buf = np.ascontiguousarray(image).tobytes()
        if len(buf) != self._bytes:
            raise ValueError(f"Y4MRecorder: a frame of {len(buf)} bytes, expected {self._bytes}")
        self._f.write(b"FRAME\n")
        self._f.write(buf)
        self.frames += 1

    def stopRecorder(self):  # noqa: N802
        self._f.close()

    def addAudio(self, audio_src):  # noqa: N802
        return 0


class NullRecorder:
    """Counts frames (benchmarks: measures the pipeline without an encoder)."""

    def __init__(self, *a, **k):
        self.frames = 0

    def writeFrame(self, image):  # noqa: N802
        self.frames += 1

    def stopRecorder(self):  # noqa: N802
        pass

    def addAudio(self, audio_src):  # noqa: N802
        return 0


# ----------------------------------------------------------------------------- the GPU pipeline
class FrameUpscaler:
    """uint8 HWC RGB frame batches → uint8 HWC BGR super-resolved frames on the
    HIP generator, one captured HIP graph per batch geometry.  `pix_fmt_in` / `pix_fmt_out` of yuv420p
    or nv12 (independently) make that side 8-bit 4:2:0 frames of `yuv_in` / `yuv_out` (a YUVFormat; by
    default limited range, left siting, the matrix by the frame's height), converted by libisr's colour
    kernels inside the same graph.  yuv420p10le / p010le make that side 10-bit frames in 16-bit words
    ([3h/2, 2w] bytes): a 10-bit input converts straight to the head's normalised fp32 input (the plan is
    built with x_u8=False), a 10-bit output straight from the tail's fp32 tanh (out_u8=False), so no
    8-bit value stands between the frame and the network on such a side.

    `gw` is an engine.GeneratorWeights (tiler.runner_for(model).gw); `mean` /
    `std` the Normalize constants fused into the head kernel."""

    def __init__(self, gw: engine.GeneratorWeights, height: int, width: int, batch: int = 1, mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225), device="cuda", graph: bool = True, pix_fmt_in: str = "rgb24",
                 pix_fmt_out: str = "bgr24", yuv_in: YUVFormat | None = None, yuv_out: YUVFormat | None = None):
        if pix_fmt_in != "rgb24" and pix_fmt_in not in yuvmod.PIX_FMTS:
            raise ValueError(f"pix_fmt_in {pix_fmt_in!r}: rgb24, {', '.join(yuvmod.PIX_FMTS)}")
        if pix_fmt_out != "bgr24" and pix_fmt_out not in yuvmod.PIX_FMTS:
            raise ValueError(f"pix_fmt_out {pix_fmt_out!r}: bgr24, {', '.join(yuvmod.PIX_FMTS)}")
        self.device = torch.device(device)
        self.batch, self.h, self.w = batch, height, width
        self.scale = 2 ** len(gw.scalers)
        self.pix_fmt_in, self.pix_fmt_out = pix_fmt_in, pix_fmt_out
        H, W = height * self.scale, width * self.scale
        self.out_hw = (H, W)
        # the 4:2:0 formats of the two sides, the matrix of each resolved by that side's own height
        self.yuv_in = self.yuv_out = None
        if pix_fmt_in != "rgb24":
            self.yuv_in = self._format(yuv_in, pix_fmt_in, height, width)
        if pix_fmt_out != "bgr24":
            self.yuv_out = self._format(yuv_out, pix_fmt_out, H, W)
        in10 = self.yuv_in is not None and self.yuv_in.depth == 10
        out10 = self.yuv_out is not None and self.yuv_out.depth == 10
        self.plan = engine.make_plan(gw, batch, height, width, self.device, not in10, not out10, mean, std)
        self.in_frame_shape = ((height, width, 3) if self.yuv_in is None
                               else yuvmod.frame_shape(height, width, self.yuv_in.depth))
        self.out_frame_shape = (H, W, 3) if self.yuv_out is None else yuvmod.frame_shape(H, W, self.yuv_out.depth)
        self.x_in = torch.zeros((batch, *self.in_frame_shape), dtype=torch.uint8, device=self.device)
        self.x = torch.empty((batch, 3, height, width), dtype=torch.float32 if in10 else torch.uint8, device=self.device)
        self.y = torch.empty(self.plan.out_shape, dtype=self.plan.out_dtype, device=self.device)
        self.y_out = torch.empty((batch, *self.out_frame_shape), dtype=torch.uint8, device=self.device)
        self.x_hwc = self.x_in if self.yuv_in is None else None  # the rgb-mode names of the staging tensors
        self.bgr = self.y_out if self.yuv_out is None else None
        self._lib = _lib.load()
        self._desc_in = self._desc_out = None
        with torch.cuda.device(self.device):
            if in10:  # 10-bit words -> the head's normalised fp32 input
                self._desc_in = yuvmod._desc16(batch, height, width, self.yuv_in, "norm_f32", self.x_in.data_ptr(),
                                               self.x.data_ptr(), mean, std)
            elif self.yuv_in is not None:
                self._desc_in = yuvmod._desc(batch, height, width, self.yuv_in, self.x_in.data_ptr(), self.x.data_ptr())
            if out10:  # the tail's fp32 tanh -> 10-bit words
                self._desc_out = yuvmod._desc16(batch, H, W, self.yuv_out, "tanh_f32", self.y.data_ptr(),
                                                self.y_out.data_ptr())
            elif self.yuv_out is not None:
                self._desc_out = yuvmod._desc(batch, H, W, self.yuv_out, self.y.data_ptr(), self.y_out.data_ptr())
        self.stream = torch.cuda.Stream(self.device)
        self.graph = None
        with torch.cuda.stream(self.stream):
            for _ in range(2):  # warm-up: lazily set kernel attributes, allocator pools
                self._body()
        self.stream.synchronize()
        if graph:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self._body()
            self.stream.synchronize()

    @staticmethod
    def _format(fmt: YUVFormat | None, pix_fmt: str, height: int, width: int) -> YUVFormat:
        fmt = fmt or YUVFormat.of_pix_fmt(pix_fmt)
        if fmt.pix_fmt != pix_fmt:
            raise ValueError(f"pix_fmt {pix_fmt!r} with a {fmt.pix_fmt} YUVFormat")
        yuvmod.check_size(height, width)
        return fmt.resolved(height)

    def _body(self):
        if self._desc_in is None:
            self.x.copy_(self.x_in.permute(0, 3, 1, 2))
        elif isinstance(self._desc_in, _lib.IsrYuv16Desc):
            _lib.check(self._lib.isr_yuv420_to_rgb_16(ctypes.byref(self._desc_in), yuvmod._stream()),
                       "isr_yuv420_to_rgb_16")
        else:  # 4:2:0 frames -> planar RGB, one kernel in place of the HWC→CHW copy
            _lib.check(self._lib.isr_yuv420_to_rgb_u8(ctypes.byref(self._desc_in), yuvmod._stream()),
                       "isr_yuv420_to_rgb_u8")
        self.plan.run(self.x, self.y)
        if self._desc_out is None:
            self.y_out.copy_(self.y.flip(1).permute(0, 2, 3, 1))  # RGB2BGR + CHW→HWC (utils/datasets.py RGB2BGR)
        elif isinstance(self._desc_out, _lib.IsrYuv16Desc):
            _lib.check(self._lib.isr_rgb_to_yuv420_16(ctypes.byref(self._desc_out), yuvmod._stream()),
                       "isr_rgb_to_yuv420_16")
        else:  # planar RGB -> 4:2:0 frames, in place of the flip / permute copy
            _lib.check(self._lib.isr_rgb_to_yuv420_u8(ctypes.byref(self._desc_out), yuvmod._stream()),
                       "isr_rgb_to_yuv420_u8")

    def run_async(self):
        """Forward of whatever x_in holds, on self.stream."""
        with torch.cuda.stream(self.stream):  # replay() launches on the current stream
            if self.graph is not None:
                self.graph.replay()
            else:
                self._body()

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        """Synchronous convenience: uint8 [b,h,w,3] RGB (host or device) → device [b,H,W,3] BGR; with a
        4:2:0 pix_fmt_in / pix_fmt_out that side is [b,3h/2,w] / [b,3H/2,W] frame bytes."""
        b = frames.shape[0]
        if b > self.batch or tuple(frames.shape[1:]) != self.in_frame_shape:
            raise ValueError(f"frames {tuple(frames.shape)} do not fit the plan {(self.batch, *self.in_frame_shape)}")
        with torch.cuda.stream(self.stream):
            self.x_in[:b].copy_(frames, non_blocking=True)
            if b < self.batch:
                self.x_in[b:].zero_()
        self.run_async()
        self.stream.synchronize()
        with torch.cuda.stream(self.stream):
            self.plan.verify()  # a persistent-chain give-up raises before the frames are handed out
        return self.y_out[:b]


class VideoUpscaler:
    """rs.py:54-76 as a streaming pipeline: source frames → FrameUpscaler →
    recorder.  Two pinned input and two pinned output slots: while the GPU runs
    batch i, the host decodes batch i+1 into the other input slot and the writer
    thread encodes batch i-1 from the other output slot."""

    def __init__(self, up: FrameUpscaler):
        self.up = up
        b = up.batch
        self.pin_in = [torch.empty((b, *up.in_frame_shape), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.pin_out = [torch.empty((b, *up.out_frame_shape), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.h2d_done = [torch.cuda.Event(), torch.cuda.Event()]
        self.d2h_done = [torch.cuda.Event(), torch.cuda.Event()]
        # per output slot: the chains' give-up counts, copied right after that batch's forward
        # (outside the captured graph) and checked by the writer before the batch is encoded
        self.chains = list(up.plan.chains)
        self.pin_state = [torch.zeros(max(1, len(self.chains)), dtype=torch.int32).pin_memory() for _ in range(2)]

    def run(self, frames, recorder, max_frames: int | None = None) -> int:
        """Upscale every frame of `frames` (iterable of uint8 HWC RGB arrays, or of [3h/2, w] 4:2:0 frames
        of the upscaler's pix_fmt_in) into `recorder.writeFrame` (BGR HWC, or a 4:2:0 frame of
        pix_fmt_out).  Returns the number of frames written."""
        up, b = self.up, self.up.batch
        q: queue.Queue = queue.Queue()
        out_free = [threading.Event(), threading.Event()]
        for e in out_free:
            e.set()
        err: list[BaseException] = []

        def writer():
            while True:
                item = q.get()
                if item is None:
                    return
                slot, n = item
                try:
                    if not err:
                        self.d2h_done[slot].synchronize()
                        for k, c in enumerate(self.chains):  # raises engine.ChainFailed
                            c.check_count(int(self.pin_state[slot][k]))
                        arr = self.pin_out[slot].numpy()
                        for i in range(n):
                            recorder.writeFrame(arr[i])
                except BaseException as e:  # noqa: BLE001
                    err.append(e)
                finally:
                    out_free[slot].set()

        th = threading.Thread(target=writer, daemon=True)
        th.start()
        written, slot = 0, 0
        it = iter(frames)
        try:
            while not err:
                self.h2d_done[slot].synchronize()  # the H2D copy of batch i-2 has left this input slot
                pin_np = self.pin_in[slot].numpy()
                n = 0
                while n < b and (max_frames is None or written + n < max_frames):
                    try:
                        pin_np[n] = next(it)
                    except StopIteration:
                        break
                    n += 1
                if n == 0:
                    break
                if n < b:
                    pin_np[n:] = 0
                out_free[slot].wait()  # the writer is done with batch i-2's output slot
                out_free[slot].clear()
                with torch.cuda.stream(up.stream):
                    up.x_in.copy_(self.pin_in[slot], non_blocking=True)
                    self.h2d_done[slot].record(up.stream)
                up.run_async()
                with torch.cuda.stream(up.stream):
                    for k, c in enumerate(self.chains):
                        c.snapshot(self.pin_state[slot][k:k + 1])
                    self.pin_out[slot].copy_(up.y_out, non_blocking=True)
                    self.d2h_done[slot].record(up.stream)
                q.put((slot, n))
                written += n
                slot ^= 1
        finally:
            q.put(None)
            th.join()
        if err:
            raise err[0]
        return written
