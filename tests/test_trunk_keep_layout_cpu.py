"""The kept-tile layout of the trunk kernel (csrc/trunk_keep.h), no GPU: a host-only program
(tests/trunk_keep_layout_check.cpp) includes the header the kernel uses and checks exhaustively, for
buffer rows of 36, 54, 130 and 8194 pixels, that every tile-epilogue register lands on the LDS unit
the halo LDS-DMA fills from the same pixel and channel half, that the 1,024 interior units and the 200
ring units are disjoint and together exactly the units of the 612 halo pixels, and that each ring
unit's source offset is the LDS-DMA's for that unit.  The program is built plain and with the address
and undefined-behaviour sanitizers; both must agree."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "trunk_keep_layout_check.cpp"
CSRC = ROOT / "image_super_resolution_amd" / "csrc"
GXX = shutil.which("g++")


def _run(tmp_path, name, extra):
    exe = tmp_path / name
    cmd = [GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra, "-I", str(CSRC), str(SRC), "-o",
           str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stderr.strip(), r.stderr[-4000:]
    return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]


@pytest.mark.skipif(GXX is None, reason="needs g++")
def test_kept_tile_layout_matches_the_halo_dma(tmp_path):
    plain = _run(tmp_path, "layout", [])
    san = _run(tmp_path, "layout_san",
               ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert plain == san, "the sanitizer build computes something else"
    # per wp: 4 waves x 4 rows x 32 x 2 interior units, 200 ring units, 2 x 612 units covered
    assert plain == [(wp, 1024, 200, 1224) for wp in (36, 54, 130, 8194)]
