"""The kept-tile layout of the trunk kernel (csrc/trunk_keep.h), no GPU: a host-only program
(tests/trunk_keep_layout_check.cpp) includes the header the kernel uses and checks exhaustively, for
buffer rows of 36, 54, 130 and 8194 pixels, that every tile-epilogue register lands on the LDS unit
the halo LDS-DMA fills from the same pixel and channel half, that the 1,024 interior units and the 200
ring units are disjoint and together exactly the units of the 612 halo pixels, and that each ring
unit's source offset is the LDS-DMA's for that unit.  The program is built plain and with the address
and undefined-behaviour sanitizers; both must agree (tests/host_program.py)."""
from pathlib import Path

import pytest

import host_program

SRC = Path(__file__).resolve().parent / "trunk_keep_layout_check.cpp"


@pytest.mark.skipif(host_program.GXX is None, reason="needs g++")
def test_kept_tile_layout_matches_the_halo_dma(tmp_path):
    (out,) = host_program.run_plain_and_sanitized(SRC, tmp_path, timeout=120)
    rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    # per wp: 4 waves x 4 rows x 32 x 2 interior units, 200 ring units, 2 x 612 units covered
    assert rows == [(wp, 1024, 200, 1224) for wp in (36, 54, 130, 8194)]
