"""Static resource check of the 10-bit colour kernels (csrc/yuv16.hip), wherever hipcc is (no GPU): both
kernels, in both sitings and each RGB kind of their direction, must compile for gfx950 without scratch
(the per-thread sample arrays stay in registers), without VGPR or SGPR spills and without LDS."""
import os

import pytest

from image_super_resolution_amd import _build


@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason="needs hipcc")
def test_yuv16_kernel_resources():
    asm, remarks = _build.device_asm(_build.CSRC / "yuv16.hip", remarks=True)
    # csrc/yuv.hip's shift_clamp8: the packed shift-and-saturate forms gave wrong results on the MI355X; the
    # clamp-before-shift order of yuv16.hip keeps the compiler from forming any of them
    assert "v_ashr_pk_" not in asm
    res = _build.kernel_resources(_build.CSRC / "yuv16.hip", remarks=remarks)
    for kernel in ("yuv420_to_rgb16_kernel", "rgb_to_yuv420_16_kernel"):
        found = {k: v for k, v in res.items() if kernel in k}
        assert len(found) == 4, f"{kernel}: expected 2 sitings x 2 RGB kinds, found {sorted(found)}"
        for name, r in sorted(found.items()):
            print(f"{name}: VGPRs {r['VGPRs']}, TotalSGPRs {r['TotalSGPRs']}, "
                  f"occupancy {r['Occupancy [waves/SIMD]']} waves/SIMD")
            assert int(r["ScratchSize [bytes/lane]"]) == 0, r
            assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
            assert int(r["LDS Size [bytes/block]"]) == 0, r
    assert len(res) == 8, sorted(res)
