"""Static resource check of the colour kernels (csrc/yuv.hip), wherever hipcc is (no GPU): both
kernels, in both sitings, must compile for gfx950 without scratch (the per-thread sample arrays stay
in registers), without VGPR or SGPR spills and without LDS."""
import os

import pytest

from image_super_resolution_amd import _build


@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason="needs hipcc")
def test_yuv_kernel_resources():
    asm, remarks = _build.device_asm(_build.CSRC / "yuv.hip", remarks=True)
    # csrc/yuv.hip's shift_clamp8: the compiler's use of this instruction gave wrong bytes on the MI355X
    assert "v_ashr_pk_u8_i32" not in asm
    res = _build.kernel_resources(_build.CSRC / "yuv.hip", remarks=remarks)
    for kernel in ("yuv420_to_rgb_kernel", "rgb_to_yuv420_kernel"):
        found = {k: v for k, v in res.items() if kernel in k}
        assert len(found) == 2, f"{kernel}: expected the left and the center instantiation, found {sorted(found)}"
        for name, r in sorted(found.items()):
            print(f"{name}: VGPRs {r['VGPRs']}, TotalSGPRs {r['TotalSGPRs']}, "
                  f"occupancy {r['Occupancy [waves/SIMD]']} waves/SIMD")
            assert int(r["ScratchSize [bytes/lane]"]) == 0, r
            assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
            assert int(r["LDS Size [bytes/block]"]) == 0, r
