"""Static resource check of the blur kernel (csrc/blur.hip), wherever hipcc is (no GPU): it must
compile for gfx950 without scratch (the median's window and the taps stay in registers), without
VGPR or SGPR spills, and with no more than 80 KiB of LDS per block (two blocks per CU)."""
import os

import pytest

from image_super_resolution_amd import _build

LDS_LIMIT = 80 * 1024


@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason="needs hipcc")
def test_blur_kernel_resources():
    res = {k: v for k, v in _build.kernel_resources(_build.CSRC / "blur.hip").items() if "blur_u8_kernel" in k}
    assert len(res) == 1, f"blur_u8_kernel not found: {sorted(res)}"
    (r,) = res.values()
    print(f"blur_u8_kernel: VGPRs {r['VGPRs']}, TotalSGPRs {r['TotalSGPRs']}, LDS {r['LDS Size [bytes/block]']} B, "
          f"occupancy {r['Occupancy [waves/SIMD]']} waves/SIMD")
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert 0 < int(r["LDS Size [bytes/block]"]) <= LDS_LIMIT, r
