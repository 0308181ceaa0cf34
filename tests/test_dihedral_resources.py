"""Static resource check of the dihedral kernels (csrc/dihedral.hip), wherever hipcc is (no GPU): each
compiles for gfx950 without scratch and without VGPR or SGPR spills, and with the LDS its design states:
one 64 x 68 B uint8 tile (4352 B) for isr_dihedral's uint8 form and the expand, one 32 x 33 fp32 tile
(4224 B) for its 4-byte form, four of those (16896 B) for the reduce."""
import os

import pytest

from image_super_resolution_amd import _build

LDS_BYTES = {
    "dihedral_kernelILi1E": 64 * 17 * 4,
    "dihedral_kernelILi4E": 32 * 33 * 4,
    "ensemble_expand_u8_kernel": 64 * 17 * 4,
    "ensemble_reduce_kernel": 4 * 32 * 33 * 4,
}


@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason="needs hipcc")
def test_dihedral_kernel_resources():
    res = _build.kernel_resources(_build.CSRC / "dihedral.hip")
    for name, lds in LDS_BYTES.items():
        found = [v for k, v in res.items() if name in k]
        assert len(found) == 1, f"{name} not found: {sorted(res)}"
        (r,) = found
        print(f"{name}: VGPRs {r['VGPRs']}, TotalSGPRs {r['TotalSGPRs']}, LDS {r['LDS Size [bytes/block]']} B, "
              f"occupancy {r['Occupancy [waves/SIMD]']} waves/SIMD")
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert 0 < int(r["LDS Size [bytes/block]"]) <= lds, (name, r)
