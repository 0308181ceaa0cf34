"""Static resource check of the persistent trunk kernel (csrc/trunk.hip), wherever hipcc is (no
GPU): both production instantiations (fp16 and bf16 storage) must compile without scratch and
without VGPR spills, at 2 waves per SIMD (two 4-wave workgroups per CU).  The SGPR spill count
(SGPRs parked in VGPR lanes) is printed; DESIGN.md section 5 carries the figure."""
import os
import re

import pytest

from image_super_resolution_amd import _build

PROD = re.compile(r"trunk_kernelILb([01])EEE")


def _resource_lines():
    found = ((PROD.search(name), r) for name, r in _build.kernel_resources(_build.CSRC / "trunk.hip").items())
    return {"fp16" if k.group(1) == "1" else "bf16": r for k, r in found if k}


@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason="needs hipcc")
def test_production_trunk_kernels_fit_the_register_file():
    res = _resource_lines()
    assert set(res) == {"fp16", "bf16"}, f"production trunk_kernel instantiations not found: {sorted(res)}"
    for storage, r in res.items():
        print(f"trunk_kernel {storage}: VGPRs {r['VGPRs']}, SGPRs Spill {r['SGPRs Spill']}, "
              f"TotalSGPRs {r['TotalSGPRs']}")
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (storage, r)
        assert int(r["VGPRs Spill"]) == 0, (storage, r)
        assert int(r["VGPRs"]) <= 256, (storage, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 2, (storage, r)
