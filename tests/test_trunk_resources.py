"""Static resource check of the persistent trunk kernel (csrc/trunk.hip), wherever hipcc is (no
GPU): both production instantiations (fp16 and bf16 storage) must compile without scratch and
without VGPR spills, at 2 waves per SIMD (two 4-wave workgroups per CU).  The SGPR spill count
(SGPRs parked in VGPR lanes) is printed; DESIGN.md section 5 carries the figure."""
import os
import re
import subprocess

import pytest

from image_super_resolution_amd import _build

PROD = re.compile(r"trunk_kernelILb([01])EEE")


def _resource_lines():
    cmd = [_build.HIPCC, *_build.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           str(_build.CSRC / "trunk.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(":")
        if key == "Function Name":
            k = PROD.search(val)
            cur = out.setdefault("fp16" if k.group(1) == "1" else "bf16", {}) if k else None
        elif cur is not None:
            cur[key.strip()] = val.strip()
    return out


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
