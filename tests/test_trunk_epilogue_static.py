"""Static check of the trunk kernel's specialised tile epilogues (csrc/trunk.hip run_tile), wherever
hipcc is (no GPU): in both production instantiations (fp16 and bf16 storage) every store-holding
basic block of a specialised body (growth, final, final + s2, final + r2; full and ragged tiles)
holds at most 5 VALU instructions per stored value and converts with the packed fp32 -> 16-bit
instruction.  The blocks are found by the marker comment each specialised body emits
(tools/trunk_isa_mix.py store_blocks)."""
import os
import sys
from pathlib import Path

import pytest

from image_super_resolution_amd import _build

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import trunk_isa_mix  # noqa: E402

PRODUCTION_FORMS = ("growth", "final", "final_r2")  # what ResNet / EResNet tables hold


@pytest.fixture(scope="module")
def store_blocks():
    return trunk_isa_mix.production_store_blocks()


@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason="needs hipcc")
def test_specialised_epilogues_are_lean_and_use_the_packed_convert(store_blocks):
    assert set(store_blocks) == {"fp16", "bf16"}, f"production trunk_kernel instantiations not found: {sorted(store_blocks)}"
    for storage, blocks in store_blocks.items():
        spec = [b for b in blocks if b["form"] is not None]
        for b in blocks:
            print(f"trunk_kernel {storage}: " + trunk_isa_mix.fmt_store_block(b, storage))
        found = {b["form"] for b in spec}
        for form in PRODUCTION_FORMS:
            for full in (True, False):
                assert (form, full) in found, f"{storage}: no store-holding block of the {form} body (full tile: {full})"
        cvt = trunk_isa_mix.PACKED_CVT[storage]
        for b in spec:
            assert b["valu_per_value"] <= 5.0, (storage, b["form"], b["valu"], b["values"])
            # one packed convert per two stored values, and no scalar convert left beside it
            assert b["ops"].get(cvt, 0) * 2 == b["values"], (storage, b["form"], dict(b["ops"]))
            if storage == "fp16":
                assert b["ops"].get("v_cvt_f16_f32", 0) == 0, (storage, b["form"], dict(b["ops"]))
        # every 16-byte epilogue store of a specialised body lies in a marked block: the marked blocks
        # of one form hold the whole tile's stores (4 rows x cout / 8 stores per lane)
        for b in spec:
            want = 8 if b["form"][0] == "growth" else 16
            assert b["stores"] == want, (storage, b["form"], b["stores"])
