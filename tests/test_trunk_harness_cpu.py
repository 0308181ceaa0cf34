"""What the trunk tests' shared harness (trunk_harness.py) copies or assumes, checked without a GPU:
its Python copy of the state layout, through which the pairs and keep tests read the geometry word
r0, must agree with the library's own size of the state (trunk.hip trunk_state_words = the record
offset + 1024 records of 16 words); every hand-built chain case must stay inside its buffers."""
import pytest

import test_gpu_trunk_epilogue as epilogue
import test_gpu_trunk_keep as keep
import test_gpu_trunk_pairs as pairs
import test_gpu_trunk_roles as roles
import trunk_harness as H

MAX_RECORDS, REC_WORDS = 1024, 16
# every (n, h, w) the five trunk files run, then a sweep over ragged sizes and tile counts on both
# sides of a multiple of 16
GEOMETRIES = [(2, 36, 52), (1, 128, 128), (16, 128, 128), (4, 256, 256), (4, 512, 512), (1, 540, 960), (10, 768, 768),
              (2, 32, 32), (1, 16, 32), (3, 224, 416), (1, 32, 64), (1, 20, 40), (1, 48, 96), (1, 48, 8192),
              (2, 24, 40), (2, 24, 32)]
GEOMETRIES += [(n, h, w) for n in (1, 3, 5) for h in (1, 17, 176, 177) for w in (31, 33, 352, 1000)]

CASES = {"roles.odd": roles.ODD_CASE}
CASES.update({f"epilogue.slope{s}": epilogue.slope_case(s) for s in epilogue.SLOPES})
CASES.update({f"pairs.{k}": v[0] for k, v in pairs.CHAINS.items()})
CASES.update({f"keep.{k}": v[0] for k, v in keep.CHAINS.items()})
CASES.update({f"keep.boundary{s}": keep.boundary_case(s) for s in keep.SHIFTS})


def test_record_offset_matches_the_library(built_lib):
    for n, h, w in GEOMETRIES:
        ha, wa = -(-h // H.TILE_H) * H.TILE_H, -(-w // H.TILE_W) * H.TILE_W
        ntiles = n * (ha // H.TILE_H) * (wa // H.TILE_W)
        assert H.rec_off(ntiles) + MAX_RECORDS * REC_WORDS == built_lib.isr_conv_chain_state_words(n, ha, wa), (n, h, w)
    assert H.GEO_R0 < H.GEO_WORDS


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_case_stays_inside_its_buffers(name):
    case = CASES[name]
    assert len(case.xseeds) == 3 and all(len(s) >= len(case.in_ch) for s in case.xseeds)
    assert all(0 < c <= H.BUF_CH and c % 16 == 0 for c in case.in_ch)
    for cin, cout, src, x_coff, dst, y_coff, slope, fold in case.layers:
        assert 0 <= src < len(case.in_ch) and 0 <= dst < len(case.in_ch)
        assert min(cin, cout) > 0 and all(v % 16 == 0 for v in (cin, cout, x_coff, y_coff))
        assert 0 <= x_coff and x_coff + max(cin, cout if fold else 0) <= H.BUF_CH, "read past the buffer"
        assert 0 <= y_coff and y_coff + cout <= H.BUF_CH, "write past the buffer"
    cin, _, src, x_coff = case.layers[0][:4]
    assert case.in_ch[src] >= x_coff + cin, "layer 0 reads channels no input fills"
