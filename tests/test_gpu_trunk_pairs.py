"""Growth pairs of the trunk kernel (trunk.hip run_tile PH 1 / 2: two growth convs of an RDB as one
item per tile over once-staged chunks): the chain must reproduce the per-conv launches of the same
descriptors BIT FOR BIT, in fp16 and bf16, with and without the acquire fence, three different inputs
back to back on one plan, and no dependency wait may give up.  What the prep kernel decided is read
from the geometry word r0 (the number of paired layers).

Whole generators: one tile (every hand-off self-dependent), 3 x 3 tiles (one with all eight
neighbours), ragged tiles across an RRDB boundary, 546 tiles on 512 workgroups (pair-major order,
prefetch across a tile boundary).  Hand-built growth-only chains on 192-channel buffers: per-layer
slopes, a pair followed by a single layer, a chain that is one pair, neighbours that must not pair,
a geometry the order rule (csrc/trunk_pairs.h) refuses, and the ISR_TRUNK_PAIRS switch (read once
per process, so each value runs in a child process: this file's __main__)."""
import json
import os

import pytest
import torch

import trunk_harness as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


# ---------------------------------------------------------------- whole generators
@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w,blocks", [(1, 16, 32, 1), (1, 48, 96, 1), (2, 36, 52, 2), (3, 224, 416, 1)],
                         ids=["one_tile", "3x3_tiles", "ragged", "546_tiles"])
def test_generator_pairs_bitwise_equal_per_conv_launches(n, h, w, blocks, f16, acquire):
    gw, xs, refs = H.model_case(n, h, w, blocks, f16, 3)
    outs, r0 = H.run_plan(gw, xs, chain=True, acquire=acquire)
    assert r0 == 4 * 3 * blocks, f"paired layers {r0}: every RDB has two growth pairs"
    for out, ref in zip(outs, refs):
        assert torch.equal(out, ref), f"chain differs from the per-conv launches: max {(out - ref).abs().max().item()}"


# ---------------------------------------------------------------- hand-built growth-only chains
# every layer reads channels [0, cin) of its buffer and writes 32 channels at y_coff of the same
# buffer: H.growth(cin, y_coff, slope, buffer index)
RDB4 = (H.growth(64, 64, 0.2), H.growth(96, 96, 0.35), H.growth(128, 128, 0.5), H.growth(160, 160, 0.65))
XSEEDS = ((20, 21), (27, 28), (34, 35))  # [input][buffer]


def _case(layers, in_ch=(64,)):
    return H.ChainCase(layers, in_ch, wseed=5, xseeds=XSEEDS)


CHAINS = {
    # name: (case, expected paired layers)
    "rdb4_slopes": (_case(RDB4), 4),
    "pair_then_single": (_case(RDB4[:3]), 2),
    "one_pair": (_case(RDB4[:2]), 2),
    "same_cin": (_case((H.growth(64, 64, 0.2), H.growth(64, 96, 0.35))), 0),
    "cin_plus_64": (_case((H.growth(64, 64, 0.2), H.growth(128, 128, 0.35))), 0),
    "other_buffer": (_case((H.growth(64, 64, 0.2), H.growth(96, 96, 0.35, 1)), (64, 96)), 0),
}


def _check_chain(name, n, h, w, f16, acquire, want=None):
    case, want_case = CHAINS[name]
    r0 = H.check_chain(H.chain_case(case, n, h, w, f16), 0, acquire)
    assert r0 == (want_case if want is None else want), f"paired layers {r0}"
    return r0


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_hand_built_chains(name, f16, acquire):
    """2 x 3 ragged tiles per image, 2 images."""
    _check_chain(name, 2, 36, 52, f16, acquire)


@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
def test_rdb4_slopes_546_tiles(f16):
    """More tiles than workgroups: pair-major order with a different slope per layer."""
    _check_chain("rdb4_slopes", 3, 224, 416, f16, False)


@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
def test_order_rule_refuses_wide_rows(f16):
    """768 tiles in rows of 256 on 512 workgroups: 2 (nbx + 2) > G, so the prep kernel must not pair
    and the stream is the unpaired one."""
    props = torch.cuda.get_device_properties(0)
    assert 2 * props.multi_processor_count < 2 * (256 + 2), "the case needs a grid the rule refuses"
    _check_chain("one_pair", 1, 48, 8192, f16, False, want=0)


@pytest.mark.parametrize("mode,want", [(0, 0), (1, 2), (2, 4)], ids=["off", "long", "all"])
def test_switch_values(mode, want):
    """ISR_TRUNK_PAIRS: 0 pairs nothing, 1 only the pair sharing 8 chunks (layers 2, 3), 2 both."""
    assert H.switch_child(__file__, {"ISR_TRUNK_PAIRS": str(mode)}) == {"fp16": want, "bf16": want}


if __name__ == "__main__":
    from image_super_resolution_amd import _build, _lib
    _build.build()
    _lib.load()
    mode = int(os.environ["ISR_TRUNK_PAIRS"])
    res = {}
    for f16 in (True, False):
        res["fp16" if f16 else "bf16"] = _check_chain("rdb4_slopes", 2, 36, 52, f16, False,
                                                      want={0: 0, 1: 2, 2: 4}[mode])
    print(json.dumps(res))
