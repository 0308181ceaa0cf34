"""Kept tiles of the trunk kernel (trunk.hip run_tile, csrc/trunk_keep.h: phase 1 of a growth pair
leaves its two output planes and phase 2's weights in LDS; phase 2 fetches only the 100-pixel ring):
the chain must reproduce the per-conv launches of the same descriptors BIT FOR BIT, in fp16 and bf16,
with and without the acquire fence, three different inputs back to back on one plan (a stale ring
slot would show), and no dependency wait may give up.

Whole generators: one tile (the ring is all padding), 3 x 3 tiles (one with all eight neighbours),
ragged tiles across an RRDB boundary (the zeroed outside pixels must match in LDS), 546 tiles on 512
workgroups (phase 2 kept; a workgroup's next item is another tile).  Hand-built growth-only chains
on 192-channel buffers at 2 x 36 x 52: per-layer slopes, and a pair followed by a single layer.  In
the generators whose workgroups own one tile, every final conv is followed by a growth pair on the
same tile, whose first two chunks are kept the same way (absent with 546 tiles); a hand-built fold
final conv followed by a pair checks that form alone, and that a pair reading from 16, 32 or 48
channels into the final conv's output, whose chunks are other planes, keeps nothing.  The switch
ISR_TRUNK_KEEP is read once per process, so each value runs in a child process (this file's
__main__): under 0, 1 and 2 the chain must equal the per-conv result."""
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
# (the geometry word r0: kept tiles exist only where layers were paired)
@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w,blocks", [(1, 16, 32, 1), (1, 48, 96, 1), (2, 36, 52, 2), (3, 224, 416, 1)],
                         ids=["one_tile", "3x3_tiles", "ragged", "546_tiles"])
def test_generator_kept_tiles_bitwise_equal_per_conv_launches(n, h, w, blocks, f16, acquire):
    gw, xs, refs = H.model_case(n, h, w, blocks, f16, 11)
    outs, r0 = H.run_plan(gw, xs, chain=True, acquire=acquire)
    assert r0 == 4 * 3 * blocks, f"paired layers {r0}: every RDB has two growth pairs, each with a kept hand-off"
    for out, ref in zip(outs, refs):
        assert torch.equal(out, ref), f"chain differs from the per-conv launches: max {(out - ref).abs().max().item()}"


# ---------------------------------------------------------------- hand-built growth-only chains
# every layer reads channels [0, cin) of one 192-channel buffer and writes 32 channels at y_coff of
# the same buffer: H.growth(cin, y_coff, slope)
RDB4 = (H.growth(64, 64, 0.2), H.growth(96, 96, 0.35), H.growth(128, 128, 0.5), H.growth(160, 160, 0.65))
XSEEDS = ((40,), (41,), (42,))  # [input][buffer]
CHAINS = {
    # name: (case, expected paired layers)
    "rdb4_slopes": (H.ChainCase(RDB4, in_ch=(64,), wseed=9, xseeds=XSEEDS), 4),
    "pair_then_single": (H.ChainCase(RDB4[:3], in_ch=(64,), wseed=9, xseeds=XSEEDS), 2),
}


def _check_chain(name, n, h, w, f16, acquire):
    case, want = CHAINS[name]
    r0 = H.check_chain(H.chain_case(case, n, h, w, f16), 0, acquire)
    assert r0 == want, f"paired layers {r0}"
    return r0


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_hand_built_chains(name, f16, acquire):
    """2 x 3 ragged tiles per image, 2 images."""
    _check_chain(name, 2, 36, 52, f16, acquire)


# ---------------------------------------------------------------- a final conv, then a pair on the same tile
# A fold final conv (192 -> 64, r1 = its own input channels [0, 64), s1 = 0.2) reads buffer A and writes
# channels [0, 64) of buffer B; a growth pair then reads B from channel `shift`: 64 channels, writing 32
# behind them, and 96, writing the next 32.  With 12 tiles every workgroup owns one tile, so the pair
# follows the final conv on the same tile.  shift 0: the pair's chunks 0 and 1 are the final conv's
# output planes 0 and 1 and are kept in LDS.  shift 16, 32, 48: a valid table as well (the pair's chunk 0
# still overlaps what the final conv wrote), but its chunks 0 and 1 are other planes: nothing may be kept.
# Both buffers start full of data: B's channels the final conv does not write are inputs of the shifted pair.
SHIFTS = (0, 16, 32, 48)


def boundary_case(shift):
    layers = ((192, 64, 0, 0, 1, 0, 1.0, True),
              H.growth(64, shift + 64, 0.2, 1, shift), H.growth(96, shift + 96, 0.35, 1, shift))
    return H.ChainCase(layers, in_ch=(192, 192), wseed=17 + shift, xseeds=((60, 80), (61, 81), (62, 82)))


@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shift", SHIFTS)
def test_final_conv_then_pair_on_the_same_tile(shift, f16):
    r0 = H.check_chain(H.chain_case(boundary_case(shift), 2, 36, 52, f16), 0, acquire=False)
    assert r0 == 2, "the two growth convs behind the final conv pair"


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["off", "on", "handoff_only"])
def test_switch_values(mode):
    """ISR_TRUNK_KEEP 0 (phase 2 stages its chunks whole), 1 (kept tiles) and 2 (kept across the
    phase-2 hand-off only, not across a final conv): all equal the per-conv launches, on a growth-only
    chain with both pairs in place and on a one-block generator of 3 x 3 tiles (two final convs, each
    followed by a pair on the same tile)."""
    want = {"keep": mode, "fp16": 4, "bf16": 4, "generator": 12}
    assert H.switch_child(__file__, {"ISR_TRUNK_KEEP": str(mode)}) == want


if __name__ == "__main__":
    from image_super_resolution_amd import _build, _lib
    _build.build()
    _lib.load()
    res = {"keep": int(os.environ["ISR_TRUNK_KEEP"])}
    for f16 in (True, False):
        res["fp16" if f16 else "bf16"] = _check_chain("rdb4_slopes", 2, 36, 52, f16, False)
    gw, xs, refs = H.model_case(1, 48, 96, 1, True, 11)
    outs, res["generator"] = H.run_plan(gw, xs, chain=True)
    assert all(torch.equal(o, r) for o, r in zip(outs, refs)), "chain differs from the per-conv launches"
    print(json.dumps(res))
