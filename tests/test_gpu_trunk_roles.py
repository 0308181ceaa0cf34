"""The trunk kernel's chunk roles (trunk.hip run_tile: first / steady / last chunk, the steady run
split at the first chunk the previous layer wrote, one chunk peeled when a count is odd): the chain
must reproduce the per-conv launches of the same descriptors BIT FOR BIT, in fp16 and bf16, with
and without the acquire fence, three different inputs back to back on one plan.

Geometries: one tile (grid of 1: every next item is the same tile, every layer boundary staged at
its own top), ragged tiles across an RRDB boundary, and 546 tiles (more than the 512 resident
workgroups: a workgroup walks two tiles of one layer and prefetches across the tile boundary).
The real RRDB table has even chunk counts only; a hand-built growth-only chain of 5, 7 and 9 chunks
(first_new 5 and 7) exercises the odd-count peel and the split."""
import pytest
import torch

import trunk_harness as H
from image_super_resolution_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w,blocks", [(1, 16, 32, 1), (2, 36, 52, 2), (3, 224, 416, 1)],
                         ids=["one_tile", "ragged", "546_tiles"])
def test_roles_bitwise_equal_per_conv_launches(n, h, w, blocks, f16, acquire):
    gw, xs, refs = H.model_case(n, h, w, blocks, f16, 3)
    for out, ref in zip(H.run_plan(gw, xs, chain=True, acquire=acquire)[0], refs):
        assert torch.equal(out, ref), f"chain differs from the per-conv launches: max {(out - ref).abs().max().item()}"


# ---- a growth-only chain with odd chunk counts: 80 -> 32 at channel 80, 112 -> 32 at 112,
# 144 -> 32 at 144 over one 192-channel buffer (5, 7 and 9 chunks; first_new = none, 5, 7) ----
ODD_LAYERS = tuple(H.growth(cin, cin, engine.LEAKY_DEFAULT) for cin in (80, 112, 144))
ODD_CASE = H.ChainCase(ODD_LAYERS, in_ch=(80,), wseed=5, xseeds=((20,), (21,), (22,)))


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w", [(2, 36, 52), (3, 224, 416)], ids=["ragged", "546_tiles"])
def test_odd_chunk_counts_growth_only_chain(n, h, w, f16, acquire):
    H.check_chain(H.chain_case(ODD_CASE, n, h, w, f16), 0, acquire)
