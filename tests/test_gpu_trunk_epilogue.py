"""The trunk kernel's tile epilogue forms (trunk.hip run_tile: one compiled body per layer form,
classified by the prep kernel; full tiles skip the `valid` select; packed fp32 -> 16-bit converts):
the chain must reproduce the per-conv launches of the same descriptors BIT FOR BIT, in fp16 and
bf16, three different inputs back to back on one plan.

One RRDB holds all three production forms (growth; final with the residual fold; final with the
fold and the RRDB residual r2).  Geometries: one full tile; four full tiles with neighbour
hand-offs; ragged in rows and columns beside full tiles (the `valid` path next to the full one);
every tile ragged.  The fallback: a hand-built growth-only chain with slopes 0.2 (specialised),
1.0 and 1.5 (outside (0, 1): the general body; a specialised LeakyReLU taken there by mistake would
still agree at 1.0, so 1.5 is the case that tells) on inputs of both signs.

Signed zero: every seventh input column is exactly zero.  The LeakyReLU kept in the specialised
growth body is the general body's compare and select (a >= 0 ? a : a * slope), not a float max:
hipcc canonicalises both inputs of a max with one more v_max each, so the max form costs the same
2.5 instructions per value (with the packed multiply) and would add a -0 / NaN argument for nothing.
The zeros stay as a probe of that choice; fp32 accumulators of real convolutions seldom land on
+-0, so they show little by themselves."""
import pytest
import torch

import trunk_harness as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w,blocks", [(1, 16, 32, 1), (1, 32, 64, 1), (2, 36, 52, 2), (1, 20, 40, 1)],
                         ids=["one_full_tile", "four_full_tiles", "ragged_beside_full", "all_ragged"])
def test_epilogue_forms_bitwise_equal_per_conv_launches(n, h, w, blocks, f16):
    gw, xs, refs = H.model_case(n, h, w, blocks, f16, 11, zero_every=7)
    for out, ref in zip(H.run_plan(gw, xs, chain=True)[0], refs):
        assert torch.equal(out, ref), f"chain differs from the per-conv launches: max {(out - ref).abs().max().item()}"


# ---- the fallback: a growth-only chain (80 -> 32 at channel 80, 112 -> 32 at 112, 144 -> 32 at 144
# over one 192-channel buffer) whose LeakyReLU slope is inside or outside (0, 1) ----
GROWTH_LAYERS = ((80, 80), (112, 112), (144, 144))  # (cin, y_coff)


def slope_case(slope):
    """Standard-normal inputs (both signs) with every seventh column zero."""
    layers = tuple(H.growth(cin, coff, slope) for cin, coff in GROWTH_LAYERS)
    return H.ChainCase(layers, in_ch=(80,), wseed=5, xseeds=((20,), (21,), (22,)), zero_every=7)


SLOPES = (0.2, 1.0, 1.5)


@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("slope", SLOPES, ids=["slope0.2", "slope1.0", "slope1.5"])
def test_growth_chain_slopes_inside_and_outside_unit_interval(slope, f16):
    built = H.chain_case(slope_case(slope), 2, 36, 52, f16)
    H.check_chain(built, 0, acquire=False)
    # the layers' outputs (planes 5..10 of [n][c/16][hp][wp][16]) hold negative values: the slope acted
    assert (built.refs[0][0][:, 80 // 16:].float() < 0).any(), "the case needs negative pre-activations"
