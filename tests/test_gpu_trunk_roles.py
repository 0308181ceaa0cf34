"""The trunk kernel's chunk roles (trunk.hip run_tile: first / steady / last chunk, the steady run
split at the first chunk the previous layer wrote, one chunk peeled when a count is odd): the chain
must reproduce the per-conv launches of the same descriptors BIT FOR BIT, in fp16 and bf16, with
and without the acquire fence, three different inputs back to back on one plan.

Geometries: one tile (grid of 1: every next item is the same tile, every layer boundary staged at
its own top), ragged tiles across an RRDB boundary, and 546 tiles (more than the 512 resident
workgroups: a workgroup walks two tiles of one layer and prefetches across the tile boundary).
The real RRDB table has even chunk counts only; a hand-built growth-only chain of 5, 7 and 9 chunks
(first_new 5 and 7) exercises the odd-count peel and the split."""
import ctypes
import functools

import pytest
import torch

from image_super_resolution_amd import engine, models, ops
from image_super_resolution_amd.weights import normalize, synth_lr_batch, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def _inputs(n, h, w, k, seed):
    return [normalize(synth_lr_batch(n, h, w, seed=seed + i, scale=4)[0]).to(DEV).contiguous() for i in range(k)]


def _run(gw, xs, chain, acquire=False):
    """One plan, one forward per input in `xs` (a stale hand-off read would return the previous
    input's activations and show up)."""
    x0 = xs[0]
    plan = engine.GeneratorPlan(gw, x0.shape[0], x0.shape[2], x0.shape[3], x0.device, False, False, MEAN, STD,
                                chain=chain, chain_acquire=acquire)
    assert (plan.chain is not None) == chain
    outs = []
    for x in xs:
        out = torch.empty(plan.out_shape, device=DEV)
        plan.run(x, out)
        outs.append(out)
    torch.cuda.synchronize()
    if chain:
        assert plan.chain.variant == 0 and not plan.chain.failed(), "a chain dependency wait gave up"
    return outs


@functools.lru_cache(maxsize=None)
def _model_case(n, h, w, blocks, f16):
    """Weights, inputs and the per-conv reference outputs of one geometry (computed once)."""
    m = models.ResNet(blocks, 0.2, scaleRate=4)
    sd = synth_state_dict(m.state_dict(), 0)
    gw = engine.pack_generator({k: v.to(DEV) for k, v in sd.items()}, enchant=False, device=DEV, f16=f16)
    xs = _inputs(n, h, w, 3, seed=3)
    return gw, xs, _run(gw, xs, chain=False)


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w,blocks", [(1, 16, 32, 1), (2, 36, 52, 2), (3, 224, 416, 1)],
                         ids=["one_tile", "ragged", "546_tiles"])
def test_roles_bitwise_equal_per_conv_launches(n, h, w, blocks, f16, acquire):
    gw, xs, refs = _model_case(n, h, w, blocks, f16)
    for out, ref in zip(_run(gw, xs, chain=True, acquire=acquire), refs):
        assert torch.equal(out, ref), f"chain differs from the per-conv launches: max {(out - ref).abs().max().item()}"


# ---- a growth-only chain with odd chunk counts: 80 -> 32 at channel 80, 112 -> 32 at 112,
# 144 -> 32 at 144 over one 192-channel buffer (5, 7 and 9 chunks; first_new = none, 5, 7) ----
ODD_LAYERS = ((80, 80), (112, 112), (144, 144))


@functools.lru_cache(maxsize=None)
def _odd_case(n, h, w, f16):
    """The buffer, descriptors (built as GeneratorPlan builds the ones it hands to ConvChain:
    ops.conv3x3_desc of a growth conv writing into its own input buffer), three inputs and the
    buffer contents the per-conv launches leave for each."""
    dtype = torch.float16 if f16 else torch.bfloat16
    g = torch.Generator().manual_seed(5)
    buf = ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=dtype)
    keep, descs = [], []
    for cin, coff in ODD_LAYERS:
        wt = (torch.randn(32, cin, 3, 3, generator=g) * (1.5 / (9 * cin) ** 0.5)).to(DEV)
        b = (torch.randn(32, generator=g) * 0.1).to(DEV).contiguous()
        wp = ops.pack_conv3x3(wt, f16=f16)
        keep += [wp, b]
        descs.append(ops.conv3x3_desc(buf, cin, wp, b, 32, buf, y_coff=coff, slope=engine.LEAKY_DEFAULT))
    xs = [torch.randn(n, 80, h, w, generator=torch.Generator().manual_seed(20 + i)).to(DEV) for i in range(3)]
    refs = []
    for x in xs:
        buf.t.zero_()
        buf.set_nchw(x, 0)
        for d in descs:
            ops.launch_conv3x3(d)
        torch.cuda.synchronize()
        refs.append(buf.t.clone())
    return buf, descs, xs, refs, keep


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w", [(2, 36, 52), (3, 224, 416)], ids=["ragged", "546_tiles"])
def test_odd_chunk_counts_growth_only_chain(n, h, w, f16, acquire):
    buf, descs, xs, refs, _ = _odd_case(n, h, w, f16)
    chain = engine.ConvChain(descs, buf, DEV, acquire=acquire, variant=0)
    stream = ops._stream()
    for x, ref in zip(xs, refs):
        buf.t.zero_()
        buf.set_nchw(x, 0)
        ops.check(chain.fn(ctypes.byref(chain.desc), stream), "isr_conv_chain")
        torch.cuda.synchronize()
        assert not chain.failed(), "a chain dependency wait gave up"
        assert torch.equal(buf.t, ref), \
            f"chain differs from the per-conv launches: max {(buf.t.float() - ref.float()).abs().max().item()}"
