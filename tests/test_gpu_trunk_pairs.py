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
import ctypes
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

from image_super_resolution_amd import engine, models, ops  # noqa: E402
from image_super_resolution_amd.weights import normalize, synth_lr_batch, synth_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TILE_H, TILE_W = 16, 32


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def paired_layers(chain):
    """Geometry word r0 of the chain's last launch: the 16 geometry words end at the layer records
    (trunk_common.h trunk_rec_off)."""
    d = chain.desc
    ntiles = d.n * (d.ha // TILE_H) * (d.wa // TILE_W)
    rec_off = (ntiles + 4 + 15) // 16 * 16 + 16
    return int(chain.state[rec_off - 16 + 13].item())


# ---------------------------------------------------------------- whole generators
def _inputs(n, h, w, k, seed):
    return [normalize(synth_lr_batch(n, h, w, seed=seed + i, scale=4)[0]).to(DEV).contiguous() for i in range(k)]


def _run(gw, xs, chain, acquire=False):
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
    return outs, (paired_layers(plan.chain) if chain else None)


@functools.lru_cache(maxsize=None)
def _model_case(n, h, w, blocks, f16):
    m = models.ResNet(blocks, 0.2, scaleRate=4)
    sd = synth_state_dict(m.state_dict(), 0)
    gw = engine.pack_generator({k: v.to(DEV) for k, v in sd.items()}, enchant=False, device=DEV, f16=f16)
    xs = _inputs(n, h, w, 3, seed=3)
    return gw, xs, _run(gw, xs, chain=False)[0]


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w,blocks", [(1, 16, 32, 1), (1, 48, 96, 1), (2, 36, 52, 2), (3, 224, 416, 1)],
                         ids=["one_tile", "3x3_tiles", "ragged", "546_tiles"])
def test_generator_pairs_bitwise_equal_per_conv_launches(n, h, w, blocks, f16, acquire):
    gw, xs, refs = _model_case(n, h, w, blocks, f16)
    outs, r0 = _run(gw, xs, chain=True, acquire=acquire)
    assert r0 == 4 * 3 * blocks, f"paired layers {r0}: every RDB has two growth pairs"
    for out, ref in zip(outs, refs):
        assert torch.equal(out, ref), f"chain differs from the per-conv launches: max {(out - ref).abs().max().item()}"


# ---------------------------------------------------------------- hand-built growth-only chains
# a layer: (cin, y_coff, slope, buffer index); every layer reads channels [0, cin) of its buffer and
# writes 32 channels at y_coff of the same buffer
RDB4 = ((64, 64, 0.2, 0), (96, 96, 0.35, 0), (128, 128, 0.5, 0), (160, 160, 0.65, 0))
CHAINS = {
    # name: (layers, input channels per buffer, expected paired layers)
    "rdb4_slopes": (RDB4, (64,), 4),
    "pair_then_single": (RDB4[:3], (64,), 2),
    "one_pair": (RDB4[:2], (64,), 2),
    "same_cin": (((64, 64, 0.2, 0), (64, 96, 0.35, 0)), (64,), 0),
    "cin_plus_64": (((64, 64, 0.2, 0), (128, 128, 0.35, 0)), (64,), 0),
    "other_buffer": (((64, 64, 0.2, 0), (96, 96, 0.35, 1)), (64, 96), 0),
}


@functools.lru_cache(maxsize=None)
def _chain_case(name, n, h, w, f16):
    """Buffers, descriptors, three inputs per buffer and the buffer contents the per-conv launches
    leave for each input."""
    layers, in_ch, want = CHAINS[name]
    dtype = torch.float16 if f16 else torch.bfloat16
    g = torch.Generator().manual_seed(5)
    bufs = [ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=dtype) for _ in in_ch]
    keep, descs = [], []
    for cin, coff, slope, bi in layers:
        wt = (torch.randn(32, cin, 3, 3, generator=g) * (1.5 / (9 * cin) ** 0.5)).to(DEV)
        b = (torch.randn(32, generator=g) * 0.1).to(DEV).contiguous()
        wp = ops.pack_conv3x3(wt, f16=f16)
        keep += [wp, b]
        descs.append(ops.conv3x3_desc(bufs[bi], cin, wp, b, 32, bufs[bi], y_coff=coff, slope=slope))
    xs = [[torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(20 + 7 * i + k)).to(DEV)
           for k, c in enumerate(in_ch)] for i in range(3)]
    refs = []
    for x in xs:
        _fill(bufs, x)
        for d in descs:
            ops.launch_conv3x3(d)
        torch.cuda.synchronize()
        refs.append([b.t.clone() for b in bufs])
    return bufs, descs, xs, refs, want, keep


def _fill(bufs, x):
    for b, xb in zip(bufs, x):
        b.t.zero_()
        b.set_nchw(xb, 0)


def _check_chain(name, n, h, w, f16, acquire, want=None):
    bufs, descs, xs, refs, want_case, _ = _chain_case(name, n, h, w, f16)
    chain = engine.ConvChain(descs, bufs[0], DEV, acquire=acquire, variant=0)
    stream = ops._stream()
    for x, ref in zip(xs, refs):
        _fill(bufs, x)
        ops.check(chain.fn(ctypes.byref(chain.desc), stream), "isr_conv_chain")
        torch.cuda.synchronize()
        assert not chain.failed(), "a chain dependency wait gave up"
        for b, rb in zip(bufs, ref):
            assert torch.equal(b.t, rb), \
                f"chain differs from the per-conv launches: max {(b.t.float() - rb.float()).abs().max().item()}"
    r0 = paired_layers(chain)
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


def _child(mode):
    """One value of the switch in a fresh process (the library reads it once)."""
    env = dict(os.environ, ISR_TRUNK_PAIRS=str(mode))
    r = subprocess.run([sys.executable, str(Path(__file__).resolve())], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("mode,want", [(0, 0), (1, 2), (2, 4)], ids=["off", "long", "all"])
def test_switch_values(mode, want):
    """ISR_TRUNK_PAIRS: 0 pairs nothing, 1 only the pair sharing 8 chunks (layers 2, 3), 2 both."""
    assert _child(mode) == {"fp16": want, "bf16": want}


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
