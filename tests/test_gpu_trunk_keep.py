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
    """Geometry word r0 of the chain's last launch (trunk_common.h trunk_rec_off): kept tiles exist
    only where layers were paired."""
    d = chain.desc
    ntiles = d.n * (d.ha // TILE_H) * (d.wa // TILE_W)
    rec_off = (ntiles + 4 + 15) // 16 * 16 + 16
    return int(chain.state[rec_off - 16 + 13].item())


# ---------------------------------------------------------------- whole generators
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
    xs = [normalize(synth_lr_batch(n, h, w, seed=11 + i, scale=4)[0]).to(DEV).contiguous() for i in range(3)]
    return gw, xs, _run(gw, xs, chain=False)[0]


@pytest.mark.parametrize("acquire", [False, True], ids=["plain", "acquire"])
@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n,h,w,blocks", [(1, 16, 32, 1), (1, 48, 96, 1), (2, 36, 52, 2), (3, 224, 416, 1)],
                         ids=["one_tile", "3x3_tiles", "ragged", "546_tiles"])
def test_generator_kept_tiles_bitwise_equal_per_conv_launches(n, h, w, blocks, f16, acquire):
    gw, xs, refs = _model_case(n, h, w, blocks, f16)
    outs, r0 = _run(gw, xs, chain=True, acquire=acquire)
    assert r0 == 4 * 3 * blocks, f"paired layers {r0}: every RDB has two growth pairs, each with a kept hand-off"
    for out, ref in zip(outs, refs):
        assert torch.equal(out, ref), f"chain differs from the per-conv launches: max {(out - ref).abs().max().item()}"


# ---------------------------------------------------------------- hand-built growth-only chains
# a layer: (cin, y_coff, slope); every layer reads channels [0, cin) of one 192-channel buffer and
# writes 32 channels at y_coff of the same buffer
RDB4 = ((64, 64, 0.2), (96, 96, 0.35), (128, 128, 0.5), (160, 160, 0.65))
CHAINS = {
    # name: (layers, expected paired layers)
    "rdb4_slopes": (RDB4, 4),
    "pair_then_single": (RDB4[:3], 2),
}


@functools.lru_cache(maxsize=None)
def _chain_case(name, n, h, w, f16):
    """The buffer, descriptors, three inputs and the buffer contents the per-conv launches leave for
    each input."""
    layers, want = CHAINS[name]
    dtype = torch.float16 if f16 else torch.bfloat16
    g = torch.Generator().manual_seed(9)
    buf = ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=dtype)
    hold, descs = [], []
    for cin, coff, slope in layers:
        wt = (torch.randn(32, cin, 3, 3, generator=g) * (1.5 / (9 * cin) ** 0.5)).to(DEV)
        b = (torch.randn(32, generator=g) * 0.1).to(DEV).contiguous()
        wp = ops.pack_conv3x3(wt, f16=f16)
        hold += [wp, b]
        descs.append(ops.conv3x3_desc(buf, cin, wp, b, 32, buf, y_coff=coff, slope=slope))
    xs = [torch.randn(n, 64, h, w, generator=torch.Generator().manual_seed(40 + i)).to(DEV) for i in range(3)]
    refs = []
    for x in xs:
        buf.t.zero_()
        buf.set_nchw(x, 0)
        for d in descs:
            ops.launch_conv3x3(d)
        torch.cuda.synchronize()
        refs.append(buf.t.clone())
    return buf, descs, xs, refs, want, hold


def _check_chain(name, n, h, w, f16, acquire):
    buf, descs, xs, refs, want, _ = _chain_case(name, n, h, w, f16)
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
    r0 = paired_layers(chain)
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
@functools.lru_cache(maxsize=None)
def _boundary_case(shift, f16):
    n, h, w = 2, 36, 52
    dtype = torch.float16 if f16 else torch.bfloat16
    g = torch.Generator().manual_seed(17 + shift)
    A = ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=dtype)
    B = ops.ActBuffer.alloc(n, h, w, 192, 1, DEV, dtype=dtype)
    hold, descs = [], []

    def conv(cin, cout):
        wt = (torch.randn(cout, cin, 3, 3, generator=g) * (1.5 / (9 * cin) ** 0.5)).to(DEV)
        b = (torch.randn(cout, generator=g) * 0.1).to(DEV).contiguous()
        wp = ops.pack_conv3x3(wt, f16=f16)
        hold.extend([wp, b])
        return wp, b

    wp, b = conv(192, 64)
    descs.append(ops.conv3x3_desc(A, 192, wp, b, 64, B, slope=1.0, r1=A, s1=0.2))
    for cin, slope in ((64, 0.2), (96, 0.35)):
        wp, b = conv(cin, 32)
        descs.append(ops.conv3x3_desc(B, cin, wp, b, 32, B, x_coff=shift, y_coff=shift + cin, slope=slope))
    xs = [(torch.randn(n, 192, h, w, generator=torch.Generator().manual_seed(60 + i)).to(DEV),
           torch.randn(n, 192, h, w, generator=torch.Generator().manual_seed(80 + i)).to(DEV)) for i in range(3)]
    refs = []
    for xa, xb in xs:
        _fill_ab(A, B, xa, xb)
        for d in descs:
            ops.launch_conv3x3(d)
        torch.cuda.synchronize()
        refs.append((A.t.clone(), B.t.clone()))
    return A, B, descs, xs, refs, hold


def _fill_ab(A, B, xa, xb):
    """Both buffers start full of data: B's channels the final conv does not write are inputs of the
    shifted pair."""
    for buf, x in ((A, xa), (B, xb)):
        buf.t.zero_()
        buf.set_nchw(x, 0)


@pytest.mark.parametrize("f16", [True, False], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shift", [0, 16, 32, 48])
def test_final_conv_then_pair_on_the_same_tile(shift, f16):
    A, B, descs, xs, refs, _ = _boundary_case(shift, f16)
    chain = engine.ConvChain(descs, A, DEV, acquire=False, variant=0)
    stream = ops._stream()
    for (xa, xb), (ra, rb) in zip(xs, refs):
        _fill_ab(A, B, xa, xb)
        ops.check(chain.fn(ctypes.byref(chain.desc), stream), "isr_conv_chain")
        torch.cuda.synchronize()
        assert not chain.failed(), "a chain dependency wait gave up"
        assert torch.equal(A.t, ra), "the chain changed its input buffer"
        assert torch.equal(B.t, rb), \
            f"chain differs from the per-conv launches: max {(B.t.float() - rb.float()).abs().max().item()}"
    assert paired_layers(chain) == 2, "the two growth convs behind the final conv pair"


def _child(mode):
    """One value of the switch in a fresh process (the library reads it once)."""
    env = dict(os.environ, ISR_TRUNK_KEEP=str(mode))
    r = subprocess.run([sys.executable, str(Path(__file__).resolve())], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["off", "on", "handoff_only"])
def test_switch_values(mode):
    """ISR_TRUNK_KEEP 0 (phase 2 stages its chunks whole), 1 (kept tiles) and 2 (kept across the
    phase-2 hand-off only, not across a final conv): all equal the per-conv launches, on a growth-only
    chain with both pairs in place and on a one-block generator of 3 x 3 tiles (two final convs, each
    followed by a pair on the same tile)."""
    assert _child(mode) == {"keep": mode, "fp16": 4, "bf16": 4, "generator": 12}


if __name__ == "__main__":
    from image_super_resolution_amd import _build, _lib
    _build.build()
    _lib.load()
    res = {"keep": int(os.environ["ISR_TRUNK_KEEP"])}
    for f16 in (True, False):
        res["fp16" if f16 else "bf16"] = _check_chain("rdb4_slopes", 2, 36, 52, f16, False)
    gw, xs, refs = _model_case(1, 48, 96, 1, True)
    outs, res["generator"] = _run(gw, xs, chain=True)
    assert all(torch.equal(o, r) for o, r in zip(outs, refs)), "chain differs from the per-conv launches"
    print(json.dumps(res))
