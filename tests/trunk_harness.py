"""What the bit-identity tests of the persistent trunk kernel (isr_conv_chain, csrc/trunk.hip) share:
inputs, the plan runner, the cached whole-generator case, hand-built chains described as data with
their builder and checker, the geometry word r0, and the child process of a once-per-process switch.
test_gpu_chain.py and test_gpu_trunk_{roles,epilogue,pairs,keep}.py hold the cases and what each
asserts alone; test_trunk_harness_cpu.py pins the state layout copied here to the library."""
import collections
import ctypes
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:  # a script run (a switch child) starts with tests/ alone on its path
    sys.path.insert(0, str(ROOT))

from image_super_resolution_amd import engine, models, ops  # noqa: E402
from image_super_resolution_amd.weights import normalize, synth_lr_batch, synth_state_dict  # noqa: E402

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TILE_H, TILE_W = 16, 32
BUF_CH = 192  # channels of every hand-built chain buffer (an RDB's dense buffer)
# the state words (csrc/trunk_common.h): progress words, then TrunkGeo, then the layer records
GEO_WORDS = 16  # sizeof(TrunkGeo) / 4, just before the records
GEO_R0 = 13     # index of r0 (the number of paired layers) in TrunkGeo
GAVE_UP = "a chain dependency wait gave up"


def rec_off(ntiles):
    """trunk_rec_off: the word at which the layer records start."""
    return (ntiles + 4 + 15) // 16 * 16 + GEO_WORDS


def paired_layers(chain):
    """Geometry word r0 of the chain's last launch: what the prep kernel decided to pair."""
    d = chain.desc
    ntiles = d.n * (d.ha // TILE_H) * (d.wa // TILE_W)
    return int(chain.state[rec_off(ntiles) - GEO_WORDS + GEO_R0].item())


def lr_inputs(n, h, w, k, seed, zero_every=None):
    """k normalised LR batches of seeds seed, seed + 1, ...; `zero_every`: every such column is
    exactly zero (a signed-zero probe)."""
    xs = []
    for i in range(k):
        x = normalize(synth_lr_batch(n, h, w, seed=seed + i, scale=4)[0])
        if zero_every:
            x[..., ::zero_every] = 0
        xs.append(x.to(DEV).contiguous())
    return xs


def pack(blocks, scale=4, enchant=False, seed=0, f16=True):
    m = (models.EResNet if enchant else models.ResNet)(blocks, 0.2, scaleRate=scale)
    sd = synth_state_dict(m.state_dict(), seed)
    return engine.pack_generator({k: v.to(DEV) for k, v in sd.items()}, enchant=enchant, device=DEV, f16=f16)


def run_plan(gw, xs, chain, acquire=False):
    """One plan, one forward per input in `xs` (different inputs back to back: a stale hand-off read
    would return the previous input's activations and show up).  Returns the outputs and, for a
    chained plan, its paired-layer count."""
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
        assert plan.chain.variant == 0 and not plan.chain.failed(), GAVE_UP
    return outs, (paired_layers(plan.chain) if chain else None)


@functools.lru_cache(maxsize=None)
def model_case(n, h, w, blocks, f16, seed, zero_every=None):
    """Weights (seed 0), three inputs and the per-conv reference outputs of one geometry, computed
    once per session and shared by every file that asks for the same key."""
    gw = pack(blocks, f16=f16)
    xs = lr_inputs(n, h, w, 3, seed, zero_every)
    return gw, xs, run_plan(gw, xs, chain=False)[0]


# ---------------------------------------------------------------- hand-built chains
# A layer: (cin, cout, source buffer, x_coff, destination buffer, y_coff, slope, fold).  `fold`: r1 is
# the layer's own source with s1 = 0.2 (an RDB final conv's residual).
# A case: its layers, the input channels written into each buffer, the seed of the one generator that
# draws every layer's weight, then bias, in order, and the input seeds as a table [input][buffer].
ChainCase = collections.namedtuple("ChainCase", "layers in_ch wseed xseeds zero_every", defaults=(None,))
BuiltChain = collections.namedtuple("BuiltChain", "case bufs descs xs refs keep")


def growth(cin, y_coff, slope, buf=0, x_coff=0):
    """A growth conv: `cin` channels from x_coff of a buffer, 32 channels written at y_coff of the same."""
    return (cin, 32, buf, x_coff, buf, y_coff, slope, False)


def fill(bufs, x):
    for b, xb in zip(bufs, x):
        b.t.zero_()
        b.set_nchw(xb, 0)


@functools.lru_cache(maxsize=None)
def chain_case(case, n, h, w, f16):
    """Buffers, descriptors (built as GeneratorPlan builds the ones it hands to ConvChain), three
    inputs per buffer and the buffer contents the per-conv launches leave for each input."""
    g = torch.Generator().manual_seed(case.wseed)
    bufs = [ops.ActBuffer.alloc(n, h, w, BUF_CH, 1, DEV, dtype=torch.float16 if f16 else torch.bfloat16)
            for _ in case.in_ch]
    keep, descs = [], []
    for cin, cout, src, x_coff, dst, y_coff, slope, fold in case.layers:
        wt = (torch.randn(cout, cin, 3, 3, generator=g) * (1.5 / (9 * cin) ** 0.5)).to(DEV)
        b = (torch.randn(cout, generator=g) * 0.1).to(DEV).contiguous()
        wp = ops.pack_conv3x3(wt, f16=f16)
        keep += [wp, b]
        res = dict(r1=bufs[src], r1_coff=x_coff, s1=0.2) if fold else {}
        descs.append(ops.conv3x3_desc(bufs[src], cin, wp, b, cout, bufs[dst], x_coff=x_coff, y_coff=y_coff,
                                      slope=slope, **res))
    xs = []
    for seeds in case.xseeds:
        x = [torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(s)) for c, s in zip(case.in_ch, seeds)]
        for xb in x:
            if case.zero_every:
                xb[..., ::case.zero_every] = 0
        xs.append([xb.to(DEV) for xb in x])
    refs = []
    for x in xs:
        fill(bufs, x)
        for d in descs:
            ops.launch_conv3x3(d)
        torch.cuda.synchronize()
        refs.append([b.t.clone() for b in bufs])
    return BuiltChain(case, bufs, descs, xs, refs, keep)


def check_chain(built, grid_buffer, acquire):
    """The chain over the case's descriptors must leave in every buffer, for every input in turn, what
    the per-conv launches left, and no dependency wait may give up.  Returns the paired-layer count."""
    chain = engine.ConvChain(built.descs, built.bufs[grid_buffer], DEV, acquire=acquire, variant=0)
    written = {layer[4] for layer in built.case.layers}
    stream = ops._stream()
    for x, ref in zip(built.xs, built.refs):
        fill(built.bufs, x)
        ops.check(chain.fn(ctypes.byref(chain.desc), stream), "isr_conv_chain")
        torch.cuda.synchronize()
        assert not chain.failed(), GAVE_UP
        for i, (b, rb) in enumerate(zip(built.bufs, ref)):
            assert torch.equal(b.t, rb), "the chain changed its input buffer" if i not in written else \
                f"chain differs from the per-conv launches: max {(b.t.float() - rb.float()).abs().max().item()}"
    return paired_layers(chain)


def switch_child(script, env):
    """`script` (a test file's __main__) in a fresh process under `env`: one value of a switch the
    library reads once per process.  Returns the last line of its output, parsed as JSON."""
    r = subprocess.run([sys.executable, str(Path(script).resolve())], env=dict(os.environ, **env), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])
