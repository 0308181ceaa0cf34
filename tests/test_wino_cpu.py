"""The fp16 Winograd F(2,3) conv path, checks that need no GPU: the three C-ABI exports (what they
refuse: tests/test_capi_refusals.py), the CPU restatement tests/wino_ref.py against the plain conv with
its roundings switched off (pins the transform matrices independently of any kernel), and the
engine's refusals of `wino` with bf16 storage or with the chained trunk."""
import re
import subprocess
import types

import pytest
import torch
import torch.nn.functional as F

from image_super_resolution_amd import _lib
from wino_ref import wino_ref


def test_wino_symbols_exported(built_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (isr_[a-z0-9_]+)\b", nm))
    for name in ("isr_conv3x3_wino_packed_bytes", "isr_pack_conv3x3_wino_f16", "isr_conv3x3_wino_fwd"):
        assert name in exported and name in _lib.SIGNATURES, name
    assert built_lib.isr_conv3x3_wino_packed_bytes(64, 192) == 64 * 192 * 12 * 2


@pytest.mark.parametrize("n,cin,cout,h,w", [(1, 16, 32, 8, 6), (1, 192, 64, 18, 40), (2, 32, 32, 5, 7)])
def test_wino_ref_unrounded_is_the_plain_conv(n, cin, cout, h, w):
    """F(2,3) is exact arithmetic: without the fp16 roundings of U and V and of the output the
    restatement equals conv2d in fp64, for even and odd widths, with the full epilogue."""
    g = torch.Generator().manual_seed(cin + w)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    W = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    r1 = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    r2 = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    ref = F.conv2d(x, W, padding=1)
    got = wino_ref(x, W, round_uv=False, round_out=False)
    assert got.shape == ref.shape and got.dtype == torch.float64
    assert (got - ref).abs().max().item() <= 1e-9 * ref.abs().max().item()
    # epilogue order: v = act(y + bias); v = v*s1 + r1; v = v*s2 + r2 (0.5 / 0.25 are exact in fp32)
    v = F.conv2d(x, W, b, padding=1)
    v = torch.where(v >= 0, v, v * 0.5)
    v = (v * 0.25 + r1) * 0.5 + r2
    got = wino_ref(x, W, b, slope=0.5, r1=r1, s1=0.25, r2=r2, s2=0.5, round_uv=False, round_out=False)
    assert (got - v).abs().max().item() <= 1e-9 * v.abs().max().item()


def test_wino_ref_rounds_once_to_fp16():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 16, 6, 9, generator=g).half().float()
    W = torch.randn(32, 16, 3, 3, generator=g) * 0.1
    y = wino_ref(x, W)
    assert torch.equal(y, y.half().double())  # fp16-representable
    exact = F.conv2d(x.double(), W.double(), padding=1)
    # U and V carry one fp16 rounding each (2^-11 relative on each product term), the output one more
    assert (y - exact).abs().max().item() <= 4e-3 * exact.abs().max().item()
    assert not torch.equal(y, exact.float().half().double())


def test_engine_refuses_wino_with_bf16_or_chain():
    """`wino` needs fp16 storage and per-conv launches; both refusals come before any GPU work."""
    from image_super_resolution_amd import engine
    with pytest.raises(ValueError, match="fp16"):
        engine.pack_generator({}, enchant=False, device="cpu", f16=False, wino="final")
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for dtype, chain, match in ((torch.float16, True, "chain"), (torch.bfloat16, None, "fp16"),
                                (torch.bfloat16, False, "fp16")):
        gw = types.SimpleNamespace(dtype=dtype)
        for build in (engine.GeneratorPlan, engine.make_plan):
            with pytest.raises(ValueError, match=match):
                build(gw, 1, 32, 32, "cpu", False, False, mean, std, chain=chain, wino="rdb")
        with pytest.raises(ValueError, match=match):
            engine.SplitGeneratorPlan(gw, 2, 32, 32, "cpu", False, False, mean, std, chain=chain, wino="final")
    with pytest.raises(ValueError, match="wino must be"):
        engine.wino_mode("2d")
    assert engine.wino_mode("") is None and engine.wino_mode("off") is None and engine.wino_mode("rdb") == "rdb"
