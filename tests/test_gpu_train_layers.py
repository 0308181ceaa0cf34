"""train_layers.py: TrainConv packs the same bytes as the ops.pack_* calls its rules stand for,
repacks in place, returns its parameters in the autograd Functions' order, and the PlanLease
frees the Denoise training plan when a forward's graph dies."""
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from image_super_resolution_amd import models, ops
from image_super_resolution_amd.train_layers import TrainConv, expand_dgrad, expand_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def _w(cout, cin, k, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * cout + cin)
    return (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5).to(DEV)


def _padded(w, cin):
    out = torch.zeros(w.shape[0], cin, *w.shape[2:], device=w.device)
    out[:, :w.shape[1]] = w
    return out


def _direct(kind, w, kw):
    """The packs spelled out: (fwd, bwd) of one layer by plain ops calls."""
    if kind == "3x3":
        cin_p = kw.get("cin_p", w.shape[1])
        return (ops.pack_conv3x3(_padded(w, cin_p)),
                ops.pack_conv3x3_dgrad(_padded(w, ops.round_up(cin_p, 32)), scale=kw.get("dgrad_scale", 1.0),
                                       sub2=kw.get("sub2", False)))
    if kind == "s2":
        return ops.pack_conv3x3(expand_fwd(w)), ops.pack_conv3x3(expand_dgrad(w))
    if kind == "head":
        return ops.pack_head9x9(w), None
    return ops.pack_tail9x9(w), ops.pack_head9x9(w.flip(2, 3).transpose(0, 1).contiguous())


CASES = [
    ("3x3", 32, 64, {}),
    ("3x3", 64, 3, dict(cin_p=16)),
    ("3x3", 64, 3, dict(cin_p=32)),
    ("3x3", 256, 64, dict(sub2=True, dgrad_scale=0.2)),
    ("s2", 64, 64, {}),
    ("head", 64, 3, {}),
    ("tail", 3, 64, {}),
]


def _same(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))


@pytest.mark.parametrize("kind,cout,cin,kw", CASES, ids=[f"{c[0]}-{c[2]}to{c[1]}-{i}" for i, c in enumerate(CASES)])
def test_pack_equals_direct_ops_calls_and_repacks_in_place(kind, cout, cin, kw):
    k = 3 if kind in ("3x3", "s2") else 9
    w = _w(cout, cin, k)
    layer = TrainConv(w, None, cin, cout, kind, **kw)
    layer.pack()
    fwd, bwd = _direct(kind, w, kw)
    assert _same(layer.fwd, fwd) and _same(layer.bwd, bwd)
    assert (layer.bwd is None) == (kind == "head")
    # in-place repack: same addresses, contents of a fresh pack of the new weights
    ptrs = (layer.fwd.data_ptr(), layer.bwd.data_ptr() if layer.bwd is not None else None)
    w.copy_(_w(cout, cin, k, seed=1))
    layer.pack()
    assert ptrs == (layer.fwd.data_ptr(), layer.bwd.data_ptr() if layer.bwd is not None else None)
    fwd2, bwd2 = _direct(kind, w, kw)
    assert _same(layer.fwd, fwd2) and _same(layer.bwd, bwd2)
    assert not torch.equal(fwd, fwd2)  # the weights really changed


def test_params_order():
    both = SimpleNamespace(conv=nn.Conv2d(16, 32, 3, padding=1, bias=True), bn=nn.BatchNorm2d(32))
    l = TrainConv.of(both)
    assert [id(p) for p in l.params()] == [id(p) for p in (both.conv.weight, both.conv.bias, both.bn.weight,
                                                           both.bn.bias)]
    bn_only = models.Conv(64, 64, 3)
    l = TrainConv.of(bn_only, "3x3")
    assert bn_only.conv.bias is None
    assert [id(p) for p in l.params()] == [id(p) for p in (bn_only.conv.weight, bn_only.bn.weight, bn_only.bn.bias)]
    bias_only = models.ConvWithoutBN(64, 256, 3, 2)
    l = TrainConv.of(bias_only)
    assert l.kind == "s2" and l.bn is None
    assert [id(p) for p in l.params()] == [id(p) for p in (bias_only.conv.weight, bias_only.conv.bias)]
    bare = nn.Conv2d(3, 64, 3, padding=1)  # a bare conv (VGG)
    l = TrainConv.of(bare, cin_p=16)
    assert (l.kind, l.cin, l.cin_p, l.cout) == ("3x3", 3, 16, 64)
    assert [id(p) for p in l.params()] == [id(bare.weight), id(bare.bias)]


def _denoise():
    torch.manual_seed(0)
    m = models.Denoise(0).to(DEV).train()
    x = torch.rand(1, 3, 32, 32, device=DEV) * 2 - 1
    return m, x


def test_lease_dead_graph_frees_the_plan():
    m, x = _denoise()
    y = m(x)
    plan = m.__dict__["_isr_train_plan"]
    assert plan.busy
    del y
    assert not plan.busy
    y = m(x)  # a second forward succeeds
    assert plan.busy and m.__dict__["_isr_train_plan"] is plan
    y.sum().backward()
    assert not plan.busy
    assert all(p.grad is not None for p in plan.params())


def test_lease_live_graph_still_holds_the_plan():
    m, x = _denoise()
    y = m(x)
    with pytest.raises(RuntimeError, match="previous forward's graph was not backpropagated"):
        m(x)
    y.sum().backward()
    assert not m.__dict__["_isr_train_plan"].busy
