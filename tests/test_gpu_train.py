"""Generator training path (train_engine.py) vs autograd through the fp32 oracle.

The oracle graph (oracle/ref_cpu.generator) is pinned to the reference's own
forward outputs (tests/golden); its gradients are plain autograd of that
graph.  The HIP path stores activations and gradients in bf16 and accumulates
in fp32, so per-tensor gradients are compared by relative L2 error (<= 5%)
and cosine similarity (>= 0.998); the loss itself to 1e-3 relative.
"""
import pytest
import torch
import torch.nn.functional as F

from image_super_resolution_amd import models
from image_super_resolution_amd.weights import normalize, synth_lr_batch, synth_state_dict
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


def _oracle_grads(sd, x, hr, blocks, scale, loss_fn):
    sdc = {k: v.detach().clone().float().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    y = R.generator(sdc, x, num_blocks=blocks, scale=scale, enchant=True)
    loss = loss_fn(y, hr)
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sdc.items() if v.grad is not None}


def _eresnet_step_vs_oracle(blocks, scale, n, h, w, loss):
    """One EResNet training step against autograd of the fp32 oracle at the module's bars;
    returns the step's training plan."""
    torch.manual_seed(0)
    m = models.EResNet(blocks, 0.2, scale)
    m.load_state_dict(synth_state_dict(m.state_dict(), 7))
    lr, hr01 = synth_lr_batch(n, h, w, seed=11, scale=scale)
    x = normalize(lr)
    hr = hr01 * 2 - 1
    loss_fn = F.mse_loss if loss == "mse" else F.l1_loss
    ref_loss, ref_g = _oracle_grads(m.state_dict(), x, hr, blocks, scale, loss_fn)

    m = m.to(DEV).train()
    y = m(x.to(DEV))
    l = loss_fn(y, hr.to(DEV))
    l.backward()
    torch.cuda.synchronize()
    plan = m.__dict__["_isr_train_plan"]
    # the training forward's trunk runs on the persistent trunk kernel (a refused layer table
    # falls back to per-conv launches: correct but ~3.5 ms slower per SRGAN step)
    assert plan.chain is not None
    assert abs(l.item() - ref_loss) <= 1e-3 * abs(ref_loss) + 1e-5, (l.item(), ref_loss)
    worst = []
    for name, p in m.named_parameters():
        g = p.grad
        assert g is not None, name
        r = ref_g[name].to(DEV)
        rel = ((g - r).norm() / r.norm().clamp_min(1e-12)).item()
        cos = F.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
        worst.append((rel, cos, name))
        assert rel <= 5e-2 and cos >= 0.998, f"{name}: rel {rel:.3e} cos {cos:.5f}"
    worst.sort(reverse=True)
    print("worst grads:", worst[:3])
    return plan


@pytest.mark.parametrize("blocks,scale,n,h,w,loss", [(1, 4, 2, 20, 24, "mse"), (2, 2, 2, 36, 40, "l1"),
                                                     (1, 4, 1, 33, 17, "mse")])
def test_eresnet_train_step_grads(blocks, scale, n, h, w, loss):
    _eresnet_step_vs_oracle(blocks, scale, n, h, w, loss)


def test_eresnet_rotating_walk_without_bn(monkeypatch):
    """ISR_TRAIN_GATHER=0: the rotating backward walk on a model without BatchNorm (its
    `bn is None` branches, which a partly BN-fused ResNet reaches too), at the same bars."""
    monkeypatch.setenv("ISR_TRAIN_GATHER", "0")
    plan = _eresnet_step_vs_oracle(1, 4, 2, 20, 24, "mse")
    assert plan.gather is False and plan.chain is not None


def test_train_step_updates_and_repacks():
    """Two optimiser steps: the packed weights follow the parameters (loss changes
    the way the fp32 reference's does)."""
    m = models.EResNet(1, 0.2, 2)
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    lr, hr01 = synth_lr_batch(2, 16, 16, seed=5, scale=2)
    x, hr = normalize(lr), hr01 * 2 - 1
    ref = models.EResNet(1, 0.2, 2)
    ref.load_state_dict(m.state_dict())
    sd_ref = {k: v.clone().requires_grad_(True) for k, v in ref.state_dict().items()}
    opt_ref = torch.optim.SGD(list(sd_ref.values()), lr=0.05)
    m = m.to(DEV).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for _ in range(2):
        opt.zero_grad()
        l = F.mse_loss(m(x.to(DEV)), hr.to(DEV))
        l.backward()
        opt.step()
        opt_ref.zero_grad()
        lr_ = F.mse_loss(R.generator(sd_ref, x, num_blocks=1, scale=2, enchant=True), hr)
        lr_.backward()
        opt_ref.step()
        assert abs(l.item() - lr_.item()) <= 2e-3 * abs(lr_.item()), (l.item(), lr_.item())


def test_resnet_train_step_vs_reference_golden(golden):
    """ResNet (train-mode BatchNorm) step vs the reference's own fp32 outputs
    (tests/golden/train_step_x2.npz): prediction, MSE loss, a spread of
    parameter gradients (conv, BN weight/bias, scaler, tail) and BN running stats."""
    g = golden("train_step_x2")
    m = models.ResNet(1, 0.2, scaleRate=2)
    m.load_state_dict(synth_state_dict(m.state_dict(), int(g["seed"])))
    m = m.to(DEV).train()
    pred = m(torch.from_numpy(g["x"]).to(DEV))
    loss = F.mse_loss(pred, torch.from_numpy(g["target"]).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    ref_pred = torch.from_numpy(g["pred"]).to(DEV)
    assert R.psnr(pred.detach().cpu(), ref_pred.cpu()) >= 40.0
    assert abs(loss.item() - float(g["loss"])) <= 1e-2 * float(g["loss"])
    params = dict(m.named_parameters())
    for k in g:
        if k.startswith("grad:"):
            got, ref = params[k[5:]].grad, torch.from_numpy(g[k]).to(DEV)
            rel = ((got - ref).norm() / ref.norm()).item()
            cos = F.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
            assert rel <= 5e-2 and cos >= 0.998, f"{k}: rel {rel:.3e} cos {cos:.5f}"
    bufs = dict(m.named_buffers())
    for k in g:
        if k.startswith("stat:"):
            got, ref = bufs[k[5:]], torch.from_numpy(g[k]).to(DEV)
            assert ((got - ref).norm() / ref.norm()).item() <= 1e-2, k
    assert int(bufs["residual.0.net.0.conv0.bn.num_batches_tracked"].item()) == 1


def test_resnet_train_step_all_grads_vs_oracle():
    m = models.ResNet(2, 0.2, scaleRate=4)
    m.load_state_dict(synth_state_dict(m.state_dict(), 9))
    lr, hr01 = synth_lr_batch(2, 20, 24, seed=21, scale=4)
    x, hr = normalize(lr), hr01 * 2 - 1
    sd = {k: v.detach().clone().float() for k, v in m.state_dict().items()}
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    y_ref = R.generator(sd, x, num_blocks=2, scale=4, train_bn=True)
    F.mse_loss(y_ref, hr).backward()
    m = m.to(DEV).train()
    F.mse_loss(m(x.to(DEV)), hr.to(DEV)).backward()
    for name, p in m.named_parameters():
        r = params[name].grad.to(DEV)
        rel = ((p.grad - r).norm() / r.norm().clamp_min(1e-12)).item()
        cos = F.cosine_similarity(p.grad.flatten(), r.flatten(), dim=0).item()
        # BN gamma/beta gradients are batch sums of bf16 slot gradients with heavy
        # cancellation: 10 % / 0.995; conv weights 5 % / 0.998
        lim_rel, lim_cos = (0.1, 0.995) if ".bn." in name else (5e-2, 0.998)
        assert rel <= lim_rel and cos >= lim_cos, f"{name}: rel {rel:.3e} cos {cos:.5f}"
    for name, b in m.named_buffers():
        if "running" in name:
            torch.testing.assert_close(b.cpu(), sd[name], rtol=1e-2, atol=1e-3)


@pytest.mark.parametrize("env,bitwise", [({"ISR_TRAIN_SIDE": "0"}, True), ({"ISR_TRAIN_WG_GROUP": "0"}, False),
                                         ({"ISR_TRAIN_BWD_CHAIN": "1"}, False)])
def test_backward_options_same_gradients(monkeypatch, env, bitwise):
    """The options of the backward plan give the production gradients: the weight gradients on
    the main stream instead of the side stream (the same descriptors through the same kernels
    with a workspace of the same size, and split-K sums of a fixed order: bit for bit), the RDB
    weight gradients as separate launches instead of one grouped launch (other split-K
    partition), and the RDB gather convs on the persistent backward chain instead of per-conv
    launches (the chain folds the RDB output gradient by MFMA, the per-conv launch adds it in the
    epilogue).  The reduce-stream case left with its option (the side stream's reductions on a
    third stream, measured slower and removed); that partials + reduce equal one call bit
    for bit stays pinned on the library, in test_gpu_kernels.py::
    test_wgrad3x3_partials_then_reduce_equals_one_call and the partials / reduce case of
    test_gpu_exact.py."""
    torch.manual_seed(0)
    sd = synth_state_dict(models.EResNet(2, 0.2, 2).state_dict(), 13)
    lr, hr01 = synth_lr_batch(2, 32, 32, seed=17, scale=2)
    x, hr = normalize(lr).to(DEV), (hr01 * 2 - 1).to(DEV)

    def grads():
        m = models.EResNet(2, 0.2, 2)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        F.l1_loss(m(x), hr).backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters()}, m.__dict__["_isr_train_plan"]

    ref, _ = grads()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, plan = grads()
    if "ISR_TRAIN_BWD_CHAIN" in env:
        assert plan.bchain is not None  # the option really ran the chain
    if "ISR_TRAIN_SIDE" in env:
        assert plan.side is None
    for k in ref:
        if bitwise:
            assert torch.equal(got[k], ref[k]), k
        else:  # bf16 gradient buffers round differently: compare as the oracle bars do, 10x tighter
            rel = ((got[k] - ref[k]).norm() / ref[k].norm().clamp_min(1e-12)).item()
            cos = F.cosine_similarity(got[k].flatten().double(), ref[k].flatten().double(), dim=0).item()
            assert rel <= 5e-3 and cos >= 0.9999, f"{k}: rel {rel:.3e} cos {cos:.6f}"
