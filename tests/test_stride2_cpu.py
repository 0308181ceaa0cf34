"""The stride-2 weight algebra of train_layers.py (expand_fwd / expand_dgrad / gather_wgrad)
against torch's own stride-2 conv, on the CPU.  The weights are drawn in float32, so the
expansions (which produce float32) are exact copies; everything is computed in float64:
the two conv identities differ from torch only by the summation order (bound 1e-12 absolute
on O(10) values, ~1e4 ulp of float64), the two gather identities are pure copies (exact; the one
that compares two backward passes of torch runs on integers, whose sums are exact in any order)."""
import pytest
import torch
import torch.nn.functional as F

from image_super_resolution_amd.train_layers import expand_dgrad, expand_fwd, gather_wgrad

CO, CI = 6, 5


def _unshuffle(x):
    return torch.cat([x[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], 1)


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(CO, CI, 3, 3, generator=g)                          # float32
    x = torch.randn(2, CI, 8, 12, generator=g, dtype=torch.float64)
    gy = torch.randn(2, CO, 4, 6, generator=g, dtype=torch.float64)
    return w, x, _unshuffle(x), gy


def test_forward_is_a_conv_over_the_unshuffled_input(case):
    w, x, xu, _ = case
    ref = F.conv2d(x, w.double(), stride=2, padding=1)
    got = F.conv2d(xu, expand_fwd(w).double(), padding=1)
    err = (got - ref).abs().max().item()
    print("stride-2 forward max abs error", err)
    assert err <= 1e-12


def test_dgrad_is_a_conv_with_a_pixel_shuffle_store(case):
    w, _, _, gy = case
    ref = F.conv_transpose2d(gy, w.double(), stride=2, padding=1, output_padding=1)
    got = F.pixel_shuffle(F.conv2d(gy, expand_dgrad(w).double(), padding=1), 2)
    err = (got - ref).abs().max().item()
    print("stride-2 dgrad max abs error", err)
    assert err <= 1e-12


def test_gather_wgrad_of_the_expanded_gradient_is_the_stride2_gradient():
    """On integers in [-3, 3]: both weight gradients are then exact in float64, so they are equal on every
    CPU; on random floats two conv backward passes agree only up to the order in which a CPU sums them."""
    g = torch.Generator().manual_seed(1)
    w, x, gy = (torch.randint(-3, 4, s, generator=g).double() for s in ((CO, CI, 3, 3), (2, CI, 8, 12), (2, CO, 4, 6)))
    w, xu = w.float(), _unshuffle(x)
    w2 = w.double().requires_grad_()
    F.conv2d(x, w2, stride=2, padding=1).backward(gy)
    wp = expand_fwd(w).double().requires_grad_()
    F.conv2d(xu, wp, padding=1).backward(gy)
    assert torch.equal(gather_wgrad(wp.grad, CI), w2.grad)


def test_gather_wgrad_inverts_expand_fwd(case):
    w = case[0]
    assert torch.equal(gather_wgrad(expand_fwd(w), CI), w)
