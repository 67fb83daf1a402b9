"""``Flatten -> Linear`` as a stage of ``ali_hip.chain``: a small classifier stack against fp64 autograd.

    Conv2d(1, 8, 3) - LeakyReLU - Conv2d(8, 12, 3, stride 2) - LeakyReLU - Flatten - Linear(240, 7) - LeakyReLU - Linear(7, 5)

on a B = 3 batch of 1 x 11 x 14 images: the map in front of the Flatten is 12 x 4 x 5 -- rectangular, channels no power
of two -- so an NCHW / NHWC or an h / w mix-up in the Flatten stage's packs or weight gradient cannot cancel.
Reference: the stock modules under autograd on the CPU in fp64; yardstick: the same in CPU fp32; bounds as in
test_gpu_xent.py (4 x the CPU-fp32 error, 2e-4 of max|ref64|), for the logits, the input gradient and every parameter
gradient.  The inputs are re-seeded until the fp64 forward has no LeakyReLU input within fp32 noise of zero
(``TieWatch`` of test_gpu_modules.py), and the comparison pass is strict about it.
"""
import copy

import pytest
import torch
import torch.nn as nn

from test_gpu_modules import TieWatch, tie_free
from test_gpu_xent import _check

gpu = pytest.mark.gpu


def small_stack():
    from classifiers._stack import ClassifierStack
    torch.manual_seed(21)
    return ClassifierStack(nn.Conv2d(1, 8, 3), nn.LeakyReLU(0.2), nn.Conv2d(8, 12, 3, 2), nn.LeakyReLU(0.2), nn.Flatten(),
                           nn.Linear(240, 7), nn.LeakyReLU(0.2), nn.Linear(7, 5))


def autograd_pass(model, x, cot, dtype=None, device="cpu"):
    """(logits, input gradient, {name: parameter gradient}) of ``sum(model(x) * cot)``"""
    m = copy.deepcopy(model)
    x, cot = x.detach().clone(), cot.detach().clone()          # (a leaf of this pass alone)
    if dtype is not None:
        m = m.to(dtype)
        x, cot = x.to(dtype), cot.to(dtype)
    m, x, cot = m.to(device), x.to(device).requires_grad_(True), cot.to(device)
    y = m(x)
    y.backward(cot)
    return y.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}


def compare_with_autograd(model, x, cot, what):
    """device pass of ``model`` against the fp64 reference with the CPU-fp32 yardstick; ``x`` must be tie free"""
    ref64 = copy.deepcopy(model).double()
    with TieWatch(ref64, strict=True), torch.no_grad():
        ref64(x.double())
    y64, gx64, gp64 = autograd_pass(model, x, cot, torch.float64)
    y32, gx32, gp32 = autograd_pass(model, x, cot, torch.float32)
    yd, gxd, gpd = autograd_pass(model, x, cot, device="cuda")
    _check(f"{what} logits", yd, y64, y32)
    _check(f"{what} input grad", gxd, gx64, gx32)
    for k in gp64:
        _check(f"{what} {k}.grad", gpd[k], gp64[k], gp32[k])


@gpu
def test_flatten_linear_stage_forward_and_gradients():
    model = small_stack()
    ref64 = copy.deepcopy(model).double()

    def make(v):
        g = torch.Generator().manual_seed(40 + v)
        return torch.randn(3, 1, 11, 14, generator=g), torch.randn(3, 5, generator=g)
    x, cot = tie_free([ref64], make, lambda x, cot: ref64(x.double()))
    compare_with_autograd(model, x, cot, "small stack")


@gpu
def test_flatten_on_a_1x1_map_is_a_plain_linear():
    from classifiers._stack import ClassifierStack
    torch.manual_seed(22)
    model = ClassifierStack(nn.Conv2d(1, 8, (3, 4)), nn.LeakyReLU(0.2), nn.Flatten(), nn.Linear(8, 4))
    ref64 = copy.deepcopy(model).double()

    def make(v):
        g = torch.Generator().manual_seed(50 + v)
        return torch.randn(2, 1, 3, 4, generator=g), torch.randn(2, 4, generator=g)
    x, cot = tie_free([ref64], make, lambda x, cot: ref64(x.double()))
    compare_with_autograd(model, x, cot, "1x1 map")


@gpu
def test_wrong_in_features_is_reported_at_the_first_forward():
    from classifiers._stack import ClassifierStack
    model = ClassifierStack(nn.Conv2d(1, 8, 3), nn.LeakyReLU(0.2), nn.Flatten(), nn.Linear(100, 4)).cuda()
    with pytest.raises(ValueError, match="in_features=100"):
        model(torch.zeros(2, 1, 6, 7, device="cuda"))
