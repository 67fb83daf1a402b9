"""``ali_hip.ssim.ssim`` on CPU tensors (stock torch ops) against an fp64 restatement of the SSIM definition, and the
binding of ``image_scms.training_utils.ssim`` to it where ``pytorch_msssim`` is absent."""
import importlib.util

import pytest
import torch
import torch.nn.functional as F

from ali_hip.ssim import ssim


def ssim_ref(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03),
             nonnegative_ssim=False):
    """The definition in fp64 (window: fp32 Gaussian over its fp32 sum, then widened)."""
    c = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(c ** 2) / (2 * win_sigma ** 2))
    g = (g / g.sum()).double()
    X, Y = X.double(), Y.double()
    C = X.shape[1]

    def filt(T):
        T = F.conv2d(T, g.reshape(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
        return F.conv2d(T, g.reshape(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)

    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = filt(X), filt(Y)
    s1, s2, s12 = filt(X * X) - mu1 ** 2, filt(Y * Y) - mu2 ** 2, filt(X * Y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    S = (2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1) * cs
    pc = S.flatten(2).mean(-1)
    if nonnegative_ssim:
        pc = torch.relu(pc)
    return pc.mean() if size_average else pc.mean(1)


def _pair(B, C, H, W, seed=0, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g) * 2 - 1
    y = (x + noise * torch.randn(B, C, H, W, generator=g)).clamp(-1, 1)
    return x, y


@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (3, 1, 28, 28), (2, 3, 37, 50)])
@pytest.mark.parametrize("data_range", [1.0, 255])
def test_matches_fp64_restatement(shape, data_range):
    x, y = _pair(*shape)
    for size_average in (True, False):
        got = ssim(x, y, data_range=data_range, size_average=size_average)
        ref = ssim_ref(x, y, data_range=data_range, size_average=size_average)
        assert got.shape == ref.shape and got.dtype == torch.float32
        # fp32 evaluation of cancelling moments: ~1e-7 of noise against C2 = (0.03*data_range)^2 in the denominator
        assert (got.double() - ref).abs().max().item() <= 2e-5
    got = ssim(x.double(), y.double(), data_range=data_range)
    assert abs(got.item() - ssim_ref(x, y, data_range=data_range).item()) <= 1e-12


def test_identity_symmetry_and_shapes():
    x, y = _pair(4, 2, 20, 23, seed=1)
    assert abs(ssim(x, x, data_range=1.0).item() - 1.0) <= 1e-6
    per_image = ssim(x, x, data_range=1.0, size_average=False)
    assert per_image.shape == (4,) and (per_image - 1.0).abs().max().item() <= 1e-6
    assert abs(ssim(x, y, data_range=1.0).item() - ssim(y, x, data_range=1.0).item()) <= 1e-6
    assert ssim(x, y, data_range=1.0).dim() == 0
    assert ssim(x, y, data_range=1.0, win_size=7).item() == pytest.approx(
        ssim_ref(x, y, data_range=1.0, win_size=7).item(), abs=2e-5)
    box = torch.full((5,), 0.2)
    assert ssim(x, y, data_range=1.0, win=box).item() == pytest.approx(
        ssim(x, y, data_range=1.0, win=box.reshape(1, 1, 1, 5)).item(), abs=0)


def test_nonnegative_ssim():
    x = (_pair(3, 1, 16, 16, seed=2)[0] + 1) / 2
    y = 1 - x                                           # positive means, negative covariance: negative SSIM
    raw = ssim(x, y, data_range=1.0, size_average=False)
    assert (raw < 0).all()
    assert torch.equal(ssim(x, y, data_range=1.0, size_average=False, nonnegative_ssim=True), torch.zeros(3))
    assert ssim(x, y, data_range=1.0, nonnegative_ssim=True).item() == 0.0
    ref = ssim_ref(x, y, data_range=1.0, size_average=False)
    assert (raw.double() - ref).abs().max().item() <= 2e-5


def test_value_errors():
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError):
        ssim(x[0], x[0])
    with pytest.raises(ValueError):
        ssim(x.unsqueeze(2), x.unsqueeze(2))
    with pytest.raises(ValueError):
        ssim(x, torch.zeros(2, 1, 16, 17))
    with pytest.raises(ValueError):
        ssim(x, x, win_size=10)
    with pytest.raises(ValueError):
        ssim(torch.zeros(2, 1, 10, 16), torch.zeros(2, 1, 10, 16))
    with pytest.raises(ValueError):
        ssim(torch.zeros(2, 1, 16, 10), torch.zeros(2, 1, 16, 10))


def test_gradcheck_fp64():
    x, y = _pair(2, 1, 12, 13, seed=3)
    x, y = x.double().requires_grad_(True), y.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ssim(a, b, data_range=1.0, size_average=False), (x, y))
    assert torch.autograd.gradcheck(lambda a, b: ssim(a, b, data_range=1.0), (x, y))


def test_gradient_matches_restatement():
    x, y = _pair(2, 2, 14, 17, seed=4)
    w = torch.tensor([0.3, 1.7])
    yp = y.clone().requires_grad_(True)
    (ssim(x, yp, data_range=1.0, size_average=False) * w).sum().backward()
    yr = y.double().requires_grad_(True)
    (ssim_ref(x, yr, data_range=1.0, size_average=False) * w.double()).sum().backward()
    assert ((yp.grad.double() - yr.grad).norm() / yr.grad.norm()).item() <= 1e-4


def test_training_utils_binds_it():
    from image_scms import training_utils as tu
    if importlib.util.find_spec("pytorch_msssim") is None:
        assert tu.ssim is ssim
    else:                                               # an installed pytorch_msssim keeps precedence
        assert tu.ssim.__module__.startswith("pytorch_msssim")

    class Id(torch.nn.Module):
        def forward(self, v, *a):
            return v

    ali = tu.AdversariallyLearnedInference(Id(), Id(), Id())
    x, _ = _pair(2, 1, 28, 28, seed=5)
    assert abs(ali.rec_loss(x).item()) <= 1e-6          # the default metric='ssim' runs: 1 - ssim(x, x)


def test_finetune_stepper_rejects_unknown_metric():
    from ali_hip.step import FinetuneStepper
    with pytest.raises(ValueError):
        FinetuneStepper(None, None, metric="psnr")
