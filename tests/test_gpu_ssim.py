"""GPU parity of the SSIM kernels (csrc/ssim.hip) and of ``FinetuneStepper(metric="ssim")``.

Yardstick for values and gradients: the fp32 evaluation of the definition with stock torch ops on the CPU, against
the fp64 evaluation of the same inputs.  The kernels may deviate from fp64 by at most 4x that (a different but equally
valid fp32 summation order), with absolute floors of 1e-6 (values) and 1e-8 (gradient max-abs).  The inputs carry the
flat -1 background of MNIST, where the variances are pure rounding noise against C2 = 9e-4.
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_callers import _check_encoder_update
from test_gpu_modules import paired_models, to_dev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 11, 11), (3, 1, 11, 13), (3, 1, 28, 28), (2, 3, 37, 50), (2, 1, 128, 128)]


def ssim_pc_ref(X, Y, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """ssim_pc [B,C] by the definition, in the dtype of X (window: fp32 Gaussian over its fp32 sum, then cast)."""
    c = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(c ** 2) / (2 * win_sigma ** 2))
    g = (g / g.sum()).to(X.dtype)
    C = X.shape[1]

    def filt(T):
        T = F.conv2d(T, g.reshape(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
        return F.conv2d(T, g.reshape(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)

    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = filt(X), filt(Y)
    s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    S = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs
    return S.flatten(2).mean(-1)


def ssim_ref(X, Y, data_range=1.0, size_average=True):
    pc = ssim_pc_ref(X, Y, data_range)
    return pc.mean() if size_average else pc.mean(1)


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs, a non-uniform cotangent of the per-image result, and the fp64 / fp32 CPU evaluations (computed once)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, C, H, W, generator=g) * 2 - 1
    x[:, :, :H // 2, :] = -1.0
    y = (x + 0.3 * torch.randn(B, C, H, W, generator=g)).clamp(-1, 1)
    y[:, :, :H // 4, :] = -1.0
    w = torch.rand(B, generator=g) + 0.5
    out = {}
    for dt in (torch.float64, torch.float32):
        xx, yy = x.to(dt).clone().requires_grad_(True), y.to(dt).clone().requires_grad_(True)
        v = ssim_ref(xx, yy, size_average=False)
        (v * w.to(dt)).sum().backward()
        out[dt] = (v.detach().double(), xx.grad.double(), yy.grad.double())
    return x, y, w, out[torch.float64], out[torch.float32]


def _gpu_eval(x, y, w):
    from ali_hip.ssim import ssim
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    v = ssim(xd, yd, data_range=1.0, size_average=False)
    (v * w.cuda()).sum().backward()
    return v.detach(), xd.grad, yd.grad


@pytest.mark.parametrize("shape", SHAPES)
def test_values_and_gradients_within_4x_of_fp32_torch(shape):
    from ali_hip.ssim import ssim
    x, y, w, (v64, gx64, gy64), (v32, gx32, gy32) = case(shape)
    v, gx, gy = _gpu_eval(x, y, w)
    assert v.shape == (shape[0],) and gx.shape == x.shape and gy.shape == y.shape
    err_v, yard_v = (v.double().cpu() - v64).abs().max().item(), (v32 - v64).abs().max().item()
    print(f"{shape} value max-abs {err_v:.3e} (fp32 torch {yard_v:.3e})")
    report = []
    for name, got, g64, g32 in (("dX", gx, gx64, gx32), ("dY", gy, gy64, gy32)):
        d, dy = got.double().cpu() - g64, g32 - g64
        rel, yrel = (d.norm() / g64.norm()).item(), (dy.norm() / g64.norm()).item()
        mx, ymx = d.abs().max().item(), dy.abs().max().item()
        print(f"{shape} {name} rel-L2 {rel:.3e} (fp32 torch {yrel:.3e}) max-abs {mx:.3e} (fp32 torch {ymx:.3e}, "
              f"max |g| {g64.abs().max().item():.3e})")
        report.append((name, rel, yrel, mx, ymx))
    assert err_v <= max(4 * yard_v, 1e-6)
    for name, rel, yrel, mx, ymx in report:
        assert rel <= 4 * yrel, (name, rel, yrel)
        assert mx <= max(4 * ymx, 1e-8), (name, mx, ymx)
    # size_average=True is the mean of the same per-plane values
    s = ssim(x.cuda(), y.cuda(), data_range=1.0)
    assert s.dim() == 0 and abs(s.item() - v64.mean().item()) <= max(4 * yard_v, 1e-6)


def test_gradient_flows_only_where_required_and_other_windows():
    from ali_hip.ssim import ssim
    x, y, w, (v64, gx64, gy64), (v32, _, gy32) = case((2, 3, 37, 50))
    yd = y.cuda().requires_grad_(True)
    xd = x.cuda()
    ssim(xd, yd, data_range=1.0, size_average=False).backward(w.cuda())
    assert xd.grad is None
    assert ((yd.grad.double().cpu() - gy64).norm() / gy64.norm()).item() <= 4 * ((gy32 - gy64).norm() / gy64.norm()).item()
    # a window size without a specialised kernel, against fp64 (random images: no cancellation; 1e-5 is ~100 fp32 ulps)
    g = torch.Generator().manual_seed(1)
    a, b = torch.rand(2, 2, 40, 33, generator=g), torch.rand(2, 2, 40, 33, generator=g)
    bd = b.cuda().requires_grad_(True)
    got = ssim(a.cuda(), bd, data_range=1.0, win_size=7, win_sigma=1.0, nonnegative_ssim=True)
    got.backward()
    b64 = b.double().requires_grad_(True)
    ref = torch.relu(ssim_pc_ref(a.double(), b64, win_size=7, win_sigma=1.0)).mean()
    ref.backward()
    assert abs(got.item() - ref.item()) <= 1e-5
    assert ((bd.grad.double().cpu() - b64.grad).norm() / b64.grad.norm()).item() <= 1e-5
    with pytest.raises(ValueError):
        ssim(a.cuda()[:, :, :10], b.cuda()[:, :, :10])
    with pytest.raises(ValueError):                      # the kernels are fp32 only
        ssim(a.cuda().double(), b.cuda().double())


@pytest.mark.parametrize("shape", [(3, 1, 28, 28), (2, 3, 37, 50), (2, 1, 128, 128)])
def test_bit_reproducible_eager_and_graph_replay(shape):
    x, y, w, _, _ = case(shape)
    first = _gpu_eval(x, y, w)
    second = _gpu_eval(x, y, w)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    from ali_hip import ops
    from ali_hip.ssim import gaussian_window
    B, C, H, W = shape
    xs, ys = x.cuda().reshape(B * C, H, W), y.cuda().reshape(B * C, H, W)
    gpc = w.cuda().repeat_interleave(C) / C
    win = gaussian_window(11, 1.5, xs.device)

    def both():
        pc, maps = ops.ssim_fwd(xs, ys, win, 1e-4, 9e-4, want_maps=True)
        return pc, ops.ssim_bwd(xs, ys, maps, gpc, win)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pc_e, gy_e = both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pc_g, gy_g = both()
    pc_g.zero_(), gy_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pc_g, pc_e) and torch.equal(gy_g, gy_e)
    assert torch.equal(pc_e.reshape(B, C).mean(1), first[0]) and torch.equal(gy_e.reshape(shape), first[2])


def _reference_finetune_ssim(E, G, x, a, lr, steps):
    """finetune_mnist_bigan.py:64-85 / finetune_audio_mnist_bigan.py:62-91 with --metric ssim, verbatim statements."""
    E.train(), G.eval()
    opt = torch.optim.Adam(E.parameters(), lr=lr)
    rec, lat = [], []
    for _ in range(steps):
        opt.zero_grad()
        codes = E(x, a)
        xr = G(codes, a)
        rec_loss = 1 - ssim_ref(x, xr, data_range=1.0).mean()
        latent = torch.square(codes).mean()
        (rec_loss + latent).backward()
        opt.step()
        rec.append(rec_loss.item()), lat.append(latent.item())
    return rec, lat


@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("family,d,B", [("mnist", 64, 4), ("audio", 8, 2)])
def test_finetune_stepper_ssim_vs_reference_statements(family, d, B, capture):
    from ali_hip.step import FinetuneStepper
    (Eo, Go, _), (E, G, _), images, c, _ = paired_models(family, d=d, B=B)
    E.train(), G.eval()
    before = copy.deepcopy(Eo.state_dict())
    lr, steps = 1e-4, 3
    rec, lat = _reference_finetune_ssim(Eo, Go, images, c, lr, steps)
    ft = FinetuneStepper(E, G, lr=lr, capture=capture, metric="ssim")
    out = []
    for _ in range(steps):
        r = ft.step(images.cuda(), to_dev(c))
        assert set(r) == {"rec", "latent"} and r["rec"].dim() == 0 and r["rec"].is_cuda
        out.append((r["rec"].item(), r["latent"].item()))
    np.testing.assert_allclose([o[0] for o in out], rec, rtol=2e-4)
    np.testing.assert_allclose([o[1] for o in out], lat, rtol=2e-4)
    _check_encoder_update(Eo, E, before, lr, steps)
    if capture:
        assert len(ft._graphs) == 1
    with pytest.raises(ValueError):
        ft.step(images.cuda().reshape(B, *images.shape[2:]), to_dev(c))


def test_finetune_stepper_mse_is_unchanged_by_the_argument():
    from ali_hip.step import FinetuneStepper
    outs = []
    for kw in ({}, {"metric": "mse"}):
        _, (E, G, _), images, c, _ = paired_models("mnist", d=64, B=4)
        E.train(), G.eval()
        ft = FinetuneStepper(E, G, lr=1e-4, **kw)
        steps = [ft.step(images.cuda(), to_dev(c)) for _ in range(2)]
        outs.append([t for r in steps for t in (r["rec"], r["latent"])] + [ft.opt_e.flat.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
