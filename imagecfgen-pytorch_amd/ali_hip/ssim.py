"""Structural similarity (SSIM) of image batches, differentiable: the ``ssim`` that the reference's
``image_scms/training_utils.py`` and ``explain/cf_example.py`` import from ``pytorch_msssim`` (``rec_loss =
1 - ssim(x, xr, data_range=1.0).mean()``, finetune_mnist_bigan.py:75-76).

For X, Y of shape [B,C,H,W]: ``g`` the fp32 Gaussian window normalised by its fp32 sum, ``F`` the separable valid
correlation with ``g`` along H, then W; C1 = (K1*data_range)^2, C2 = (K2*data_range)^2;

    mu1 = F(X), mu2 = F(Y), s1 = F(X*X) - mu1^2, s2 = F(Y*Y) - mu2^2, s12 = F(X*Y) - mu1*mu2
    cs = (2*s12 + C2) / (s1 + s2 + C2),   S = (2*mu1*mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs
    ssim_pc[b,c] = mean over the map of S

and the result is ``ssim_pc.mean()`` (``size_average``) or ``ssim_pc.mean(1)``.  Images are taken as they come (the
reference feeds [-1,1] images with ``data_range=1.0``; nothing is rescaled).

CUDA tensors (fp32 only: any other dtype raises ``ValueError``) run the kernels of csrc/ssim.hip under a
``torch.autograd.Function`` (first derivatives only); CPU tensors run the same
definition with stock torch ops.  One deviation from the library: an axis shorter than ``win_size`` raises
``ValueError`` (the library skips the filter along that axis with a warning).
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops

_WINDOWS = {}


def gaussian_window(win_size, win_sigma, device="cpu"):
    """g[i] = exp(-(i - win_size//2)^2 / (2*win_sigma^2)) / sum, in fp32; one cached tensor per device."""
    key = (int(win_size), float(win_sigma), str(device))
    g = _WINDOWS.get(key)
    if g is None:
        c = torch.arange(win_size, dtype=torch.float32) - win_size // 2
        g = torch.exp(-(c ** 2) / (2 * win_sigma ** 2))
        g = (g / g.sum()).to(device)
        _WINDOWS[key] = g
    return g


def _filter(T, g):
    C, k = T.shape[1], g.numel()
    T = F.conv2d(T, g.reshape(1, 1, k, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(T, g.reshape(1, 1, 1, k).repeat(C, 1, 1, 1), groups=C)


def _ssim_pc_torch(X, Y, g, C1, C2):
    g = g.to(X.dtype)
    mu1, mu2 = _filter(X, g), _filter(Y, g)
    s1 = _filter(X * X, g) - mu1 * mu1
    s2 = _filter(Y * Y, g) - mu2 * mu2
    s12 = _filter(X * Y, g) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    S = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs
    return S.flatten(2).mean(-1)


class _SsimPC(torch.autograd.Function):
    """ssim_pc [B,C] of CUDA fp32 images through ali_ssim_fwd / ali_ssim_bwd.  The forward launch also leaves the
    coefficient maps of whichever operand needs a gradient (the metric is symmetric: X's maps are the launch with the
    operands exchanged)."""

    @staticmethod
    def forward(ctx, X, Y, g, C1, C2):
        B, C, H, W = X.shape
        x, y = X.detach().contiguous().reshape(B * C, H, W), Y.detach().contiguous().reshape(B * C, H, W)
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        pc, maps_y = ops.ssim_fwd(x, y, g, C1, C2, want_maps=need_y)
        maps_x = ops.ssim_fwd(y, x, g, C1, C2, want_maps=True)[1] if need_x else None
        ctx.save_for_backward(X, Y, g, maps_x, maps_y)
        return pc.reshape(B, C)

    @staticmethod
    @once_differentiable
    def backward(ctx, gpc):
        X, Y, g, maps_x, maps_y = ctx.saved_tensors
        B, C, H, W = X.shape
        x, y = X.contiguous().reshape(B * C, H, W), Y.contiguous().reshape(B * C, H, W)
        gpc = gpc.contiguous().reshape(-1)
        gx = ops.ssim_bwd(y, x, maps_x, gpc, g).reshape(X.shape) if maps_x is not None else None
        gy = ops.ssim_bwd(x, y, maps_y, gpc, g).reshape(Y.shape) if maps_y is not None else None
        return gx, gy, None, None, None


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
         nonnegative_ssim=False):
    """``pytorch_msssim.ssim``: see the module docstring.  ``win`` (optional) is a 1-D window replacing the Gaussian."""
    if X.dim() != 4 or Y.dim() != 4:
        raise ValueError(f"ssim: inputs must be [B,C,H,W], got {tuple(X.shape)} and {tuple(Y.shape)}")
    if X.shape != Y.shape:
        raise ValueError(f"ssim: inputs must have the same shape, got {tuple(X.shape)} and {tuple(Y.shape)}")
    if win is not None:
        win = win.reshape(-1)
        win_size = win.numel()
    if win_size % 2 != 1:
        raise ValueError(f"ssim: win_size must be odd, got {win_size}")
    if X.shape[2] < win_size or X.shape[3] < win_size:
        raise ValueError(f"ssim: H and W must be at least win_size={win_size}, got {tuple(X.shape[2:])}")
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    if X.is_cuda:
        if X.dtype != torch.float32 or Y.dtype != torch.float32:
            raise ValueError(f"ssim: the kernels are fp32 only, got {X.dtype} and {Y.dtype} on {X.device}")
        g = gaussian_window(win_size, win_sigma, X.device) if win is None else win.to(X.device, torch.float32).contiguous()
        pc = _SsimPC.apply(X, Y, g, C1, C2)
    else:
        g = gaussian_window(win_size, win_sigma) if win is None else win
        pc = _ssim_pc_torch(X, Y, g, C1, C2)
    if nonnegative_ssim:
        pc = torch.relu(pc)
    return pc.mean() if size_average else pc.mean(1)
