"""GAN family at the reference's shapes (bs = 64, d = 64, 128 x 128 images): one "gan" and one "wgan" iteration of
``GanStepper`` (HIP-graph replay, and eager) against the loop body of gans/audio_mnist.py:300-337 written with stock
torch on the same layers as stock ``nn.Sequential`` stacks on ROCm PyTorch (``BCEWithLogitsLoss`` /
``autograd.grad(create_graph=True)`` penalty, ``torch.optim.Adam``), and each csrc/gan.hip kernel on its own at B = 64,
P = 16384.  Every call is timed on its own with device events after a warm-up; prints median, min and max per
measurement and the ratio of the medians.  Needs a GPU.  ``--calls N`` (default 10), ``--d``, ``--bs``;
``--launches``: the kernel table (torch.profiler) of one eager wgan iteration."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import gans.audio_mnist as gm  # noqa: E402
from ali_hip import ops  # noqa: E402
from ali_hip.gan import GanStepper  # noqa: E402


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def fmt(t):
    return f"median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def stock_body(G, D, oG, oD, images, mode, lam=10.0):
    """the reference's iteration on stock modules ([B, 1, H, W] images), host draws uploaded like the reference's"""
    bce = nn.BCEWithLogitsLoss()
    n, dev = len(images), images.device
    valid, fake = torch.ones(n, 1, device=dev), torch.zeros(n, 1, device=dev)

    def body():
        z = torch.randn(n, 100).to(dev)
        oG.zero_grad()
        loss_G = bce(D(G(z)), valid) if mode == "gan" else -D(G(z)).mean()
        loss_G.backward()
        oG.step()
        oD.zero_grad()
        z = torch.randn(n, 100).to(dev)
        if mode == "gan":
            loss_D = (bce(D(images), valid) + bce(D(G(z)), fake)) / 2
        else:
            x_fake = G(z)
            eps = torch.rand(n, 1, 1, 1).to(dev)
            xhat = (eps * images + (1 - eps) * x_fake).requires_grad_(True)
            grad = torch.autograd.grad(D(xhat), xhat, torch.ones(n, 1, device=dev), create_graph=True)[0]
            pen = ((grad.view(n, -1).norm(2, dim=1) - 1) ** 2).mean()
            loss_D = (D(x_fake) - D(images) + lam * pen).mean()
        loss_D.backward()
        oD.step()
        z = torch.randn(n, 100).to(dev)
        with torch.no_grad():
            DG, DE = D(G(z)), D(images)
            if mode == "gan":
                DG, DE = DG.sigmoid(), DE.sigmoid()
        return DG.mean(), DE.mean()
    return body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--launches", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    torch.manual_seed(0)
    ops.set_workspace_bytes(1 << 30)
    B, d = a.bs, a.d
    G0, D0 = gm.Generator(d), gm.Discriminator(d)
    G0.apply(gm.init_weights), D0.apply(gm.init_weights)
    images = (torch.rand(B, 1, 128, 128) * 2 - 1).cuda()

    # ---- the kernels of csrc/gan.hip on their own
    P = 128 * 128
    xr, xf = torch.randn(B, P).cuda(), torch.randn(B, P).cuda()
    eps, ctr = torch.rand(B).cuda(), torch.zeros(1, dtype=torch.int64).cuda()
    out = torch.empty_like(xr)
    lf, lr_ = torch.randn(B).cuda(), torch.randn(B).cuda()
    print(f"ali_gp_mix (eps given) B={B} P={P}: {fmt(timed(lambda: ops.gp_mix(xr, xf, eps=eps, out=out), a.calls))}")
    print(f"ali_gp_mix (eps drawn) B={B} P={P}: {fmt(timed(lambda: ops.gp_mix(xr, xf, seed=1, dev_counter=ctr, out=out), a.calls))}")
    print(f"ali_gp_penalty B={B} P={P}: {fmt(timed(lambda: ops.gp_penalty(xr, 10.0, out=out), a.calls))}")
    print(f"ali_gp_penalty (v aliased) B={B} P={P}: {fmt(timed(lambda: ops.gp_penalty(out, 10.0, out=out), a.calls))}")
    print(f"ali_wgan_critic B={B}: {fmt(timed(lambda: ops.wgan_critic(lf, lr_), a.calls))}", flush=True)

    for mode in ("gan", "wgan"):
        res = {}
        for capture in (True, False):
            stepper = GanStepper(copy.deepcopy(G0).cuda(), copy.deepcopy(D0).cuda(), loss_mode=mode, capture=capture)
            res[capture] = timed(lambda: stepper.step(images), a.calls)
            del stepper
            torch.cuda.empty_cache()
        Gs = nn.Sequential(*copy.deepcopy(list(G0.layers.children()))).cuda()
        Ds = nn.Sequential(*copy.deepcopy(list(D0.layers.children()))).cuda()
        oG = torch.optim.Adam(Gs.parameters(), lr=1e-4, betas=(0.5, 0.9))
        oD = torch.optim.Adam(Ds.parameters(), lr=1e-4, betas=(0.5, 0.9))
        stock = timed(stock_body(Gs, Ds, oG, oD, images, mode), a.calls)
        del Gs, Ds, oG, oD
        torch.cuda.empty_cache()
        print(f"{mode} iteration bs={B} d={d}: GanStepper graph {fmt(res[True])}; eager {fmt(res[False])}; stock torch "
              f"{fmt(stock)}; stock / graph = {stock[0] / res[True][0]:.2f}x, stock / eager = {stock[0] / res[False][0]:.2f}x",
              flush=True)

    if a.launches:
        from torch.profiler import ProfilerActivity, profile
        stepper = GanStepper(copy.deepcopy(G0).cuda(), copy.deepcopy(D0).cuda(), loss_mode="wgan", capture=False)
        for _ in range(2):
            stepper.step(images)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            stepper.step(images)
            torch.cuda.synchronize()
        print(prof.key_averages().table(sort_by="cuda_time_total", row_limit=30, max_name_column_width=70))


if __name__ == "__main__":
    main()
