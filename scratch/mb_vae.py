"""Conditional-VAE family at the training scripts' own shapes (MNIST B=64, AudioMNIST B=128, whale B=32; 4 draws per
step): one training step (VaeStepper, HIP-graph replay) and one 32-round reconstruction (VaeReconstructor, one graph)
against the stock-torch statement of the same modules on the same GPU -- the CPU path's statement run on CUDA tensors
of a plain copy of the layers: per-draw decoder passes, ``exp`` / ``randn`` / ``cat`` as ATen launches, the closed-form
log-likelihood, ``torch.optim.Adam`` -- and the three kernels of csrc/vae.hip alone against their algorithmic bytes.
Every call is timed on its own with device events after a warm-up; prints median, min and max per measurement and the
ratio of the medians.  Needs a GPU.  ``--calls N`` (default 20), ``--only FAMILY``."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from ali_hip import ops  # noqa: E402
from ali_hip.vae import VaeReconstructor, VaeStepper  # noqa: E402
from deepscm_vae._vae import gaussian_log_prob  # noqa: E402


def family(name):
    if name == "mnist":
        import deepscm_vae.mnist as m
        attrs, cont = {"digit": 10}, ("intensity", "slant", "thickness")
        return m.MorphoMNISTVAE(), attrs, cont, 28, 64
    if name == "audio":
        import deepscm_vae.audio_mnist as m
        return m.VAE(), dict(m.ATTRIBUTE_DIMS), (), 128, 128
    import deepscm_vae.whalecalls as m
    return m.WhaleCallVAE(), {"call_type": 3}, (), 256, 32


class Stock:
    """the modules' CPU statement on CUDA tensors: stock ATen / MIOpen ops of the same layers"""

    def __init__(self, vae, name):
        self.v, self.name = vae, name

    def encode(self, x, c):
        E = self.v.encoder
        if self.name == "mnist":
            from deepscm_vae.mnist import _torch_features
            up = E.layers(_torch_features(E.digit_embedding, x, c))
        else:
            up = E.layers(E._features_torch(x, c))
        return E.mean_head(up), E.log_var_head(up)

    def decode(self, z, c):
        G = self.v.decoder
        if self.name == "mnist":
            feats = [z, c["digit"].matmul(G.digit_embedding.weight).reshape(-1, 256, 1, 1)] + [
                c[k].reshape(-1, 1, 1, 1) for k in sorted(k for k in c if k != "digit")]
            return G.layers(torch.concat(feats, dim=1))
        z = z.reshape(-1, 512)
        return G.layers(torch.concat([z] + [c[k].float().matmul(G.table(k).weight) for k in G.cat_keys], dim=1))

    def elbo(self, x, c, S, klw):
        mean, lv = self.encode(x, c)
        std = torch.exp(0.5 * lv)
        xf = x.reshape(x.shape[0], -1)
        lp = 0
        for _ in range(S):
            z = mean + torch.randn(mean.shape, device=x.device) * std
            lp = lp + gaussian_log_prob(xf, self.decode(z, c).reshape(xf.shape), -5.0)
        dkl = .5 * (std.square() + mean.square() - 1 - lv).reshape(x.shape[0], -1).sum(1)
        return (lp / S).mean() - klw * dkl.mean()

    @torch.no_grad()
    def reconstruct(self, x, c, rounds):
        rec = 0
        for _ in range(rounds):
            mean, lv = self.encode(x, c)
            rec = rec + self.decode(mean + torch.randn(mean.shape, device=x.device) * torch.exp(lv), c)
        return rec / rounds


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


def report(name, what, new, old):
    print(f"{name}: {what}: HIP path median {new[0]:.3f} ms (min {new[1]:.3f}, max {new[2]:.3f}); stock torch median "
          f"{old[0]:.3f} ms (min {old[1]:.3f}, max {old[2]:.3f}); stock / HIP = {old[0] / new[0]:.2f}x", flush=True)


def kernels(name, B, S, P, ld, n_emb, calls):
    L = 512
    mean, lv = torch.randn(B, L).cuda(), torch.randn(B, L).cuda() * 0.1
    eps, rows = torch.randn(S, B, L).cuda(), torch.empty(S * B, ld).cuda()
    x, xhat = torch.rand(B, P).cuda(), torch.rand(S * B, P).cuda()
    gin, gm, gv = torch.randn(S * B, ld).cuda(), torch.empty(B, L).cuda(), torch.empty(B, L).cuda()
    for what, fn, nbytes in (
            ("latent_fwd", lambda: ops.vae_latent_fwd(mean, lv, S, rows, eps=eps), 4 * (2 * S * B * L + 2 * B * L)),
            ("loglik", lambda: ops.vae_loglik(x, xhat, S), 4 * 3 * S * B * P),
            ("latent_bwd", lambda: ops.vae_latent_bwd(gin, eps, mean, lv, S, gm, gv, ncond=256 * n_emb),
             4 * (S * B * (2 * L + 256 * n_emb) + 4 * B * L + B * 256 * n_emb))):
        med, lo, hi = timed(fn, calls)
        print(f"{name}: ali_vae_{what} B={B} S={S}: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); "
              f"{nbytes / 1e6:.2f} MB algorithmic -> {nbytes / med / 1e9:.3f} TB/s (event-timed single launches include "
              f"the launch itself)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    S, KLW, R = 4, 10.0, 32
    for name in ("mnist", "audio", "whale"):
        if a.only and name != a.only:
            continue
        torch.manual_seed(0)
        vae, attr_dims, cont, hw, B = family(name)
        vae = vae.cuda()
        c = {k: torch.eye(n)[torch.randint(0, n, (B,))].cuda() for k, n in attr_dims.items()}
        c.update({k: torch.rand(B).cuda() * 2 - 1 for k in cont})
        x = torch.rand(B, 1, hw, hw).cuda() * 2 - 1

        ref = Stock(copy.deepcopy(vae), name)
        opt = torch.optim.Adam(ref.v.parameters(), lr=1e-4)

        def stock_step():
            opt.zero_grad()
            loss = -ref.elbo(x, c, S, KLW)
            loss.backward()
            opt.step()
            return loss
        old = timed(stock_step, a.calls)
        stepper = VaeStepper(copy.deepcopy(vae), lr=1e-4, kl_weight=KLW, num_samples=S, capture=True)
        report(name, f"training step B={B} S={S}", timed(lambda: stepper.step(x, c), a.calls), old)
        del stepper, opt

        n = min(B, 10)                       # the demo block's batch (mnist.py:191)
        xs, cs = x[:n].contiguous(), {k: v[:n].contiguous() for k, v in c.items()}
        rec = VaeReconstructor(vae.eval(), rounds=R)
        report(name, f"reconstruction B={n} rounds={R}", timed(lambda: rec.add(xs, cs), a.calls),
               timed(lambda: ref.reconstruct(xs, cs, R), a.calls))
        n_emb = len(attr_dims)
        g_log = 512 + 256 * n_emb + len(cont)
        kernels(name, B, S, hw * hw, g_log + (-g_log) % 32, n_emb, a.calls)
        del rec, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
