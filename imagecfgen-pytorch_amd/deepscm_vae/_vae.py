"""Shared implementation of the three DeepSCM conditional VAEs of the reference (``deepscm_vae/mnist.py``,
``audio_mnist.py``, ``whalecalls.py``): the closed form of their pyro likelihood, the ELBO, ``encoder.sample`` and the
training loop.

pyro is not needed to state the model.  ``ConditionalTransformedDistribution(MultivariateNormal(0, I),
[AffineTransform(decoder(z, c), exp(log_var / 2))]).log_prob(x)`` (mnist.py:94-116,128) is

    -0.5 * sum_p (x_p - bias_p)^2 * exp(-log_var) - P * log_var / 2 - P / 2 * log(2 pi)

(``gaussian_log_prob``; tests/test_vae_cpu.py holds it against ``torch.distributions`` in fp64), and the reference's
``(lp - kl_weight * dkl).mean()`` -- ``[B]`` against ``[B,1,1]``, a ``[B,1,B]`` broadcast -- is exactly
``lp.mean() - kl_weight * dkl.mean()``.  The models hold no ``base`` / ``dist`` objects; those carry no parameters or
buffers in the reference either, so ``state_dict`` keys are the reference's.

CUDA tensors run on the HIP kernels (``ali_hip.vae``: the stacks through ``ali_hip.chain``, csrc/vae.hip between
them); CPU tensors run the stock torch statement below.
"""
import math

import torch
import torch.nn as nn

LATENT_DIM = 512


def gaussian_log_prob(x, bias, log_var):
    """log N(x; bias, exp(log_var) I) per row of x [B, P]"""
    P = x.shape[1]
    return -0.5 * (x - bias).square().sum(dim=1) * math.exp(-log_var) - 0.5 * P * log_var - 0.5 * P * math.log(2 * math.pi)


def hip_heads(enc, feat):
    """the two 1x1 heads on the NHWC feature map [B,1,1,C] -> (mean, log_var) [B, L, 1, 1], autograd aware"""
    from ali_hip.chain import run_chain
    from ali_hip.vae import head_chains
    B = feat.shape[0]
    hm, hv = head_chains(enc)
    return (run_chain(hm, feat).reshape(B, -1, 1, 1), run_chain(hv, feat).reshape(B, -1, 1, 1))


class EncoderMixin:
    """``sample`` of the three encoders (mnist.py:58-61, audio_mnist.py:229-232, whalecalls.py:278-281): the draw is
    scaled by ``exp(log_var)`` -- the variance, not the standard deviation; that is the reference's statement."""

    def sample(self, x, c, device=None, eps=None):
        """``eps`` (optional, the shape of ``mean``): the draw, instead of ``torch.randn(mean.shape)``.  On CUDA
        tensors the result comes from ``ali_vae_latent_fwd`` (k = 1) and carries no autograd history."""
        mean, log_var = self(x, c)
        if eps is None:
            eps = torch.randn(mean.shape).to(mean.device)
        if not mean.is_cuda:
            return mean + eps * torch.exp(log_var)
        from ali_hip import ops
        B, L = mean.shape[0], mean.shape[1]
        z = torch.empty(B, L, dtype=torch.float32, device=mean.device)
        ops.vae_latent_fwd(mean.detach().reshape(B, L), log_var.detach().reshape(B, L), 1, z, k=1.0,
                           eps=eps.reshape(1, B, L).float().contiguous(), want_kl=False)
        return z.reshape(mean.shape)


class VAEBase(nn.Module):
    """encoder + decoder + the ELBO (mnist.py:105-133).  ``decoder_log_var``: log-variance of p(x | z), -5."""
    decoder_log_var = -5.0

    def elbo(self, x, c, num_samples=4, device='cpu', kl_weight=1.0, eps=None):
        """mean_b [ (1/S) sum_s log p(x_b | z_sb, c_b) - kl_weight * KL(q(z | x_b, c_b) || N(0, I)) ].
        ``eps`` (optional, [num_samples, B, LATENT_DIM]): the draws, instead of one ``torch.randn`` per sample."""
        if x.is_cuda:
            from ali_hip import vae as _hip
            return _hip.elbo(self, x, c, num_samples=num_samples, kl_weight=kl_weight, eps=eps)
        z_mean, z_log_var = self.encoder(x, c)
        z_std = torch.exp(z_log_var * .5)
        lp = 0
        x_reshaped = x.reshape((x.shape[0], -1))
        for s in range(num_samples):
            e = torch.randn(z_mean.shape).to(device) if eps is None else eps[s].reshape(z_mean.shape)
            z = z_mean + e * z_std
            lp = lp + gaussian_log_prob(x_reshaped, self.decoder(z, c).reshape(x_reshaped.shape), self.decoder_log_var)
        lp = lp / num_samples
        dkl = .5 * (torch.square(z_std) + torch.square(z_mean) - 1 - 2 * torch.log(z_std)).sum(dim=1)
        return lp.mean() - kl_weight * dkl.mean()


def reconstruct(vae, x, c, rounds=32):
    """the demo block of the train functions (mnist.py:213-217): mean of ``rounds`` sampled reconstructions"""
    from ali_hip.vae import VaeReconstructor
    return VaeReconstructor(vae, rounds=rounds, capture=False).add(x, c)


def train_on_stream(vae, stream_fn, n_epochs, l_rate, device, preprocess, attr_keys, attr_cast, num_samples, kl_weight,
                    weight_decay=0.0):
    """The loop of audio_mnist.train / whalecalls.train (audio_mnist.py:366-386) over a generator of batch dicts.
    CUDA without weight decay: the hand-scheduled ``VaeStepper`` (flat Adam, HIP graph per batch shape); with weight
    decay (whalecalls.py:388-390) the autograd ``elbo`` on the same kernels under ``torch.optim.Adam``.
    Returns (vae, optimizer, epoch means of -elbo)."""
    dev = torch.device(device)
    stepper = None
    if dev.type == "cuda" and not weight_decay:
        from ali_hip.vae import VaeStepper
        stepper = VaeStepper(vae, lr=l_rate, kl_weight=kl_weight, num_samples=num_samples, capture=True)
        optimizer = stepper.opt
    else:
        optimizer = torch.optim.Adam(vae.parameters(), lr=l_rate, weight_decay=weight_decay)
    H, W = vae.encoder.image_hw
    scores = []
    for epoch in range(n_epochs):
        vae.train()
        total = torch.zeros((), device=dev)
        n = 0
        for batch in stream_fn():
            images = batch["audio"].reshape((-1, 1, H, W)).float().to(dev)
            c = {k: torch.clone(batch[k]).to(attr_cast).to(dev) for k in attr_keys}
            if preprocess is not None:
                images = preprocess(images)
            if stepper is not None:
                eps = torch.stack([torch.randn(len(images), LATENT_DIM) for _ in range(num_samples)]).to(dev)
                total += stepper.step(images, c, eps)["loss"]
            else:
                optimizer.zero_grad()
                loss = -vae.elbo(images, c, num_samples=num_samples, device=device, kl_weight=kl_weight)
                loss.backward()
                optimizer.step()
                total += loss.detach()
            n += 1
        scores.append(total.item() / max(n, 1))
        print(f'Epoch {epoch + 1}/{n_epochs}:', scores[-1])
    return vae, optimizer, scores


def run_training(vae, data, stream_kwargs, attr_keys, n_epochs, l_rate, device, attr_cast, num_samples, kl_weight,
                 weight_decay=0.0):
    """statistics pass, ``spect_to_img``, the loop (audio_mnist.py:343-386, whalecalls.py:400-445)"""
    from image_scms import _spect
    stream = lambda: data.stream(**stream_kwargs)  # noqa: E731
    fused = hasattr(data, "fuse_spect_to_img")
    if fused:
        data.fuse_spect_to_img(None)
    mean, std, _ = _spect.spectrogram_statistics(stream, device)
    try:
        if fused:
            data.fuse_spect_to_img(mean, std, 3.0)
            prep = None
        else:
            prep = lambda s: torch.clip((s - mean) / (std + 1e-6), -3, 3) / 3.0  # noqa: E731
        vae, optimizer, _ = train_on_stream(vae, stream, n_epochs, l_rate, device, prep, attr_keys, attr_cast,
                                            num_samples, kl_weight, weight_decay)
    finally:
        if fused:
            data.fuse_spect_to_img(None)
    return vae, optimizer
