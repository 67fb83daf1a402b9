"""MorphoMNIST conditional VAE -- drop-in for the reference's ``deepscm_vae/mnist.py`` (VAEEncoder :21-61, VAEDecoder
:64-91, MorphoMNISTVAE :105-133, train :136-242).  Same class names, constructor order (=> identical RNG consumption
and ``state_dict`` keys), same signatures; no pyro (``_vae``).  The encoder stack is ``image_scms.mnist.Encoder.layers``
plus a trailing ``LeakyReLU(0.2)``, the decoder stack ``Generator.layers``; on CUDA tensors they run through
``ali_hip.chain`` and the ELBO through csrc/vae.hip, on CPU tensors the stock torch ops of the same modules."""
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from image_scms.mnist import (Generator, _cont_keys, _hip_features, _plane_embedding, _scale_batch, _torch_features,
                              continuous_feature_map)  # noqa: F401

from . import _vae
from .training_utils import batchify, batchify_dict, init_weights

LATENT_DIM = 512
N_CONTINUOUS = 3
AttributeDict = Dict[str, torch.Tensor]
_IMG = 28


class VAEEncoder(_vae.EncoderMixin, nn.Module):
    def __init__(self):
        super().__init__()
        self.digit_embedding = _plane_embedding()
        mods = []
        for ci, co, k, p in [(1 + N_CONTINUOUS + 1, 64, 3, 1), (64, 128, 4, 1), (128, 256, 4, 1), (256, 512, 4, 1)]:
            mods += [nn.Conv2d(ci, co, (k, k), (2, 2), p), nn.LeakyReLU(0.2)]
        mods += [nn.Conv2d(512, LATENT_DIM, (1, 1), (2, 2)), nn.LeakyReLU(0.2)]
        self.layers = nn.Sequential(*mods)
        self.mean_linear = nn.Conv2d(LATENT_DIM, LATENT_DIM, (1, 1))
        self.log_var_linear = nn.Conv2d(LATENT_DIM, LATENT_DIM, (1, 1))

    mean_head = property(lambda self: self.mean_linear)
    log_var_head = property(lambda self: self.log_var_linear)

    def forward(self, X: torch.Tensor, c: AttributeDict):
        if not X.is_cuda:
            upstream = self.layers(_torch_features(self.digit_embedding, X, c))
            return self.mean_linear(upstream), self.log_var_linear(upstream)
        from ali_hip.chain import run_chain
        x0, n_log = _hip_features(self.digit_embedding, X, c)
        return _vae.hip_heads(self, run_chain(self.layers, x0, n_log))


class VAEDecoder(Generator):
    """``Generator`` verbatim: ``digit_embedding`` then ``layers`` (mnist.py:64-91)"""


class MorphoMNISTVAE(_vae.VAEBase):
    def __init__(self, device='cpu'):
        super().__init__()
        self.encoder = VAEEncoder().to(device)
        self.decoder = VAEDecoder().to(device)

    def forward(self, x: torch.Tensor, c: AttributeDict, num_samples=10):
        return self.elbo(x, c, num_samples=num_samples)


def train(x_train: torch.Tensor,
          a_train: AttributeDict,
          x_test=None,
          a_test=None,
          n_epochs=200,
          l_rate=1e-4,
          device='cpu',
          save_images_every=1,
          image_output_path='.',
          num_samples_per_step=4,
          kl_weight=10,
          batch_size=64):
    """Same signature, RNG order and return value as the reference's train (mnist.py:136-242).  On a CUDA device the
    iteration runs on the hand-scheduled ``ali_hip.vae.VaeStepper`` (HIP-graph replay) with the draws made on the host
    in the reference's order; the returned optimiser is then its flat Adam group.  The demo reconstruction
    (:213-217) runs on ``VaeReconstructor``; the matplotlib dump stays with the reference."""
    vae = MorphoMNISTVAE(device=device)
    vae.encoder.apply(init_weights)
    vae.decoder.apply(init_weights)
    dev = torch.device(device)
    stepper = None
    if dev.type == "cuda":
        from ali_hip.vae import VaeStepper
        stepper = VaeStepper(vae, lr=l_rate, kl_weight=kl_weight, num_samples=num_samples_per_step, capture=True)
        optimizer = stepper.opt
    else:
        optimizer = torch.optim.Adam(vae.parameters(), lr=l_rate)

    for epoch in range(n_epochs):
        epoch_elbo = torch.zeros((), device=dev)
        vae.train()
        num_batches = 0
        perm = np.random.permutation(len(x_train))
        img_batches = batchify(x_train[perm], batch_size=batch_size)
        attr_batches = batchify_dict({k: v[perm] for k, v in a_train.items()}, batch_size=batch_size)
        attr_stats = {k: (v.min(dim=0).values, v.max(dim=0).values) for k, v in a_train.items() if k != "digit"}
        for (images,), attrs in zip(img_batches, attr_batches):
            num_batches += 1
            images, c = _scale_batch(images, attrs, attr_stats, device)
            if stepper is not None:
                eps = torch.stack([torch.randn(len(images), LATENT_DIM, 1, 1)
                                   for _ in range(num_samples_per_step)]).to(dev)
                epoch_elbo += stepper.step(images, c, eps)["loss"]
            else:
                optimizer.zero_grad()
                elbo_loss = -vae.elbo(images, c, num_samples=num_samples_per_step, device=device, kl_weight=kl_weight)
                elbo_loss.backward()
                optimizer.step()
                epoch_elbo += elbo_loss.detach()
        print(epoch_elbo.item() / num_batches)

        if save_images_every and (epoch + 1) % save_images_every == 0 and x_test is not None:
            _save_demo(vae, x_test, a_test, attr_stats, device, epoch, image_output_path)
    return vae, optimizer


def _save_demo(vae, x_test, a_test, attr_stats, device, epoch, path, n_show=10):
    """generated / real / reconstructed rows for the first test digits (reference :190-240); the reconstruction is the
    mean of 32 sampled ones, one batched decoder pass (``VaeReconstructor``)"""
    vae.eval()
    with torch.no_grad():
        x, c = _scale_batch(x_test[:n_show], {k: v[:n_show] for k, v in a_test.items()}, attr_stats, device)
        z = torch.randn(len(x), LATENT_DIM, 1, 1).to(device)
        rows = [vae.decoder(z, c).reshape(n_show, _IMG, _IMG).cpu().numpy(),
                2 * x_test[:n_show].cpu().numpy() / 255 - 1,
                _vae.reconstruct(vae, x, c, rounds=32).reshape(n_show, _IMG, _IMG).cpu().numpy()]
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(3, n_show, figsize=(15, 5))
    fig.suptitle(f'Epoch {epoch + 1}')
    for r, (row, label) in enumerate(zip(rows, ('Generated', 'Original', 'Reconstructed'))):
        fig.text(0, 0.75 - 0.25 * r, label, ha='left')
        for j in range(n_show):
            ax[r, j].imshow(row[j], cmap='gray', vmin=-1, vmax=1)
            ax[r, j].axis('off')
    plt.savefig(f'{path}/epoch-{epoch + 1}.png')
    plt.close()
