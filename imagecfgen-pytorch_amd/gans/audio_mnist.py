"""Unconditional AudioMNIST spectrogram GAN / WGAN-GP -- drop-in for the reference's ``gans/audio_mnist.py``
(VALIDATION_RUNS :16, init_weights :19-24, compute_gradient_penalty :27-46, wgan_loss_it :49-61, constants :64-65,
Generator :168-197, Discriminator :200-224, train :227-391): the same names, constructor arguments, layer order and
``state_dict`` keys (``layers.0.weight`` ... ``layers.11.weight``).

CPU tensors run the stock ``nn.Sequential`` modules under stock autograd (``create_graph=True`` in the penalty
included).  CUDA tensors run on the HIP kernels: ``G(z)`` and ``D(x)`` are one autograd node each
(``ali_hip.chain.run_chain``), the penalty is ``ali_hip.gan.GradientPenaltyFn`` -- a tangent forward pass instead of a
double backward -- and ``train`` runs the hand-scheduled ``ali_hip.gan.GanStepper``.

The zip / wav reader (``AudioMNISTData``, :68-165) is the step before the hot path and is not re-implemented: ``train``
takes a data source with its interface (``image_scms._spect.WaveformData``) where the reference takes the zip path.
The demo-image / wav dump (:341-389, matplotlib) is not part of the path."""
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from image_scms import _spect

np.random.seed(42)   # the reference seeds numpy at import time (:15)
VALIDATION_RUNS = np.random.randint(0, 50, size=(10,)).tolist()   # (:16; unused by ``train``, which streams every run)

LATENT_DIM = 100
IMAGE_SHAPE = (128, 128)

AudioMNISTData = _spect.data_adapter_unavailable("AudioMNISTData", "torchaudio, librosa, sklearn")


def init_weights(layer, std=0.001):
    """N(0, std) on modules whose class name starts with 'Conv' (Conv2d, ConvTranspose2d; NOT the Linears), zero bias"""
    if layer.__class__.__name__.startswith('Conv'):
        torch.nn.init.normal_(layer.weight, mean=0, std=std)
        if layer.bias is not None:
            torch.nn.init.constant_(layer.bias, 0)


def compute_gradient_penalty(disc: nn.Module, interpolates: torch.Tensor):
    """WGAN-GP penalty mean_b (||d D(x_b) / d x_b||_2 - 1)^2 at ``interpolates`` (unweighted)."""
    if interpolates.is_cuda and isinstance(disc, Discriminator):
        from ali_hip.gan import gradient_penalty
        return gradient_penalty(disc, interpolates)
    interpolates = interpolates.requires_grad_(True)
    d_interpolates = disc(interpolates)
    gradients = torch.autograd.grad(outputs=d_interpolates, inputs=interpolates,
                                    grad_outputs=torch.ones_like(d_interpolates), create_graph=True,
                                    retain_graph=True, only_inputs=True)[0]
    gradients = gradients.view(gradients.size(0), -1)
    return ((gradients.norm(2, dim=1) - 1) ** 2).mean()


def wgan_loss_it(disc: nn.Module, x_real: torch.Tensor, x_fake: torch.Tensor, penalty_weight=10.0) -> torch.Tensor:
    """per-sample critic loss D(x_fake) - D(x_real) [B, 1] plus ``penalty_weight`` times the gradient penalty at
    eps * x_real + (1 - eps) * x_fake, eps ~ U[0, 1) per sample (host draw, like the reference)"""
    assert x_real.shape[0] == x_fake.shape[0], "batch size must be constant"
    loss_no_penalty = disc(x_fake) - disc(x_real)
    eps = torch.rand((x_real.shape[0], 1, 1, 1)).to(x_real.device)
    x_rand = eps * x_real + (1 - eps) * x_fake
    return loss_no_penalty + penalty_weight * compute_gradient_penalty(disc, x_rand)


class Generator(nn.Module):
    def __init__(self, d=64):
        super().__init__()
        ct2d = partial(nn.ConvTranspose2d, stride=2, padding=2, output_padding=1)
        self.layers = nn.Sequential(
            nn.Linear(LATENT_DIM, 256 * d), nn.Unflatten(1, (16 * d, 4, 4)), nn.LeakyReLU(0.2),
            ct2d(16 * d, 8 * d, (5, 5)), nn.LeakyReLU(0.2),
            ct2d(8 * d, 4 * d, (5, 5)), nn.LeakyReLU(0.2),
            ct2d(4 * d, 2 * d, (5, 5)), nn.LeakyReLU(0.2),
            ct2d(2 * d, d, (5, 5)), nn.LeakyReLU(0.2),
            ct2d(d, 1, (5, 5)), nn.Tanh())

    @property
    def device(self):
        return next(self.parameters()).device

    def forward(self, z: torch.Tensor):
        z = z.reshape((-1, LATENT_DIM))
        if not z.is_cuda:
            return self.layers(z)
        from ali_hip.chain import run_chain
        from ali_hip.gan import g_input
        y = run_chain(self.layers, g_input(z), LATENT_DIM)          # NHWC [B, H, W, 1]: the memory of [B, 1, H, W]
        return y.reshape(y.shape[0], 1, y.shape[1], y.shape[2])


class Discriminator(nn.Module):
    def __init__(self, d=64):
        super().__init__()
        c2d = partial(nn.Conv2d, kernel_size=(5, 5), stride=(2, 2))
        self.layers = nn.Sequential(
            c2d(1, d), nn.LeakyReLU(0.2),
            c2d(d, 2 * d), nn.LeakyReLU(0.2),
            c2d(2 * d, 4 * d), nn.LeakyReLU(0.2),
            c2d(4 * d, 8 * d), nn.LeakyReLU(0.2),
            c2d(8 * d, 16 * d), nn.LeakyReLU(0.2),
            nn.Flatten(),
            nn.Linear(16 * d, 1))

    @property
    def device(self):
        return next(self.parameters()).device

    def forward(self, X: torch.Tensor):
        X = X.reshape((-1, 1, *IMAGE_SHAPE))
        if not X.is_cuda:
            return self.layers(X)
        from ali_hip.chain import run_chain
        from ali_hip.gan import d_input
        return run_chain(self.layers, d_input(X), 1).reshape(X.shape[0], 1)


def _loop_body(G, D, optimizer_G, optimizer_D, images, ctr, d_updates_per_g_update, loss_mode, gan_loss):
    """one iteration of the reference loop (:300-337) under autograd (CPU devices): (DG mean, DE mean) as tensors"""
    device = images.device
    n = len(images)
    valid = torch.ones(n, 1, device=device)
    fake = torch.zeros(n, 1, device=device)
    if ctr % d_updates_per_g_update == 0:
        z = torch.randn((n, LATENT_DIM)).to(device)
        optimizer_G.zero_grad()
        if loss_mode == "gan":
            loss_G = gan_loss(D(G(z)), valid)
        else:
            loss_G = -D(G(z)).mean()
        loss_G.backward()
        optimizer_G.step()
    optimizer_D.zero_grad()
    z = torch.randn((n, LATENT_DIM)).to(device)
    if loss_mode == "gan":
        loss_D = (gan_loss(D(images), valid) + gan_loss(D(G(z)), fake)) / 2
    else:
        loss_D = wgan_loss_it(D, images, G(z)).mean()
    loss_D.backward()
    optimizer_D.step()
    z = torch.randn((n, LATENT_DIM)).to(device)
    with torch.no_grad():
        DG, DE = D(G(z)), D(images)
        if loss_mode == "gan":
            DG, DE = DG.sigmoid(), DE.sigmoid()
    return DG.mean(), DE.mean()


def train(path_to_zip,
          n_epochs=200,
          l_rate=1e-4,
          device='cpu',
          save_images_every=1,
          batch_size=64,
          image_output_path='',
          generator_size=64,
          discriminator_size=64,
          d_updates_per_g_update=1,
          discriminator_weight_decay=0.0,
          loss_mode="gan"):
    """Reference signature and loop: statistics pass over the stream, ``spect_to_img`` standardisation, GAN or WGAN-GP
    iterations with Adam betas (0.5, 0.9).  ``path_to_zip``: the AudioMNIST zip (needs the reference's reader -- raises
    ImportError) or a data source, e.g. ``_spect.WaveformData(waveforms, {}, **image_scms.audio_mnist.STFT,
    device=device)``.  On a CUDA device the iterations are ``ali_hip.gan.GanStepper``'s (latents drawn on the device;
    the returned optimisers are its flat Adam groups), on the CPU the modules under autograd with ``torch.optim.Adam``.
    ``save_images_every`` / ``image_output_path`` are accepted and unused (no demo dump).
    Returns (G, D, optimizer_D, optimizer_G)."""
    if loss_mode not in ("gan", "wgan"):
        raise NotImplementedError(loss_mode)
    G = Generator(generator_size).to(device)
    D = Discriminator(discriminator_size).to(device)
    G.apply(init_weights)
    D.apply(init_weights)
    data = path_to_zip if _spect.is_data_source(path_to_zip) else AudioMNISTData(path_to_zip, device=device)
    stream = lambda: data.stream(batch_size=batch_size)  # noqa: E731
    mean, std, n_batches = _spect.spectrogram_statistics(stream, device)
    on_device = torch.device(device).type == "cuda"
    if on_device:
        from ali_hip.gan import GanStepper
        stepper = GanStepper(G, D, lr=l_rate, betas=(0.5, 0.9), loss_mode=loss_mode,
                             d_updates_per_g_update=d_updates_per_g_update, capture=True,
                             discriminator_weight_decay=discriminator_weight_decay)
        optimizer_G, optimizer_D = stepper.opt_g, stepper.opt_d
    else:
        optimizer_G = torch.optim.Adam(G.parameters(), lr=l_rate, betas=(0.5, 0.9))
        optimizer_D = torch.optim.Adam(D.parameters(), lr=l_rate, betas=(0.5, 0.9),
                                       weight_decay=discriminator_weight_decay)
    gan_loss = nn.BCEWithLogitsLoss()
    ctr = 0
    for epoch in range(n_epochs):
        D.train()
        G.train()
        d_score = torch.zeros((), device=device)
        eg_score = torch.zeros((), device=device)
        for batch in stream():
            images = torch.clip((batch["audio"].float().to(device) - mean) / (std + 1e-6), -3, 3) / 3.0
            if on_device:
                r = stepper.step(images.reshape((-1, 1) + IMAGE_SHAPE))
                dg, de = r["DG"], r["DE"]
            else:
                dg, de = _loop_body(G, D, optimizer_G, optimizer_D, images, ctr, d_updates_per_g_update, loss_mode,
                                    gan_loss)
            ctr += 1
            d_score += dg                      # on the device: one host read per epoch
            eg_score += de
        print(d_score.item() / max(n_batches, 1), eg_score.item() / max(n_batches, 1))
    return G, D, optimizer_D, optimizer_G
