"""AudioMNIST conditional VAE -- drop-in for the reference's ``deepscm_vae/audio_mnist.py`` (constants :17-30,
init_weights :33-38, VAEEncoder :176-232, VAEDecoder :235-278, VAE :292-320, train :323-453).  The stacks are the
``c2d(5, stride 2, padding 1)`` / ``Linear -> Unflatten -> ct2d(5, stride 2, padding 2, output_padding 1)`` shapes of
``image_scms._spect`` without BatchNorm or Dropout.  The zip / wav reader (``AudioMNISTData``, :41-173) is the step
before the hot path and is not re-implemented: ``train`` takes a data source (``image_scms._spect.WaveformData``)
where the reference takes the zip path, as ``image_scms.audio_mnist.train`` does."""
import numpy as np
import torch
import torch.nn as nn

from image_scms import _spect
from image_scms._spect import init_weights  # noqa: F401  (std=0.001, reference :33)

from . import _vae

np.random.seed(42)   # the reference seeds numpy at import time (:17)
VALIDATION_RUNS = [38, 7, 42, 10, 14, 18, 20, 22, 28]

LATENT_DIM = 512
ATTRIBUTE_COUNT = 47
IMAGE_SHAPE = (128, 128)
ATTRIBUTE_DIMS = {
    "country_of_origin": 13,
    "native_speaker": 2,
    "accent": 15,
    "digit": 10,
    "age": 5,
    "gender": 2
}
_KEYS = tuple(sorted(ATTRIBUTE_DIMS.keys()))

AudioMNISTData = _spect.data_adapter_unavailable("AudioMNISTData", "torchaudio, librosa")


class _Family:
    image_hw = IMAGE_SHAPE
    cat_keys = _KEYS
    cont_key = None

    def plane_module(self, k):
        return self.embedding_dict[k]

    def table(self, k):
        return self.embedding_dict[k]


class VAEEncoder(_Family, _vae.EncoderMixin, _spect.SpectBase):
    def __init__(self, d=64):
        super().__init__()
        self.embedding_dict = nn.ModuleDict({k: _spect.plane_embedding(v, 8) for k, v in ATTRIBUTE_DIMS.items()})
        self.layers = nn.Sequential(*_spect.conv_stack(len(ATTRIBUTE_DIMS) + 1, [1, 2, 4, 8, 16, None], d),
                                    nn.LeakyReLU(0.2))
        self.mean = nn.Conv2d(LATENT_DIM, LATENT_DIM, (1, 1), stride=(1, 1))     # (reference: padding="same", no-op)
        self.log_var = nn.Conv2d(LATENT_DIM, LATENT_DIM, (1, 1), stride=(1, 1))

    mean_head = property(lambda self: self.mean)
    log_var_head = property(lambda self: self.log_var)

    def forward(self, X, a):
        if not X.is_cuda:
            feat = self.layers(self._features_torch(X, a))
            return self.mean(feat), self.log_var(feat)
        from ali_hip.chain import run_chain
        x0, n_log = self._features_hip(X, a)
        return _vae.hip_heads(self, run_chain(self.layers, x0, n_log))

    def sample(self, X, a, device=None, eps=None):
        return super().sample(X, a, device, eps)


class VAEDecoder(_Family, _spect.SpectGenerator):
    def __init__(self, d=64):
        super().__init__()
        self.embedding_dict = nn.ModuleDict({k: nn.Embedding(v, 256) for k, v in ATTRIBUTE_DIMS.items()})
        self.layers = _spect.deconv_stack(LATENT_DIM + 256 * len(ATTRIBUTE_DIMS), [8, 4, 2, 1, None], d)


class VAE(_vae.VAEBase):
    def __init__(self, device='cpu', d=64):
        super().__init__()
        self.encoder = VAEEncoder(d).to(device)
        self.decoder = VAEDecoder(d).to(device)

    def forward(self, x, c, num_samples=4):
        return self.elbo(x, c, num_samples=num_samples)


def train(path_to_zip: str,
          n_epochs=200,
          l_rate=1e-4,
          device='cpu',
          save_images_every=2,
          batch_size=128,
          image_output_path='',
          num_samples_per_step=4,
          kl_weight=10):
    """Reference signature (:323-331).  ``path_to_zip`` may be a data source with the ``AudioMNISTData`` interface
    (``image_scms._spect.WaveformData``); the plots and wav dumps (:388-451) stay with the reference."""
    vae = VAE(device=device)
    vae.encoder.apply(init_weights)
    vae.decoder.apply(init_weights)
    data = path_to_zip if _spect.is_data_source(path_to_zip) else AudioMNISTData(path_to_zip, device=device)
    attr_cols = [k for k in data.data if k in ATTRIBUTE_DIMS]
    return _vae.run_training(vae, data, dict(batch_size=batch_size, excluded_runs=VALIDATION_RUNS), attr_cols,
                             n_epochs, l_rate, device, torch.float32, num_samples_per_step, kl_weight)
