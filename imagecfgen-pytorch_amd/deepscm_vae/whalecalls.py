"""Right-whale call conditional VAE -- drop-in for the reference's ``deepscm_vae/whalecalls.py`` (constants :19-25,
init_weights :28-33, VAEEncoder :235-281, VAEDecoder :284-328, WhaleCallVAE :342-370, train :373-511).  256x256
log-spectrograms, one categorical attribute (``call_type``); the decoder keeps the reference's unused
``digit_embedding`` (a ``state_dict`` key).  The reference's likelihood here is a ``Normal`` summed over pixels -- the
same closed form.  The wav / .mat reader (``WhaleCallData``, :43-232) is not re-implemented: ``train`` takes a data
source as its first argument where the reference takes the three directories."""
import torch
import torch.nn as nn

from image_scms import _spect
from image_scms._spect import init_weights  # noqa: F401  (std=0.001, reference :28)

from . import _vae
from .training_utils import batchify, batchify_dict  # noqa: F401  (imported like the reference)

ATTRIBUTE_DIMS = {
    "call_type": 3,
    "path": 1,
    "time": 2
}
IMAGE_SHAPE = (256, 256)
LATENT_DIM = 512
_KEYS = tuple(k for k in sorted(ATTRIBUTE_DIMS.keys()) if k not in ("time", "path"))

WhaleCallData = _spect.data_adapter_unavailable("WhaleCallData", "torchaudio, scipy")


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
        self.embedding_dict = nn.ModuleDict({k: _spect.plane_embedding(ATTRIBUTE_DIMS[k], 16) for k in _KEYS})
        self.layers = _spect.conv_stack(2, [1, 2, 4, 8, 16, 16, None], d)
        self.mean_linear = nn.Conv2d(LATENT_DIM, LATENT_DIM, (1, 1))
        self.log_var_linear = nn.Conv2d(LATENT_DIM, LATENT_DIM, (1, 1))

    mean_head = property(lambda self: self.mean_linear)
    log_var_head = property(lambda self: self.log_var_linear)

    def forward(self, X: torch.Tensor, a):
        if not X.is_cuda:
            upstream = self.layers(self._features_torch(X, a))
            return self.mean_linear(upstream), self.log_var_linear(upstream)
        from ali_hip.chain import run_chain
        x0, n_log = self._features_hip(X, a)
        return _vae.hip_heads(self, run_chain(self.layers, x0, n_log))


class VAEDecoder(_Family, _spect.SpectGenerator):
    def __init__(self, d=64):
        super().__init__()
        self.digit_embedding = nn.Embedding(10, 256)          # unused, as in the reference (:287)
        self.embedding_dict = nn.ModuleDict({k: nn.Embedding(ATTRIBUTE_DIMS[k], 256) for k in _KEYS})
        self.layers = _spect.deconv_stack(LATENT_DIM + 256, [16, 8, 4, 2, 1, None], d)


class WhaleCallVAE(_vae.VAEBase):
    def __init__(self, device='cpu', d=64):
        super().__init__()
        self.encoder = VAEEncoder(d).to(device)
        self.decoder = VAEDecoder(d).to(device)

    def forward(self, x: torch.Tensor, c, num_samples=10):
        return self.elbo(x, c, num_samples=num_samples)


def train(nocall_directory,
          gunshot_directory=None,
          upcall_directory=None,
          n_epochs=200,
          l_rate=1e-4,
          device='cpu',
          save_images_every=2,
          batch_size=32,
          image_output_path='',
          filter_length=None,
          num_samples_per_step=4,
          kl_weight=10):
    """Reference signature (:373-384).  ``nocall_directory`` may be a data source with the ``WhaleCallData`` interface.
    The reference's Adam carries ``weight_decay=0.01`` (:388-390), which the flat Adam kernel does not implement: the
    loop runs the autograd ``elbo`` on the HIP kernels under ``torch.optim.Adam``."""
    vae = WhaleCallVAE(device=device)
    vae.encoder.apply(init_weights)
    vae.decoder.apply(init_weights)
    if _spect.is_data_source(nocall_directory):
        data = nocall_directory
    else:
        data = WhaleCallData(nocall_directory, gunshot_directory, upcall_directory, device=device,
                             filter_length=filter_length)
    return _vae.run_training(vae, data, dict(batch_size=batch_size), list(_KEYS), n_epochs, l_rate, device, torch.int32,
                             num_samples_per_step, kl_weight, weight_decay=0.01)
