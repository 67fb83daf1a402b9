"""North Atlantic right whale call classifier -- drop-in for the reference's ``classifiers/whalecalls.py``
(constants :14-20, init_weights :23-28, NARWClassifier :230-253, train :256-319).  The wav / .mat readers
(``WhaleCallData``, :38-227) are the step before the hot path and are not re-implemented: ``train`` takes a data source
with that interface (``image_scms._spect.WaveformData``) in place of the three directories."""
import torch
import torch.nn as nn

from image_scms import _spect

from . import _stack
from .training_utils import batchify  # noqa: F401  (re-exported like the reference)

ATTRIBUTE_DIMS = {
    "call_type": 3,
    "path": 1,
    "time": 2
}
IMAGE_SHAPE = (256, 256)
LATENT_DIM = 512

WhaleCallData = _spect.data_adapter_unavailable("WhaleCallData", "torchaudio, scipy")


def init_weights(layer, std=0.001):
    if layer.__class__.__name__.startswith('Conv'):
        torch.nn.init.normal_(layer.weight, mean=0, std=std)
        if layer.bias is not None:
            torch.nn.init.constant_(layer.bias, 0)


class NARWClassifier(_stack.ClassifierStack):
    def __init__(self, num_classes: int = 3):
        super().__init__(*_stack.conv_layers([32, 64, 128, 256, 512, 1024, 1024, 1024], [1, 2, 1, 2, 2, 2, 2, 2]),
                         nn.Flatten(),
                         nn.Linear(4096, 1024),
                         nn.LeakyReLU(0.2),
                         nn.Linear(1024, num_classes))


def train(nocall_directory,
          gunshot_directory=None,
          upcall_directory=None,
          n_epochs=200,
          l_rate=1e-4,
          device='cpu',
          batch_size=32,
          filter_length=None):
    """Reference signature and loop (:256-319).  ``nocall_directory`` may be a data source (then the other two
    directories are not used); the labels are the ``call_type`` one-hot rows, which for one-hot rows is the
    class-index CrossEntropyLoss of :300."""
    if _spect.is_data_source(nocall_directory):
        data = nocall_directory
    else:
        data = WhaleCallData(nocall_directory, gunshot_directory, upcall_directory, device=device,
                             filter_length=filter_length)
    clf = NARWClassifier().to(device)
    kw = dict(batch_size=batch_size)
    return _stack.train_on_source(clf, data, lambda b: b["call_type"], IMAGE_SHAPE, kw, kw, n_epochs, l_rate, device)
