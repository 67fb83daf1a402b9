"""AudioMNIST attribute classifiers -- drop-in for the reference's ``classifiers/audio_mnist.py``
(VALIDATION_RUNS :18, AudioMNISTClassifier :21-42, ATTRIBUTE_DIMS :180-187, evaluate :190-238, train :241-307).
The zip / wav reader (``AudioMNISTData``, :45-177) is the step before the hot path and is not re-implemented:
``train`` / ``evaluate`` take a data source with its interface (``image_scms._spect.WaveformData``) where the reference
takes the zip path, as ``image_scms.audio_mnist.train`` does."""
import numpy as np
import torch
import torch.nn as nn

from image_scms import _spect

from . import _stack
from .training_utils import batchify  # noqa: F401  (re-exported like the reference)

np.random.seed(42)   # the reference seeds numpy at import time (:17)
VALIDATION_RUNS = [38, 7, 42, 10, 14, 18, 20, 22, 28]
IMAGE_SHAPE = (128, 128)

AudioMNISTData = _spect.data_adapter_unavailable("AudioMNISTData", "torchaudio, librosa")


class AudioMNISTClassifier(_stack.ClassifierStack):
    def __init__(self, num_classes: int = 10):
        super().__init__(*_stack.conv_layers([32, 64, 128, 256, 512, 1024, 1024], [1, 2, 1, 2, 2, 2, 2]),
                         nn.Flatten(),
                         nn.Linear(4096, 1024),
                         nn.LeakyReLU(0.2),
                         nn.Linear(1024, num_classes))


ATTRIBUTE_DIMS = {
    "country_of_origin": 13,
    "native_speaker": 2,
    "accent": 15,
    "digit": 10,
    "age": 5,
    "gender": 2
}

_TRAIN_RUNS_EXCLUDED = VALIDATION_RUNS
_VALID_RUNS_EXCLUDED = sorted(set(range(50)) - set(VALIDATION_RUNS))


def _source(zip_path, device):
    return zip_path if _spect.is_data_source(zip_path) else AudioMNISTData(zip_path, device=device)


def _label_of(attribute, device):
    def label_of(batch):
        if attribute == "subject":          # subjects are numbered from 1 (:281)
            return torch.eye(60, device=device)[batch[attribute].flatten().long() - 1].reshape((-1, 60))
        return batch[attribute]
    return label_of


def evaluate(zip_path,
             model_path: str,
             attribute: str = "digit",
             stats_prefix: str = None,
             batch_size: int = 128):
    """Validation-run accuracy of a saved classifier (:190-238).  ``zip_path``: the AudioMNIST zip (needs the
    reference's reader) or a data source; ``model_path``: a ``{"model": classifier}`` pickle, or the classifier."""
    device = "cuda" if torch.cuda.is_available() else "cpu"
    data = _source(zip_path, device)
    model = model_path if isinstance(model_path, nn.Module) else \
        torch.load(model_path, map_location=device, weights_only=False)['model']
    if stats_prefix is not None:
        mean = torch.from_numpy(np.load(stats_prefix + '_mean.npy')).float().to(device)
        std = torch.from_numpy(np.load(stats_prefix + '_std.npy')).float().to(device)
    else:
        mean, std, _ = _spect.spectrogram_statistics(
            lambda: data.stream(batch_size=batch_size, excluded_runs=_TRAIN_RUNS_EXCLUDED), device,
            clamp_variance=True)
    model.eval()
    return _stack.accuracy_on_stream(model, data.stream(batch_size=batch_size, excluded_runs=_VALID_RUNS_EXCLUDED),
                                     _label_of(attribute, device), _stack.spect_to_img_fn(mean, std), IMAGE_SHAPE,
                                     device)


def train(zip_path,
          epochs: int = 100,
          batch_size: int = 100,
          attribute: str = "digit"):
    """Reference signature and loop (:241-307); ``zip_path`` may be a data source (see the module docstring)."""
    device = "cuda" if torch.cuda.is_available() else "cpu"
    data = _source(zip_path, device)
    model = AudioMNISTClassifier(60 if attribute == "subject" else ATTRIBUTE_DIMS[attribute]).to(device)
    return _stack.train_on_source(model, data, _label_of(attribute, device), IMAGE_SHAPE,
                                  dict(batch_size=batch_size, excluded_runs=_TRAIN_RUNS_EXCLUDED),
                                  dict(batch_size=batch_size, excluded_runs=_VALID_RUNS_EXCLUDED), epochs, 1e-4, device)
