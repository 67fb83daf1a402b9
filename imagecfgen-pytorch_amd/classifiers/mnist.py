"""MorphoMNIST digit classifier -- drop-in for the reference's ``classifiers/mnist.py`` (MNISTClassifier :11-24,
train :27-68): same class name, layer order and ``state_dict`` keys, so a reference checkpoint
(``torch.load(path)["model"]`` / ``["clf"]``) resolves to this class.  CUDA batches run on the HIP kernels."""
import os

import numpy as np
import torch
import torch.nn as nn

from . import _stack
from .training_utils import batchify


class MNISTClassifier(_stack.ClassifierStack):
    def __init__(self):
        super().__init__(*_stack.conv_layers([32, 64, 128, 256], [1, 2, 1, 2]),
                         nn.Flatten(),
                         nn.Linear(4096, 10))


def _load(data_dir, name, device):
    return torch.from_numpy(np.load(os.path.join(data_dir, name))).float().to(device)


def train(data_dir: str,
          epochs: int = 100,
          batch_size: int = 128):
    """Reference signature and loop (:27-68): the four ``mnist-{x,a}-{train,test}.npy`` files, images scaled to
    [-1, 1], Adam(1e-4) on CrossEntropyLoss against the one-hot digit columns, test accuracy per epoch.  On a CUDA
    device the step is ``ali_hip.classify.ClassifierStepper`` (one HIP graph per batch shape) and the test accuracy
    ``ClassifierScorer``; loss and accuracy are read once per epoch instead of once per batch."""
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    x_train = _load(data_dir, 'mnist-x-train.npy', device).reshape((-1, 1, 28, 28)) / 255.0
    a_train = _load(data_dir, 'mnist-a-train.npy', device)[:, :10]
    x_test = _load(data_dir, 'mnist-x-test.npy', device).reshape((-1, 1, 28, 28)) / 255.0
    a_test = _load(data_dir, 'mnist-a-test.npy', device)[:, :10]

    model = MNISTClassifier().to(device)
    stepper = _stack.make_stepper(model, 1e-4)
    from ali_hip.classify import ClassifierScorer
    scorer = ClassifierScorer({"digit": model}, capture=device.type == "cuda")
    for e in range(epochs):
        loss = hits = n = 0
        for x, y in _stack.progress(list(batchify(x_train, a_train, batch_size=batch_size))):
            r = stepper.step(2 * x - 1, y)
            loss, hits, n = loss + r["loss"], hits + r["hits"], n + 1
        print(f"loss = {float(loss) / max(n, 1):.4f} acc = {float(hits) / max(len(x_train), 1):.4f}")
        scorer.reset()
        for x, y in batchify(x_test, a_test, batch_size=batch_size):
            scorer.add(2 * x - 1, {"digit": y})
        print(torch.tensor(scorer.result()["digit"]))
    return model
