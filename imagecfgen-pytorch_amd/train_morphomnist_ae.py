"""Class autoencoders of the MorphoMNIST counterfactual metrics -- drop-in for the reference's
``train_morphomnist_ae.py`` (Encoder :12-25, Decoder :28-43, arguments :46-58, loop :61-118): the module name, the class
names, constructor arguments, attribute names and ``state_dict`` keys (``conv1.*``, ``conv2.*``, ``fc.*``) are the
reference's, so checkpoints pickled there (``torch.save({'E': E, 'G': G})``, loaded by ``morphomnist_cf_metrics.py``
and ``mnist_oracle_scores.py``) resolve here.

CPU tensors run the plain torch statement.  CUDA tensors run on the HIP kernels: each ``forward`` is one autograd node
of ``ali_hip.chain`` over an ``nn.Sequential`` view of the same parameter objects (kept outside the module: a
checkpoint holds the three layers and nothing else), and ``train`` runs ``ali_hip.cfmetrics.AeStepper``."""
import os
import weakref
from argparse import ArgumentParser

import numpy as np
import torch
import torch.nn as nn

from image_scms.training_utils import batchify

_VIEWS = weakref.WeakKeyDictionary()     # module -> its nn.Sequential view (never part of the module's state)


def _view(mod, build):
    seq = _VIEWS.get(mod)
    if seq is None:
        seq = _VIEWS[mod] = build()
    seq.train(mod.training)
    return seq


class Encoder(nn.Module):
    """[B,1,28,28] -> [B,latent_dim]: two stride-2 4x4 convolutions with ReLU, then a Linear on the flattened 7x7 map"""

    def __init__(self, capacity=64, latent_dim=10):
        super().__init__()
        c = capacity
        self.conv1 = nn.Conv2d(1, c, 4, 2, 1)             # c x 14 x 14
        self.conv2 = nn.Conv2d(c, 2 * c, 4, 2, 1)         # 2c x 7 x 7
        self.fc = nn.Linear(2 * c * 7 * 7, latent_dim)

    def chain_view(self) -> nn.Sequential:
        return _view(self, lambda: nn.Sequential(self.conv1, nn.ReLU(), self.conv2, nn.ReLU(), nn.Flatten(), self.fc))

    def forward(self, X):
        if X.is_cuda:
            from ali_hip.cfmetrics import encode
            return encode(self, X)
        X = torch.relu(self.conv2(torch.relu(self.conv1(X))))
        return self.fc(X.view(X.size(0), -1))


class Decoder(nn.Module):
    """[B,latent_dim] -> [B,1,28,28] in [-1, 1]: a Linear onto a 2c x 7 x 7 map, a stride-2 4x4 transposed convolution
    with ReLU and one with tanh"""

    def __init__(self, capacity=64, latent_dim=10):
        super().__init__()
        self.c = capacity
        self.fc = nn.Linear(latent_dim, 2 * self.c * 7 * 7)
        self.conv2 = nn.ConvTranspose2d(2 * self.c, self.c, 4, 2, 1)
        self.conv1 = nn.ConvTranspose2d(self.c, 1, 4, 2, 1)

    def chain_view(self) -> nn.Sequential:
        return _view(self, lambda: nn.Sequential(self.fc, nn.Unflatten(1, (2 * self.c, 7, 7)), self.conv2, nn.ReLU(),
                                                 self.conv1, nn.Tanh()))

    def forward(self, X):
        if X.is_cuda:
            from ali_hip.cfmetrics import decode
            return decode(self, X)
        X = self.fc(X).view(X.size(0), 2 * self.c, 7, 7)
        return torch.tanh(self.conv1(torch.relu(self.conv2(X))))


def _load(data_dir, name, device):
    return torch.from_numpy(np.load(os.path.join(data_dir, name))).float().to(device)


def _scale(x):
    return 2 * x.reshape((-1, 1, 28, 28)) / 255.0 - 1


def train(data_dir, steps=200, cls=None, latent_dim=100, batch_size=64, learning_rate=1e-4, device=None):
    """The script's loop as a function: reads ``mnist-{a,x}-{train,test}.npy`` from ``data_dir``, keeps the images of
    digit ``cls`` (all when None), trains E and G for ``steps`` epochs on the mean squared reconstruction error with
    Adam(lr, betas (0.5, 0.9)) and prints the training and the test error after every epoch.  On a CUDA device the iteration is
    ``AeStepper``'s (HIP-graph replay, the loss stays on the device: one host read per epoch).  Returns (E, G)."""
    from ali_hip.cfmetrics import AeStepper
    device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    a_train, a_test = _load(data_dir, 'mnist-a-train.npy', device), _load(data_dir, 'mnist-a-test.npy', device)
    x_train, x_test = _load(data_dir, 'mnist-x-train.npy', device), _load(data_dir, 'mnist-x-test.npy', device)
    if cls is not None:
        x_train = x_train[a_train[:, :10].argmax(1) == cls]
        x_test = x_test[a_test[:, :10].argmax(1) == cls]
    print(f'{len(x_train)} training and {len(x_test)} test images')
    E = Encoder(latent_dim=latent_dim).to(device)
    G = Decoder(latent_dim=latent_dim).to(device)
    stepper = AeStepper(E, G, lr=learning_rate, betas=(0.5, 0.9), capture=device.type == "cuda")
    for epoch in range(steps):
        E.train()
        G.train()
        print(f'Epoch {epoch + 1}/{steps}')
        total, batches = torch.zeros((), device=device), 0
        for (x,) in batchify(x_train, batch_size=batch_size):
            total += stepper.step(_scale(x))["loss"]
            batches += 1
        with torch.no_grad():
            xt = _scale(x_test)
            test_loss = (G(E(xt)) - xt).square().mean().item()
        print(f'train mse {total.item() / max(batches, 1):.6g}, test mse {test_loss:.6g}')
    return E, G


parser = ArgumentParser()
parser.add_argument('--data-dir', type=str, default='',
                    help='directory that holds mnist-{a,x}-{train,test}.npy')
parser.add_argument('--steps', type=int, default=200, help='passes over the training images')
parser.add_argument('--cls', type=int, default=None)
parser.add_argument('--output-path', type=str, default='morphomnist_ae.tar')
parser.add_argument('--latent-dim', type=int, default=100)
parser.add_argument('--batch-size', type=int, default=64)
parser.add_argument('--learning-rate', type=float, default=1e-4)


if __name__ == '__main__':
    args = parser.parse_args()
    E, G = train(args.data_dir, steps=args.steps, cls=args.cls, latent_dim=args.latent_dim, batch_size=args.batch_size,
                 learning_rate=args.learning_rate)
    torch.save({'E': E, 'G': G}, args.output_path)
