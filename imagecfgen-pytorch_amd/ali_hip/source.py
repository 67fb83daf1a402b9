"""Device-side input pipeline of the training loops (opt-in: ``mnist.train(input_pipeline="device")``,
``train_on_stream(z_source="device")``).

``DeviceDataset``   the images, attributes and attribute statistics of a MorphoMNIST-style data set, uploaded once;
                    an epoch is one uploaded permutation, a batch one slice of it, and ``AliStepper.step_indexed``
                    assembles the batch on the device (``ali_batch_gather``) inside its captured iteration.
``normal_reference``  the latent generator ``ali_normal_fill`` implements, in fp64 on the host; it and the other host
                    references of the device's draws live in ``ali_hip.rng`` and are re-exported here.
"""
import numpy as np
import torch

from . import ops
from .rng import (DEFAULT_Z_SEED, gumbel_reference, latent_bits, normal_reference, rank_seed,  # noqa: F401
                  uniform_reference)


class DeviceDataset:
    """A MorphoMNIST-style data set resident in device memory, for ``AliStepper.step_indexed``.

    ``images`` [N, H, W] (uint8 stays uint8: a quarter of the bytes; anything else becomes fp32), ``attrs`` the
    attribute dict of ``image_scms.mnist.train``: ``class_key`` holds one-hot rows, every other key one fp32 value per
    sample.  The continuous keys are fixed in sorted order (the order ``MnistFamily.conditioning`` uses) and stored
    behind the one-hot columns of one [N, n_cls + n_cont] matrix; ``attr_stats`` {key: (lo, hi)} defaults to the
    per-key minimum / maximum, like the training loop's."""

    def __init__(self, images, attrs, device, batch_size=64, class_key="digit", attr_stats=None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"DeviceDataset needs a CUDA device, got {device!r}")
        N = len(images)
        self.hw = tuple(int(v) for v in images.shape[-2:])
        self.keys = sorted(k for k in attrs if k != class_key)
        for k in self.keys:
            if attrs[k].dtype != torch.float32 or attrs[k].numel() != N:
                raise ValueError(f"attribute {k!r}: need one fp32 value per sample, got {attrs[k].dtype} "
                                 f"{tuple(attrs[k].shape)}")
        if attr_stats is None:
            attr_stats = {k: (attrs[k].min(dim=0).values, attrs[k].max(dim=0).values) for k in self.keys}
        self.attr_stats = {k: attr_stats[k] for k in self.keys}
        onehot = attrs[class_key].reshape(N, -1).float()
        self.n_cls = onehot.shape[1]
        self.images = (images if images.dtype == torch.uint8 else images.float()).reshape(N, -1).contiguous().to(dev)
        self.attrs = torch.cat([onehot.cpu()] + [attrs[k].reshape(N, 1).cpu() for k in self.keys], dim=1).contiguous().to(dev)
        stat = lambda j: torch.stack([torch.as_tensor(self.attr_stats[k][j], dtype=torch.float32).reshape(())  # noqa: E731
                                      for k in self.keys]).to(dev) if self.keys else None
        self.lo, self.hi = stat(0), stat(1)
        self.batch_size = int(batch_size)
        self.perm = None
        # what a captured graph bakes in: the buffers' addresses and the row / column geometry
        self.key = (self.images.data_ptr(), self.attrs.data_ptr(), N, self.images.shape[1], self.images.dtype,
                    self.n_cls, len(self.keys), None if self.lo is None else (self.lo.data_ptr(), self.hi.data_ptr()))

    def __len__(self):
        return self.images.shape[0]

    def set_epoch(self, perm):
        """upload the epoch's sample order (validated on the host: the gather kernel cannot raise)"""
        perm = np.asarray(perm.cpu() if torch.is_tensor(perm) else perm).astype(np.int64).reshape(-1)
        if perm.size == 0 or perm.min() < 0 or perm.max() >= len(self):
            raise ValueError("set_epoch: indices outside the data set")
        self.perm = torch.from_numpy(perm).to(self.images.device)
        return self

    @property
    def n_batches(self):
        return 0 if self.perm is None else -(-self.perm.numel() // self.batch_size)

    def batch(self, i):
        """the index slice of batch ``i`` of the epoch (the last one may be ragged)"""
        if self.perm is None or not 0 <= i < self.n_batches:
            raise IndexError(f"batch {i} of {self.n_batches}")
        return self.perm[i * self.batch_size:(i + 1) * self.batch_size]

    def gather(self, index):
        """(images [B,1,H,W], one-hot rows [B,n_cls], idx [B,1] int32, cont [B,n_cont] | None): one launch"""
        x, onehot, idx, cont = ops.batch_gather(self.images, self.attrs, self.n_cls, index, self.lo, self.hi)
        return x.view((index.numel(), 1) + self.hw), onehot, idx, cont
