"""Device-side input pipeline of the training loops (opt-in: ``mnist.train(input_pipeline="device")``,
``train_on_stream(z_source="device")``).

``DeviceDataset``   the images, attributes and attribute statistics of a MorphoMNIST-style data set, uploaded once;
                    an epoch is one uploaded permutation, a batch one slice of it, and ``AliStepper.step_indexed``
                    assembles the batch on the device (``ali_batch_gather``) inside its captured iteration.
``normal_reference``  the definition of the latent generator ``ali_normal_fill`` implements, evaluated in fp64 on the
                    host: anyone who wants the latents of a run reproduces them from (z_seed, iteration, index).
"""
import numpy as np
import torch

from . import ops

DEFAULT_Z_SEED = 0x5EED
_LATENT_STREAM = 0x4C4154454E545A31          # csrc/elementwise.hip: kLatentStream
_COUNTER_MUL = 0xD1B54A32D192ED03
_M64 = (1 << 64) - 1


def _mix64(z):
    """splitmix64's finaliser (csrc/elementwise.hip: mix64) on a uint64 array"""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _mix64_int(z):
    return int(_mix64(np.array([z & _M64], dtype=np.uint64))[0])


def rank_seed(z_seed, rank):
    """the seed data-parallel rank ``rank`` draws its latents with (rank 0: ``z_seed`` itself)"""
    z_seed = int(z_seed) & _M64
    return z_seed if rank == 0 else _mix64_int(z_seed ^ (rank * _COUNTER_MUL & _M64))


def latent_bits(seed, counter, n, offset=0):
    """The integers behind elements ``offset .. offset + n`` of the latent stream keyed by (seed, counter):
    (k1 in [1, 2^24], k2 in [0, 2^24), odd) -- element g = offset + i is
    ``sqrt(-2 ln(k1 / 2^24)) * (sin if odd else cos)(2 pi k2 / 2^24)``, k1 / k2 being bits 40..63 / 16..39 of
    ``mix64(key ^ (g >> 1))``."""
    key = _mix64_int(_mix64_int(_mix64_int(int(seed)) ^ (int(counter) * _COUNTER_MUL & _M64)) ^ _LATENT_STREAM)
    g = np.arange(n, dtype=np.uint64) + np.uint64(int(offset) & _M64)
    r = _mix64(np.uint64(key) ^ (g >> np.uint64(1)))
    k1 = (r >> np.uint64(40)).astype(np.int64) + 1
    k2 = ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.int64)
    return k1, k2, (g & np.uint64(1)).astype(bool)


def normal_reference(seed, counter, n, offset=0):
    """fp64 host evaluation of ``ali_normal_fill(seed, &counter, offset, out, n)``: a float64 CPU tensor [n].  The
    integers are exact on both sides; the device differs by the rounding of its fp32 log / sqrt / sin / cos only."""
    k1, k2, odd = latent_bits(seed, counter, n, offset)
    rad = np.sqrt(-2.0 * np.log(k1 / 16777216.0))
    ang = (2.0 * np.pi) * (k2 / 16777216.0)
    return torch.from_numpy(rad * np.where(odd, np.sin(ang), np.cos(ang)))


_GP_STREAM = 0x47504D4958455053              # csrc/gan.hip: kGpStream


def uniform_reference(seed, counter, n, offset=0):
    """host evaluation of the per-image ``eps`` that ``ali_gp_mix(eps=NULL, seed, &counter, offset, B=n, ...)`` draws: a
    float32 CPU tensor [n], exact (k / 2^24, k the top 24 bits of ``mix64(key ^ g)`` under the latent key mixed once
    more with the stream's constant)."""
    key = _mix64_int(_mix64_int(_mix64_int(int(seed)) ^ (int(counter) * _COUNTER_MUL & _M64)) ^ _LATENT_STREAM)
    key = _mix64_int(key ^ _GP_STREAM)
    g = np.arange(n, dtype=np.uint64) + np.uint64(int(offset) & _M64)
    k = (_mix64(np.uint64(key) ^ g) >> np.uint64(40)).astype(np.int64)
    return torch.from_numpy((k / 16777216.0).astype(np.float32))


_GUMBEL_STREAM = 0x47554D42454C3031           # csrc/flow.hip: kGumbelStream


def gumbel_reference(seed, counter, n, offset=0):
    """fp64 host evaluation of the Gumbel(0, 1) draws of ``ali_gumbel_posterior(g=NULL, seed, &counter, offset, ...)``:
    a float64 CPU tensor [n], element e = offset + row * C + class.  g = -log(-log u) with u = (k + 0.5) / 2^24
    strictly inside (0, 1), k the top 24 bits of ``mix64(key ^ e)`` under the latent key mixed once more with the
    stream's constant.  k is exact on both sides; the device evaluates the logarithms in fp64 too and rounds g to fp32
    once, so ``gumbel_reference(...).float()`` is what it stores, up to the last bit of the device's log."""
    key = _mix64_int(_mix64_int(_mix64_int(int(seed)) ^ (int(counter) * _COUNTER_MUL & _M64)) ^ _LATENT_STREAM)
    key = _mix64_int(key ^ _GUMBEL_STREAM)
    e = np.arange(n, dtype=np.uint64) + np.uint64(int(offset) & _M64)
    k = (_mix64(np.uint64(key) ^ e) >> np.uint64(40)).astype(np.float64)
    return torch.from_numpy(-np.log(-np.log((k + 0.5) / 16777216.0)))


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
