"""``batchify`` / ``batchify_dict`` / ``init_weights`` of the reference's ``deepscm_vae/training_utils.py``
(init std 0.0001, not ``image_scms``' 0.01)."""
import torch

from image_scms.training_utils import batchify, batchify_dict  # noqa: F401


def init_weights(layer):
    if layer.__class__.__name__.startswith('Conv'):
        torch.nn.init.normal_(layer.weight, mean=0, std=0.0001)
        if layer.bias is not None:
            torch.nn.init.constant_(layer.bias, 0)
