"""Device-side input pipeline, the parts that need no GPU: the host definition of the latent generator
(``ali_hip.source.normal_reference``, which ``ali_normal_fill`` implements) passes fixed-seed statistical tests, is
consistent under offsets, and the public entry points keep the reference's positional order and refuse the device
pipeline on a CPU device."""
import inspect
import math

import numpy as np
import pytest
import torch

import ali_oracle as orc

N = 1 << 20
SEEDS = (0x5EED, 1, 2, 12345)
COUNTERS = (0, 1, 7)


def _ks_sqrt_n(x):
    """Kolmogorov-Smirnov D * sqrt(n) of a float64 sample against the standard normal CDF"""
    xs = np.sort(x)
    F = torch.special.ndtr(torch.from_numpy(xs)).numpy()
    n = len(xs)
    i = np.arange(1, n + 1)
    return max((i / n - F).max(), (F - (i - 1) / n).max()) * math.sqrt(n)


@pytest.mark.parametrize("seed", SEEDS)
def test_normal_reference_statistics(seed):
    """4-sigma / alpha ~ 1e-3 bounds for a fixed-seed test: |mean| sqrt(n) < 4, |var - 1| sqrt(n/2) < 4 (the variance of
    a sample variance of normals is 2/n), KS D sqrt(n) < 1.95, and the correlation between the draws of two
    consecutive counters, times sqrt(n), < 4."""
    from ali_hip.source import normal_reference
    draws = {}
    for counter in COUNTERS:
        x = normal_reference(seed, counter, N)
        assert x.dtype == torch.float64 and x.shape == (N,) and bool(torch.isfinite(x).all())
        x = draws[counter] = x.numpy()
        m, v, ks = abs(x.mean()) * math.sqrt(N), abs(x.var() - 1.0) * math.sqrt(N / 2), _ks_sqrt_n(x)
        print(f"seed {seed:#x} counter {counter}: mean {m:.2f} var {v:.2f} ks {ks:.2f}")
        assert m < 4, (seed, counter, m)
        assert v < 4, (seed, counter, v)
        assert ks < 1.95, (seed, counter, ks)
    corr = abs(np.corrcoef(draws[0], draws[1])[0, 1]) * math.sqrt(N)
    print(f"seed {seed:#x}: corr(counter 0, counter 1) * sqrt(n) = {corr:.2f}")
    assert corr < 4, (seed, corr)


def test_normal_reference_streams_differ_by_seed_and_counter():
    from ali_hip.source import normal_reference
    a = normal_reference(1, 0, 4096)
    assert not torch.equal(a, normal_reference(2, 0, 4096))
    assert not torch.equal(a, normal_reference(1, 1, 4096))
    assert torch.equal(a, normal_reference(1, 0, 4096))


@pytest.mark.parametrize("k", [1, 2, 333, 4096])
def test_normal_reference_offset_consistency(k):
    """element g of a stream does not depend on where the call started"""
    from ali_hip.source import normal_reference
    n = 5001
    whole = normal_reference(0x5EED, 3, n)
    assert torch.equal(whole[k:], normal_reference(0x5EED, 3, n - k, offset=k))


def test_rank_seed_keeps_rank_zero_and_separates_ranks():
    from ali_hip.source import rank_seed
    assert rank_seed(77, 0) == 77
    assert len({rank_seed(77, r) for r in range(8)}) == 8


def test_device_pipeline_on_cpu_raises():
    import image_scms.mnist as pm
    x, a = orc.synth_morphomnist(8, seed=2)
    with pytest.raises(ValueError):
        pm.train(x, a, n_epochs=1, device="cpu", save_images_every=None, batch_size=4, input_pipeline="device")
    with pytest.raises(ValueError):
        pm.train(x, a, n_epochs=1, device="cpu", save_images_every=None, batch_size=4, input_pipeline="gpu")


def test_z_source_device_on_cpu_raises():
    from image_scms import _spect
    with pytest.raises(ValueError):
        _spect.train_on_stream(None, None, None, lambda: iter(()), device="cpu", z_source="device")


REFERENCE_PARAMETERS = {
    "mnist": ["x_train", "a_train", "x_test", "a_test", "n_epochs", "l_rate", "device", "save_images_every",
              "image_output_path", "batch_size", "d_updates_per_g_update"],
    "audio_mnist": ["path_to_zip", "n_epochs", "l_rate", "device", "save_images_every", "batch_size",
                    "image_output_path"],
    "whalecalls": ["nocall_directory", "gunshot_directory", "upcall_directory", "n_epochs", "l_rate", "device",
                   "save_images_every", "batch_size", "image_output_path", "filter_length"],
    "esrf_acoustic": ["path_to_wavs", "path_to_labels", "n_epochs", "l_rate", "device", "save_images_every",
                      "batch_size", "image_output_path", "validation_split", "start_model_path"],
}


@pytest.mark.parametrize("modname", sorted(REFERENCE_PARAMETERS))
def test_train_signatures_keep_the_reference_order(modname):
    """the reference's parameters come first, in its order; the pipeline keywords are appended and default to the
    host behaviour"""
    import importlib
    train = importlib.import_module(f"image_scms.{modname}").train
    params = inspect.signature(train).parameters
    names = list(params)
    ref = REFERENCE_PARAMETERS[modname]
    assert names[:len(ref)] == ref
    key = "input_pipeline" if modname == "mnist" else "z_source"
    assert names.index(key) >= len(ref) and params[key].default == "host"
    assert names.index("z_seed") >= len(ref) and params["z_seed"].default is None
