"""The host definition of the counter RNG (ali_hip/rng.py) against the streams recorded before the key schedule moved
into it (tests/rng_cases.py, tests/golden/rng_streams.npz), and the properties of the mask reference."""
import numpy as np
import torch

import rng_cases as rc
from ali_hip import rng


def test_mix64_is_splitmix64():
    assert rng.mix64(0) == 0xE220A8397B1DCDAF                 # splitmix64's first output from state 0
    assert int(rng.mix64(np.zeros(1, dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF


def test_host_streams_match_the_recorded_ones():
    golden = {k: v for k, v in rc.load().items() if k.startswith("host.")}
    now = rc.host_streams()
    assert golden and set(now) == set(golden)
    for k, v in golden.items():
        assert now[k].dtype == v.dtype and now[k].shape == v.shape and (now[k] == v).all(), k


def test_public_names_stay_where_they_were():
    from ali_hip import griffinlim, source
    for name in ("normal_reference", "latent_bits", "uniform_reference", "gumbel_reference", "rank_seed", "DEFAULT_Z_SEED"):
        assert getattr(source, name) is getattr(rng, name)
    assert griffinlim.uniform_reference is rng.phase_reference


def test_mask_reference():
    for p in rc.MASK_P:
        whole = rng.mask_reference(0x5EED, 3, 64, 12, p)
        inv = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))          # fp32 throughout
        assert whole.dtype == torch.float32 and whole.shape == (64, 12)
        assert ((whole == 0) | (whole == inv)).all() and (whole == 0).any() and (whole == inv).any()
        for k in (5, 36):                                      # a chunk drawn at offset k is the slice [k:] of the whole
            chunk = rng.mask_reference(0x5EED, 3, 1, 64 * 12 - k, p, offset=k)
            assert torch.equal(chunk.reshape(-1), whole.reshape(-1)[k:])
        assert torch.equal(rng.mask_reference(7, None, 64, 12, p), rng.mask_reference(7, 0, 64, 12, p))
        assert not torch.equal(rng.mask_reference(0x5EEE, 3, 64, 12, p), whole)
        assert not torch.equal(rng.mask_reference(0x5EED, 4, 64, 12, p), whole)
