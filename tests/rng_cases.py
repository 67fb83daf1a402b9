"""Shared by tests/test_rng_cpu.py and tests/test_gpu_rng_streams.py: the cases that pin the bits of the counter RNG
(csrc/ali_rng.h, ali_hip/rng.py) and the two functions that evaluate them, on the host references and through ``ops``.

``python tests/rng_cases.py --record`` writes tests/golden/rng_streams.npz: the ``host.*`` entries always, the ``dev.*``
entries when a GPU is present (otherwise the ones already in the file are kept).  The committed file was recorded
before the key schedule moved into one header and one module, so it states what the streams were, not what the
current code happens to give.

The cases are the smallest that reach every branch of the key and index arithmetic: a NULL counter, a counter past
2^32 under an all-ones seed, an odd offset (``normal_fill`` starts on the sine half of a pair) and an offset that
carries into the high word of the 64-bit add."""
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rng_streams.npz")

KEYS = [(0, None), (0x5EED, 3), (2 ** 64 - 1, 2 ** 40 + 3)]
OFFSETS = [0, 5, 2 ** 32 + 5]
# (key index, offset index): every key at offset 0, every offset under the middle key
COMBOS = [(0, 0), (1, 0), (2, 0), (1, 1), (1, 2)]
MASK_SHAPES = [(5, 3), (64, 12)]
MASK_P = [0.2, 0.5]
MULTI_SEGS = [(5, 3, 4, 0.2), (2, 8, 8, 0.5), (3, 5, 8, 0.2)]        # (B, clog, cpad, p)
N_FILL = 37
GP_B, GP_P = 4, 8
GUMBEL_N, GUMBEL_C = 3, 5
GL_B, GL_F, GL_T = 1, 3, 5
VAE_S, VAE_B, VAE_L = 2, 2, 6


def combos():
    """(tag, seed, counter or None, offset) of every (key, offset) pair the streams are recorded at"""
    return [(f"k{ki}.o{oi}",) + KEYS[ki] + (OFFSETS[oi],) for ki, oi in COMBOS]


def multi_layout():
    """(seg_end, seg_p, seg_clog, seg_cpad) of MULTI_SEGS as ``ops.dropout_mask_multi`` takes them"""
    ends, n = [], 0
    for B, _, cpad, _ in MULTI_SEGS:
        n += B * cpad
        ends.append(n)
    return ends, [s[3] for s in MULTI_SEGS], [s[1] for s in MULTI_SEGS], [s[2] for s in MULTI_SEGS]


def host_streams():
    """{name: numpy array}: the host references of the four streams that have one, at every combo"""
    from ali_hip import griffinlim, source
    out = {}
    for tag, seed, counter, offset in combos():
        c = counter or 0
        k1, k2, odd = source.latent_bits(seed, c, N_FILL, offset)
        out[f"host.latent_k1.{tag}"], out[f"host.latent_k2.{tag}"], out[f"host.latent_odd.{tag}"] = k1, k2, odd
        out[f"host.gp.{tag}"] = source.uniform_reference(seed, c, GP_B, offset).numpy()
        out[f"host.gumbel.{tag}"] = source.gumbel_reference(seed, c, GUMBEL_N * GUMBEL_C, offset).numpy()
        out[f"host.phase.{tag}"] = griffinlim.uniform_reference(seed, c, GL_B * GL_F * GL_T, offset).numpy()
    return out


def device_streams():
    """{name: numpy array}: the draws of the seven launchers through ``ops`` on cuda:0, at every combo"""
    from ali_hip import ops
    dev = torch.device("cuda:0")
    new = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
    out = {}
    for tag, seed, counter, offset in combos():
        ctr = None if counter is None else torch.full((1,), counter, dtype=torch.int64, device=dev)
        for B, C in MASK_SHAPES:
            for p in MASK_P:
                out[f"dev.mask.{B}x{C}.p{p}.{tag}"] = ops.dropout_mask(seed, offset, p, B, C, dev, dev_counter=ctr)
        if offset == 0:                                        # (the multi launcher takes no offset)
            ends, ps, clog, cpad = multi_layout()
            out[f"dev.mask_multi.{tag}"] = ops.dropout_mask_multi(seed, ctr, ends, ps, clog, cpad, new(ends[-1]))
        buf = new(N_FILL + 3)
        assert buf.data_ptr() % 16 == 0
        out[f"dev.normal.{tag}"] = ops.normal_fill(seed, buf[1:1 + N_FILL], ctr, offset)
        out[f"dev.gp.{tag}"] = ops.gp_mix(new(GP_B, GP_P), new(GP_B, GP_P), None, seed, ctr, offset)[1]
        y = torch.zeros(GUMBEL_N, dtype=torch.int64, device=dev)
        out[f"dev.gumbel.{tag}"] = ops.gumbel_posterior(new(GUMBEL_N, GUMBEL_C), y, None, seed, ctr, offset,
                                                        want_g=True)[1]
        mag, X = new(GL_B * GL_T, GL_F), new(GL_B * GL_T, 2 * GL_F)
        ops.gl_init(new(GL_B, GL_F, GL_T), ops.GL_SRC_LOG, mag, X, seed=seed, dev_counter=ctr, offset=offset)
        assert (mag == 1).all()                                # exp(0): X holds the phases themselves
        out[f"dev.phase.{tag}"] = X
        out[f"dev.vae_eps.{tag}"] = ops.vae_latent_fwd(new(VAE_B, VAE_L), new(VAE_B, VAE_L), VAE_S,
                                                       new(VAE_S * VAE_B, VAE_L), seed=seed, dev_counter=ctr,
                                                       offset=offset, want_eps=True, want_kl=False)[1]
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def load():
    """the recorded streams: {name: numpy array}"""
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def record():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "imagecfgen-pytorch_amd"))
    entries = host_streams()
    if torch.cuda.is_available():
        entries.update(device_streams())
    elif os.path.exists(GOLDEN):
        entries.update({k: v for k, v in load().items() if k.startswith("dev.")})
    np.savez_compressed(GOLDEN, **entries)
    print(f"wrote {GOLDEN}: {sum(k.startswith('host.') for k in entries)} host and "
          f"{sum(k.startswith('dev.') for k in entries)} device entries")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/rng_cases.py --record")
    record()
