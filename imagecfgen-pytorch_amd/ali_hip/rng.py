"""The counter RNG of the HIP path on the host: the key schedule of csrc/ali_rng.h (the table there is the statement)
and the references that reproduce a run's draws from (seed, counter, index) -- Dropout2d masks, latents, the WGAN-GP
``eps``, Gumbel noise, Griffin-Lim phases, the tiebreak of the thinning order and the background rows and mixing weights
of the expected-gradients estimator, and the skeleton locations of the Morpho-MNIST local perturbations.  The integers
are exact on both sides."""
import numpy as np
import torch

DEFAULT_Z_SEED, COUNTER_MUL = 0x5EED, 0xD1B54A32D192ED03
LATENT_STREAM, GP_STREAM = 0x4C4154454E545A31, 0x47504D4958455053
GUMBEL_STREAM, PHASE_STREAM = 0x47554D42454C3031, 0x474C504841534531
THIN_STREAM = 0x5448494E4B455931
EG_STREAM = 0x4547425249445831
LOCATE_STREAM = 0x534B454C4C4F4331                                   # "SKELLOC1"
MAX_DRAWS = 8                    # locations one image draws per call (ali_morpho_locate)
STREAMS = {"mask": (), "latent": (LATENT_STREAM,), "gp": (LATENT_STREAM, GP_STREAM),       # the tags mixed into the
           "gumbel": (LATENT_STREAM, GUMBEL_STREAM), "phase": (PHASE_STREAM,),               # base key, in order
           "thin": (THIN_STREAM,), "eg": (EG_STREAM,), "locate": (LOCATE_STREAM,)}
M64, TWO24 = (1 << 64) - 1, 16777216.0


def mix64(z):
    """splitmix64's finaliser on a uint64 array, or on an int (reduced to 64 bits)"""
    if not isinstance(z, np.ndarray):
        return int(mix64(np.array([int(z) & M64], dtype=np.uint64))[0])
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def key(seed, counter, stream):
    """the key of ``stream`` (a name of STREAMS) under (seed, counter); ``counter`` None is 0"""
    k = mix64(mix64(seed) ^ (int(counter or 0) * COUNTER_MUL & M64))
    for tag in STREAMS[stream]:
        k = mix64(k ^ tag)
    return k


def hashes(key, n, offset=0, shift=0):
    """the hashes [n] (uint64) of ``(offset + i) >> shift``, i < n, under ``key``; the sum wraps like the device's"""
    e = np.arange(n, dtype=np.uint64) + np.uint64(int(offset) & M64)
    return mix64(np.uint64(key) ^ (e >> np.uint64(shift)))


def hi24(r):
    return (r >> np.uint64(40)).astype(np.int64)


def lo24(r):
    return ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.int64)


def rank_seed(z_seed, rank):
    """the seed data-parallel rank ``rank`` draws its latents with (rank 0: ``z_seed`` itself)"""
    z_seed = int(z_seed) & M64
    return z_seed if rank == 0 else mix64(z_seed ^ (rank * COUNTER_MUL & M64))


def mask_reference(seed, counter, B, C, p, offset=0):
    """exact host evaluation of ``ali_dropout_mask(seed, offset, &counter, p, out, B*C)``: a float32 CPU tensor [B, C],
    fp32 throughout -- 1 / (1 - p) where hi24 * 2^-24 < 1 - p, else 0"""
    one, p = np.float32(1), np.float32(p)
    u = hi24(hashes(key(seed, counter, "mask"), B * C, offset)).astype(np.float32) * np.float32(1 / TWO24)
    return torch.from_numpy(np.where(u < one - p, one / (one - p), np.float32(0)).reshape(B, C))


def latent_bits(seed, counter, n, offset=0):
    """The integers behind elements ``offset .. offset + n`` of the latent stream keyed by (seed, counter):
    (k1 in [1, 2^24], k2 in [0, 2^24), odd) -- element g = offset + i is
    ``sqrt(-2 ln(k1 / 2^24)) * (sin if odd else cos)(2 pi k2 / 2^24)``, k1 / k2 being hi24 / lo24 of hash ``g >> 1``."""
    r = hashes(key(seed, counter, "latent"), n, offset, shift=1)
    return hi24(r) + 1, lo24(r), (np.arange(n) + (int(offset) & 1)) % 2 == 1


def normal_reference(seed, counter, n, offset=0):
    """fp64 host evaluation of ``ali_normal_fill(seed, &counter, offset, out, n)``: a float64 CPU tensor [n].  The
    integers are exact on both sides; the device differs by the rounding of its fp32 log / sqrt / sin / cos only."""
    k1, k2, odd = latent_bits(seed, counter, n, offset)
    rad = np.sqrt(-2.0 * np.log(k1 / TWO24))
    ang = (2.0 * np.pi) * (k2 / TWO24)
    return torch.from_numpy(rad * np.where(odd, np.sin(ang), np.cos(ang)))


def uniform_reference(seed, counter, n, offset=0):
    """host evaluation of the per-image ``eps`` that ``ali_gp_mix(eps=NULL, seed, &counter, offset, B=n, ...)`` draws: a
    float32 CPU tensor [n], exact (hi24 / 2^24 of hash ``offset + b`` under the "gp" key)."""
    k = hi24(hashes(key(seed, counter, "gp"), n, offset))
    return torch.from_numpy((k / TWO24).astype(np.float32))


def gumbel_reference(seed, counter, n, offset=0):
    """fp64 host evaluation of the Gumbel(0, 1) draws of ``ali_gumbel_posterior(g=NULL, seed, &counter, offset, ...)``:
    a float64 CPU tensor [n], element e = offset + row * C + class.  g = -log(-log u) with u = (k + 0.5) / 2^24
    strictly inside (0, 1), k = hi24 of hash e under the "gumbel" key.  The device evaluates the logarithms in fp64 too
    and rounds g to fp32 once: ``gumbel_reference(...).float()`` is what it stores, up to the last bit of its log."""
    k = hi24(hashes(key(seed, counter, "gumbel"), n, offset)).astype(np.float64)
    return torch.from_numpy(-np.log(-np.log((k + 0.5) / TWO24)))


def phase_reference(seed, counter, n, offset=0):
    """Host recipe of the initial phases ``ali_gl_init`` draws (``griffinlim.uniform_reference``): a float32 CPU tensor
    [2, n], row 0 the real and row 1 the imaginary parts of elements ``offset .. offset + n`` (element e = (b*F + f)*T
    + t of a [B,F,T] batch): hi24 / lo24 of hash e under the "phase" key over 2^24, exact in fp32, in [0, 1)."""
    r = hashes(key(seed, counter, "phase"), n, offset)
    return torch.from_numpy((np.stack([hi24(r), lo24(r)]) / TWO24).astype(np.float32))


def thin_reference(seed, n):
    """The tiebreaks of ``ali_morpho_thin(seed)`` for the pixels of linear index 0 .. n of an image: an int64 array [n],
    hi24 of hash i under the "thin" key of ``seed`` (no counter).  The same for every image of a batch."""
    return hi24(hashes(key(seed, None, "thin"), n))


def eg_index_reference(seed, counter, n, n_background, offset=0):
    """The background rows ``ali_eg_input(idx=NULL, seed, &counter, offset, ...)`` draws for (explained row, sample)
    pairs ``offset .. offset + n`` (pair e = row * S + sample; the launcher's ``offset`` counts rows: pass ``offset *
    S``): an int64 array [n] in [0, n_background), ``(hi24 * n_background) >> 24`` of hash e under the "eg" key.  Exact."""
    return (hi24(hashes(key(seed, counter, "eg"), n, offset)) * int(n_background)) >> 24


def eg_t_reference(seed, counter, n, offset=0):
    """The mixing weights of the same pairs: a float32 CPU tensor [n] in [0, 1), lo24 / 2^24 of the same hash.  Exact."""
    return torch.from_numpy((lo24(hashes(key(seed, counter, "eg"), n, offset)) / TWO24).astype(np.float32))


def locate_reference(seed, counter, n_candidates, row, k):
    """Draw ``k`` (< MAX_DRAWS) of image ``row`` of ``ali_morpho_locate(seed, &counter, offset, ...)``: an index into the
    image's ``n_candidates`` skeleton candidates in row-major order, ``(hi24 * n_candidates) >> 24`` of hash
    ``row * MAX_DRAWS + k`` under the "locate" key.  ``row`` counts from the first image of the whole call (the
    launcher's ``offset`` plus the row of the launch).  Exact; draw k does not depend on how many are drawn."""
    if not 0 <= int(k) < MAX_DRAWS:
        raise ValueError(f"locate_reference: draw {k} outside 0 .. {MAX_DRAWS - 1}")
    h = hi24(hashes(key(seed, counter, "locate"), 1, int(row) * MAX_DRAWS + int(k)))
    return int((int(h[0]) * int(n_candidates)) >> 24)
