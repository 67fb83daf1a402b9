"""The two kernels of the Morpho-MNIST local perturbations (csrc/morpho.hip) on the device, against the statement
``morphomnist.perturb.local_continue_from``: ``ops.morpho_locate`` (candidate counts, fallback flags, centres, end points
and the draws of ``rng.locate_reference`` exactly; split row ranges with ``offset``) and ``ops.morpho_local`` (thin, thick,
fracture and default-strength swelling bitmaps, radii, pad bits and status rows exactly; a swelling through ``pow`` but
for the pixels whose source coordinate lies within 1e-6 of a pixel boundary, of which the chosen seed has none).

Built bitmaps: the skeletons of ``local_cases.skeletons`` (24 x 72: the word boundaries at x = 32 and 64) in bitmaps grown
around them.  Images: those of tests/test_gpu_morpho_kernels.py -- 5 x 9 at scales 1, 2, 4 and 28 x 28 at scale 4 with B in
{1, 3, 70}; 28 x 28 at scale 16 with B = 3 -- taken through the four measurement kernels, the statement continued from the
device's own bitmap, distance map, skeleton and fp32 thickness.  Every call is made twice and must give the same bits."""
import numpy as np
import pytest
import torch

import local_cases as lc
import morpho_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(H, W, s, B) for (H, W, s) in mc.SMALL for B in mc.BATCHES] + [(28, 28, 16, 3)]
KEYS = ("bits", "radius", "sums", "status", "n_candidates", "fallback", "centres", "endpoints")


def _mo():
    from ali_hip import morpho
    return morpho


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _twice(fn):
    a, b = fn(), fn()
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    return a


def _built(scale):
    """the built cases as one batch: numpy (binary, d2, d2c, skel, thickness) with the device tensors of the same"""
    cases = lc.skeletons()
    names = list(cases)
    skel = np.stack([cases[n] for n in names])
    parts = [lc.around(s) for s in skel]
    binary, d2, d2c = (np.stack([q[i] for q in parts]) for i in range(3))
    thick = np.array([q[3] for q in parts], dtype=np.float32) / np.float32(scale)
    mo = _mo()
    values = torch.zeros(len(names), 5, device=DEV)                  # a column of pitch 5, as ``morpho_measure`` leaves it
    values[:, 2] = _dev(thick, np.float32)
    dev = dict(bits=mo.pack_bits(binary).to(DEV), d2=_dev(d2, np.int32), d2c=_dev(d2c, np.int32),
               skel=mo.pack_bits(skel).to(DEV), thick=values[:, 2])
    return names, (binary, d2, skel, thick), dev


@pytest.mark.parametrize("scale", [1, 2, 4])
@pytest.mark.parametrize("kind", range(5))
def test_built_bitmaps(scale, kind):
    names, host, dev = _built(scale)
    B, (Hh, Wh) = len(names), host[0].shape[1:]
    status = np.zeros(B, dtype=np.int32)
    status[names.index("col")] = 2                                   # a status passes through unchanged
    kinds = np.full(B, kind, dtype=np.int32)
    ctr = torch.tensor([3], dtype=torch.int64, device=DEV)
    got = _twice(lambda: lc.device_local(dev["bits"], dev["d2"], dev["d2c"], dev["skel"], dev["thick"],
                                         _dev(status, np.int32), _dev(kinds, np.int32), scale, Wh, seed=7, counter=ctr))
    want = lc.statement_rows(*host, status, kinds, Hh // scale, Wh // scale, scale, seed=7, counter=3)
    lc.compare(f"built s={scale} kind={kind}", got, want, Wh)
    st = [w["status"] for w in want]
    assert st[names.index("col")] == 2 and st[names.index("none")] == 4          # nothing: an empty result
    if kind == 4:
        fell = [w["fallback"] for w in want]
        assert 1 in fell and 0 in fell, fell                         # (the 2 x 2 block is all forks)
        from ali_hip import rng
        from morphomnist.skeleton import candidates
        b = names.index("ring")                                      # no tips, no forks: drawn from the whole ring
        coords = np.argwhere(candidates(host[2][b], scale, 2., 2.))
        assert len(coords) == int(got["n_candidates"][b]) == int(host[2][b].sum())
        for k in range(3):
            at = coords[rng.locate_reference(7, 3, len(coords), b, k)]
            assert got["centres"][b, k].tolist() == at.tolist()


def test_locate_split_row_ranges_and_prune_radii():
    """rows 4 .. B of a call draw with ``offset`` 4 what the whole call draws; a None radius skips that erase"""
    from ali_hip import ops
    from morphomnist import skeleton as sk
    names, host, dev = _built(2)
    B = len(names)
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    kinds = torch.full((B,), 4, dtype=torch.int32, device=DEV)
    whole = ops.morpho_locate(dev["skel"], dev["d2"], st, kinds, 2, 4, 4, 8, seed=1)
    for lo, hi in ((0, 4), (4, B)):
        part = ops.morpho_locate(dev["skel"][lo:hi], dev["d2"][lo:hi], st[lo:hi], kinds[lo:hi], 2, 4, 4, 8, seed=1,
                                 offset=lo)
        for a, b in zip(whole, part):
            assert torch.equal(a[lo:hi], b)
    moved = ops.morpho_locate(dev["skel"], dev["d2"], st, kinds, 2, 4, 4, 8, seed=1, offset=1)
    assert not torch.equal(moved[2], whole[2])
    for tips, forks in ((None, 3), (3, None), (0, 0), (None, None), (2000, 1)):
        n_cand = ops.morpho_locate(dev["skel"], dev["d2"], st, kinds, 2, tips, forks, 1)[0].tolist()
        for b in range(B):
            cand = host[2][b]
            if tips is not None:
                cand = sk.erase(cand, sk.num_neighbours(cand) == 1, tips)
            if forks is not None:
                cand = sk.erase(cand, sk.num_neighbours(cand) == 3, forks)
            n = int(cand.sum())
            assert n_cand[b] == (n if n else int(host[2][b].sum())), (names[b], tips, forks)


def _measured(H, W, scale, B, seed):
    """the four measurement kernels on ``image_batch``: device tensors and their numpy twins"""
    from ali_hip import ops
    mo = _mo()
    x = torch.from_numpy(mc.image_batch(B, H, W, seed).astype(np.float32)).to(DEV)
    mm = mo.MorphoMeasure(scale=scale)
    AH, AW = mm.operators(H, W, x.device)
    bits, fg, hstats = ops.morpho_binarise(x, scale, AH, AW, 0.5)
    d2, st = ops.morpho_edt(bits, W * scale)
    skel = ops.morpho_thin(bits, d2, fg, st, mm._keep, 0)
    _, values, _ = ops.morpho_measure(x, scale, skel, d2, fg, hstats, st)
    d2c, _ = ops.morpho_edt(ops.morpho_complement(bits, W * scale), W * scale)
    host = (mo.unpack_bits(bits, W * scale), d2.cpu().numpy(), mo.unpack_bits(skel, W * scale),
            values[:, 2].cpu().numpy(), st.cpu().numpy())
    return dict(bits=bits, d2=d2, d2c=d2c, skel=skel, thick=values[:, 2], status=st), host


@pytest.mark.parametrize("H,W,scale,B", SHAPES)
def test_measured_images_every_kind(H, W, scale, B):
    dev, (binary, d2, skel, thick, status) = _measured(H, W, scale, B, seed=scale)
    kinds = (np.arange(B) + scale) % 5                               # every kind in every batch of 5 or more
    rounds = [kinds] if B >= 5 else [np.full(B, k) for k in range(5)]
    for r, kd in enumerate(rounds):
        kd = kd.astype(np.int32)
        got = _twice(lambda: lc.device_local(dev["bits"], dev["d2"], dev["d2c"], dev["skel"], dev["thick"], dev["status"],
                                             _dev(kd, np.int32), scale, W * scale, seed=11))
        want = lc.statement_rows(binary, d2, skel, thick, status, kd, H, W, scale, seed=11)
        lc.compare(f"{H}x{W} s={scale} B={B} round {r}", got, want, W * scale)
        if H == 28:
            assert all(w["status"] == 0 for w in want)
            assert all(w["fallback"] == 0 and w["n_candidates"] >= 30 for w in want if w["centres"][1, 0] >= 0)


def test_complement_keeps_the_pad_bits_clear():
    from ali_hip import ops
    mo = _mo()
    g = np.random.default_rng(0)
    for Wh in (9, 32, 36, 72):
        images = g.random((2, 5, Wh)) < 0.5
        c = ops.morpho_complement(mo.pack_bits(images).to(DEV), Wh)
        assert lc.pad_bits_clear(c, Wh) and np.array_equal(mo.unpack_bits(c, Wh), ~images)


SWELL_SEED = 0


def test_swelling_through_pow():
    """strength 2.5 (an exponent of 0.75: ``pow`` on the device, whose last bits may differ from numpy's).  A pixel is
    left out only if the fp64 statement's source coordinate plus 0.5 lies within 1e-6 of an integer in either axis;
    SWELL_SEED is chosen so that none is."""
    H = W = 28
    scale, B = 16, 3
    from morphomnist import perturb as p
    dev, (binary, d2, skel, thick, status) = _measured(H, W, scale, B, seed=16)
    params = dict(lc.PARAMS, swell_strength=2.5)
    kinds = np.full(B, 3, dtype=np.int32)
    got = _twice(lambda: lc.device_local(dev["bits"], dev["d2"], dev["d2c"], dev["skel"], dev["thick"], dev["status"],
                                         _dev(kinds, np.int32), scale, W * scale, params, seed=SWELL_SEED))
    want = lc.statement_rows(binary, d2, skel, thick, status, kinds, H, W, scale, params, seed=SWELL_SEED)
    skip = np.zeros(binary.shape, dtype=bool)
    for b, w in enumerate(want):
        R = p.swelling_radius(thick[b], 7., scale)
        f = p.swell(binary[b], w["centres"][0], R, 2.5)[1]
        skip[b] = (np.abs(f - np.rint(f)) <= 1e-6).any(0)
        assert w["status"] == 0 and not np.array_equal(w["bitmap"], binary[b])
    print(f"swelling at strength 2.5: {int(skip.sum())} pixels within 1e-6 of a boundary")
    assert not skip.any()
    lc.compare("swell 2.5", got, want, W * scale, skip=skip)
