"""Shared by tests/test_morphomnist_local_cpu.py, tests/test_gpu_morpho_local_kernels.py and
tests/test_gpu_morphomnist_local.py: built skeletons, the bitmaps around them, and the comparison of the two kernels
``ali_morpho_locate`` / ``ali_morpho_local`` with the statement ``morphomnist.perturb.local_continue_from``."""
import numpy as np
from scipy import ndimage

import morpho_cases as mc

KINDS = ("plain", "thin", "thick", "swell", "fracture")
PARAMS = dict(thin_amount=.7, thick_amount=1., swell_strength=3., swell_radius=7., frac_thickness=1.5, frac_prune=2.,
              num_frac=3)
INT_KEYS = ("status", "radius", "n_candidates", "fallback")


def tee(H=24, W=72):
    """a T-junction: a horizontal run across the word boundaries and a stem down from x = 33"""
    s = np.zeros((H, W), dtype=bool)
    s[4, 20:60] = True
    s[5:H - 2, 33] = True
    return s


def plus(H=24, W=72):
    s = np.zeros((H, W), dtype=bool)
    s[11, 22:43] = True
    s[2:21, 32] = True
    return s


def ring_skeleton(H=24, W=72):
    """a closed 8-connected loop without tips: every pixel has 2 neighbours"""
    s = np.zeros((H, W), dtype=bool)
    s[3, 26:40] = True
    s[20, 26:40] = True
    s[4:20, 25] = True
    s[4:20, 40] = True
    return s


def skeletons(H=24, W=72):
    """{name: bool [H, W]}: the crossings of the word boundary at x = 32 of ``morpho_cases.skeleton_cases``, a T, a plus,
    a ring, one pixel, nothing, and the skeletons of two blob images"""
    from morphomnist import morpho
    out = {k: v[0] for k, v in mc.skeleton_cases(H, W).items()}
    one = np.zeros((H, W), dtype=bool)
    one[H // 2, 32] = True
    out.update(tee=tee(H, W), plus=plus(H, W), ring=ring_skeleton(H, W), one=one)
    for k in range(2):
        b = mc.blobs(H, W, seed=k, fill=0.35)
        b[0, :] = b[-1, :] = False
        out[f"blobs{k}"] = morpho.thin(b, morpho.squared_distance(b))
    return out


def around(skel, grow=2):
    """(binary, d2, d2c, thickness at scale 1) around a built skeleton: the skeleton dilated ``grow`` times by the 3 x 3
    square; the thickness is 2 * mean sqrt(d2) over the skeleton (NaN without one)"""
    from morphomnist import morpho
    binary = ndimage.binary_dilation(skel, np.ones((3, 3), dtype=bool), iterations=grow) if skel.any() else skel.copy()
    d2 = morpho.squared_distance(binary) if not binary.all() else np.zeros(binary.shape, dtype=np.int64)
    d2c = morpho.squared_distance(~binary) if binary.any() else np.zeros(binary.shape, dtype=np.int64)
    thick = np.float32(2 * np.sqrt(d2[skel]).mean()) if skel.any() else np.float32("nan")
    return binary, d2, d2c, thick


def pad_bits_clear(words, Wh):
    w = words.cpu().numpy().view(np.uint32)
    return not (Wh % 32) or not (w[:, :, -1] >> (Wh % 32)).any()


def device_local(bits, d2, d2c, skel, thick, status, kinds, scale, Wh, params=PARAMS, seed=0, counter=None, offset=0):
    """locate and local on device tensors: the dict of ``MorphoLocal.apply`` less the images, with the moment sums"""
    from ali_hip import ops
    from morphomnist import perturb
    from morphomnist.skeleton import prune_radius
    prune = prune_radius(params["frac_prune"], scale)
    n_cand, fb, ce, en = ops.morpho_locate(skel, d2, status, kinds, scale, prune, prune, params["num_frac"], seed, counter,
                                           offset)
    new, radius, sums, st = ops.morpho_local(bits, Wh, d2, d2c, thick, status, kinds, n_cand, ce, en, scale,
                                             params["thin_amount"], params["thick_amount"], params["swell_strength"],
                                             params["swell_radius"],
                                             perturb.fracture_radius(params["frac_thickness"], scale), params["num_frac"])
    return dict(bits=new, radius=radius, sums=sums, status=st, n_candidates=n_cand, fallback=fb, centres=ce, endpoints=en)


def statement_rows(binary, d2, skel, thick, status, kinds, H, W, scale, params=PARAMS, seed=0, counter=0, offset=0,
                   dtype=np.float64):
    """``local_continue_from`` for every row of numpy intermediates; row b draws as global row ``offset + b``"""
    from morphomnist import perturb
    return [perturb.local_continue_from(binary[b], d2[b], skel[b], thick[b], int(kinds[b]), H, W, scale, int(status[b]),
                                        dtype, seed, counter, offset + b, **params) for b in range(len(binary))]


def compare(name, got, want, Wh, bitmaps=True, skip=None):
    """the device's dict against the statement's rows: every integer and the bitmap exactly.  ``skip``: bool [B, Hh, Wh]
    pixels left out of the bitmap comparison."""
    from ali_hip import morpho as mo
    assert pad_bits_clear(got["bits"], Wh), name
    maps = mo.unpack_bits(got["bits"], Wh)
    host = {k: got[k].cpu().numpy() for k in INT_KEYS + ("centres", "endpoints")}
    for b, w in enumerate(want):
        for k in INT_KEYS:
            assert int(host[k][b]) == int(w[k]), (name, b, k, int(host[k][b]), int(w[k]))
        assert np.array_equal(host["centres"][b], w["centres"]), (name, b, host["centres"][b], w["centres"])
        assert np.array_equal(host["endpoints"][b], w["endpoints"]), (name, b, host["endpoints"][b], w["endpoints"])
        if bitmaps:
            differ = maps[b] != w["bitmap"]
            if skip is not None:
                differ &= ~skip[b]
            assert not differ.any(), (name, b, int(differ.sum()), np.argwhere(differ)[:4].tolist())
        if w["status"]:
            assert not maps[b].any(), (name, b)
