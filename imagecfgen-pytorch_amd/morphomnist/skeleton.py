"""Locations along a skeleton -- ``num_neighbours``, ``erase``, ``get_angle`` and ``LocationSampler`` of the reference's
``morphomnist.skeleton`` -- written on numpy alone.  This module is the *statement* the kernel ``ali_morpho_locate``
(csrc/morpho.hip) is tested against; agreement with scikit-image's ``disk`` has not been checked (DESIGN 3.20 says
why, and lists the deviations).

  neighbours  the 8-neighbour count of every skeleton pixel, zero padded; 0 off the skeleton.
  erase       every skeleton pixel p with a seed q, |p - q|^2 <= r^2, is cleared (the exact disk).
  candidates  erase around the tips (1 neighbour), then around the forks (3 neighbours) of what the first erase left.
  direction   (cos, sin) of the major axis of the skeleton inside a square window, from six integer sums, in fp64 with
              square roots and divisions only: the same bits on the host and on the device.
  sample      draw k of image ``row`` is candidate ``ali_hip.rng.locate_reference(seed, counter, n, row, k)`` in
              row-major order: the counter RNG, not ``np.random``; with replacement.
"""
import numpy as np

from ali_hip.rng import MAX_DRAWS, locate_reference


def num_neighbours(skel):
    """int64 [H, W]: the number of set 8-neighbours of every set pixel (outside the image is 0), 0 elsewhere"""
    s = np.asarray(skel).astype(bool).astype(np.int64)
    H, W = s.shape
    p = np.pad(s, 1)
    total = sum(p[r:r + H, c:c + W] for r in range(3) for c in range(3)) - s
    return total * s


def erase(skel, seeds, r):
    """``skel`` without the pixels p that have a seed q with |p - q|^2 <= r^2; r = 0 clears the seeds themselves"""
    skel = np.asarray(skel, dtype=bool)
    out = skel.copy()
    r = int(r)
    H, W = skel.shape
    for i, j in zip(*np.nonzero(seeds)):
        lo_i, hi_i, lo_j, hi_j = max(i - r, 0), min(i + r + 1, H), max(j - r, 0), min(j + r + 1, W)
        y, x = np.mgrid[lo_i:hi_i, lo_j:hi_j]
        out[lo_i:hi_i, lo_j:hi_j] &= (y - i) ** 2 + (x - j) ** 2 > r * r
    return out


def prune_radius(prune, scale):
    """int(prune * scale), or None"""
    return None if prune is None else int(prune * scale)


def candidates(skel, scale, prune_tips=None, prune_forks=None):
    """The skeleton pruned around its tips, then around the forks of the pruned skeleton (bool [H, W])"""
    skel = np.asarray(skel, dtype=bool)
    if prune_tips is not None:
        skel = erase(skel, num_neighbours(skel) == 1, prune_radius(prune_tips, scale))
    if prune_forks is not None:
        skel = erase(skel, num_neighbours(skel) == 3, prune_radius(prune_forks, scale))
    return skel


def window_sums(skel, i, j, r):
    """(n, sum x, sum y, sum x^2, sum x y, sum y^2) as Python ints over the set pixels of the (2 r + 1)^2 window around
    (i, j); x is the column and y the row inside the window, 0 .. 2 r; outside the image is 0"""
    skel = np.asarray(skel, dtype=bool)
    H, W = skel.shape
    i, j, r = int(i), int(j), int(r)
    lo_i, hi_i, lo_j, hi_j = max(i - r, 0), min(i + r + 1, H), max(j - r, 0), min(j + r + 1, W)
    ys, xs = np.nonzero(skel[lo_i:hi_i, lo_j:hi_j])
    ys = ys.astype(np.int64) + (lo_i - (i - r))
    xs = xs.astype(np.int64) + (lo_j - (j - r))
    return tuple(int(v) for v in (len(ys), xs.sum(), ys.sum(), (xs * xs).sum(), (xs * ys).sum(), (ys * ys).sum()))


def direction(sums):
    """(cos t, sin t) of t = 0.5 * arctan2(2 u11, u20 - u02) for the moments behind ``sums``, in fp64 without
    trigonometric functions: a = n sxx - sx^2 - (n syy - sy^2) and b = 2 (n sxy - sx sy) are exact integers, h =
    sqrt(a a + b b), c2 = a / h, cos = sqrt((1 + c2) / 2), sin = copysign(sqrt((1 - c2) / 2), b) -- every operation
    rounded once.  h == 0 (one pixel, nothing, or an isotropic window): (1, 0)."""
    n, sx, sy, sxx, sxy, syy = (int(v) for v in sums)
    A, C, Bc = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
    a, b = np.float64(A - C), np.float64(2 * Bc)
    h = np.sqrt(a * a + b * b)
    if h == 0:
        return np.float64(1), np.float64(0)
    c2 = a / h
    one, two = np.float64(1), np.float64(2)
    return np.sqrt((one + c2) / two), np.copysign(np.sqrt((one - c2) / two), b)


def get_angle(skel, i, j, r):
    """the local angle of the skeleton inside the window of radius r around (i, j), in radians"""
    c, s = direction(window_sums(skel, i, j, r))
    return float(np.arctan2(s, c))


class LocationSampler:
    """Random pixel locations along the skeleton of an ``ImageMorphology``, away from its tips and forks by
    ``prune_tips`` / ``prune_forks`` low-resolution pixels (None: not pruned)."""

    def __init__(self, prune_tips=None, prune_forks=None):
        self.prune_tips, self.prune_forks = prune_tips, prune_forks

    def candidates(self, morph):
        return candidates(morph.skeleton, morph.scale, self.prune_tips, self.prune_forks)

    def sample(self, morph, num=None, seed=0, counter=0, row=0):
        """(i, j) for ``num`` None, else int64 [num, 2]: draws 0 .. num - 1 of image ``row`` under (seed, counter)"""
        n = 1 if num is None else int(num)
        if not 0 <= n <= MAX_DRAWS:
            raise ValueError(f"LocationSampler: num in 0 .. {MAX_DRAWS}")
        coords = np.argwhere(self.candidates(morph))               # row-major
        if coords.shape[0] == 0:
            raise ValueError("Overpruned skeleton")
        idx = [locate_reference(seed, counter, coords.shape[0], row, k) for k in range(n)]
        picked = coords[idx].astype(np.int64).reshape(n, 2)
        return picked[0] if num is None else picked
