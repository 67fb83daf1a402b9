"""Morphometrics of a digit image -- ``ImageMorphology`` and ``ImageMoments`` with the attributes the measured-
counterfactual scripts use -- written on numpy and scipy alone.  This module is the *statement* the HIP kernels of
csrc/morpho.hip are tested against; agreement with scikit-image's ``pyramid_expand`` / ``medial_axis`` has not been
checked (DESIGN 3.16 says why).

  expand     hires = 255 * A(H, s) X A(W, s)^T for scale s > 1, A(n, s) the [n s, n] matrix whose column j is the
             cubic-spline zoom of the unit vector e_j (mirror boundary, grid mode) smoothed by a Gaussian of sigma
             2 s / 6 (reflect boundary, truncated at 4 sigma); s == 1: hires = X.
  binarise   bin = hires >= min + (max - min) * threshold; a constant image is all foreground (A's rows sum to 1).
  distance   d2 = the exact squared Euclidean distance to the nearest background pixel inside the image (an integer).
             An image without background has status 1, no skeleton and NaN measures.
  thin       every foreground pixel has the key (d2, corner, tiebreak, linear index): corner = 9 - the set pixels of
             its 3 x 3 neighbourhood in ``bin`` (zero padded), tiebreak = ``ali_hip.rng.thin_reference(seed, n)``.  The
             pixels are visited once each, in ascending key order, and set to KEEP[current neighbourhood].
  measures   area = foreground / s^2; stroke_length = (straight + sqrt 2 * diagonal neighbour pairs of the skeleton) / s;
             mean_thickness = 2 * mean of sqrt(d2) over the skeleton / s.
  reduce     low = R(H, s) hires R(W, s)^T, R(n, s) the [n, n s] matrix whose column k is the cubic-spline zoom by 1 / s
             (mirror boundary, grid mode) of the unit vector e_k smoothed by the same Gaussian: the transpose-shaped
             twin of A.  ``downscale`` = ``quantise`` of it (the perturbation half, morphomnist/perturb.py).
"""
import functools

import numpy as np
from scipy import ndimage

from ali_hip.rng import thin_reference

_BIT = (1 << np.arange(9)).reshape(3, 3)            # bit 3 * r + c of a neighbourhood index; the centre is bit 4


def _components(cells):
    """the number of 8-connected components of a set of (r, c) cells"""
    left, n = set(cells), 0
    while left:
        n += 1
        stack = [left.pop()]
        while stack:
            r, c = stack.pop()
            for q in [(r + dr, c + dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1)]:
                if q in left:
                    left.remove(q)
                    stack.append(q)
    return n


@functools.lru_cache(maxsize=None)
def thin_tables():
    """(keep, corner): uint8 and int64 arrays [512] over the neighbourhood index.  keep: the centre is set, and clearing
    it would change the number of 8-connected components of the pattern or the pattern has fewer than 3 set pixels
    (the end of a line stays).  corner = 9 - the set pixels."""
    keep, corner = np.zeros(512, dtype=np.uint8), np.zeros(512, dtype=np.int64)
    for i in range(512):
        cells = [(k // 3, k % 3) for k in range(9) if i >> k & 1]
        corner[i] = 9 - len(cells)
        if i >> 4 & 1:
            rest = [c for c in cells if c != (1, 1)]
            keep[i] = _components(cells) != _components(rest) or len(cells) < 3
    return keep, corner


def keep_bits():
    """the keep table as 16 words of 32 bits (what ``ali_morpho_thin`` takes)"""
    return np.packbits(thin_tables()[0], bitorder="little").view(np.uint32).copy()


@functools.lru_cache(maxsize=None)
def expand_operator(n, scale):
    """A(n, scale): float64 [n * scale, n], read-only"""
    sigma = 2 * scale / 6.0
    cols = [ndimage.gaussian_filter1d(ndimage.zoom(e, scale, order=3, mode="mirror", grid_mode=True), sigma,
                                      mode="reflect") for e in np.eye(n)]
    A = np.stack(cols, axis=1)
    A.setflags(write=False)
    return A


def expand(image, scale, dtype=np.float64):
    """hires of ``image`` [H, W]; the operators rounded to ``dtype`` and the products taken in it"""
    image = np.asarray(image, dtype=dtype)
    if scale == 1:
        return image
    H, W = image.shape
    AH, AW = expand_operator(H, scale).astype(dtype), expand_operator(W, scale).astype(dtype)
    return dtype(255) * (AH @ (image @ AW.T))


@functools.lru_cache(maxsize=None)
def reduce_operator(n, scale, order=3):
    """R(n, scale): float64 [n, n * scale], read-only; the identity at scale 1.  Its rows sum to 1 (5e-16 at (28, 16))."""
    if scale == 1:
        R = np.eye(n)
    else:
        sigma = 2 * scale / 6.0
        cols = [ndimage.zoom(ndimage.gaussian_filter1d(e, sigma, mode="reflect"), n / (n * scale), order=order,
                             mode="mirror", grid_mode=True) for e in np.eye(n * scale)]
        R = np.stack(cols, axis=1)
    R.setflags(write=False)
    return R


def reduce(image, scale, dtype=np.float64):
    """``image`` [H s, W s] brought down to [H, W]: RH image RW^T, the operators rounded to ``dtype`` and the products
    taken in it (the image's own units: no factor of 255)"""
    image = np.asarray(image, dtype=dtype)
    if scale == 1:
        return image
    Hh, Wh = image.shape
    RH, RW = reduce_operator(Hh // scale, scale).astype(dtype), reduce_operator(Wh // scale, scale).astype(dtype)
    return RH @ (image @ RW.T)


QUANTISE_GUARD = 2.0 ** -7       # of a grey level


def quantise_levels(levels):
    """floor(clip(levels, 0, 255) + 2^-7) in the dtype of ``levels`` (grey levels, 0 .. 255): float-valued integers"""
    levels = np.asarray(levels)
    return np.floor(np.clip(levels, 0, 255) + levels.dtype.type(QUANTISE_GUARD))


def quantise(v):
    """floor(clip(255 v, 0, 255) + 2^-7).  The reference writes ``(255. * v).astype(np.uint8)``, which wraps above 255
    and makes a plate of ones 254 or 255 by the last bit of a sum (the fp32 rows of R times 255 sum to 254.99998 .. 255);
    the clamp replaces the wrap and the guard of 1 / 128 grey level makes plate and background deterministic."""
    v = np.asarray(v)
    if not np.issubdtype(v.dtype, np.floating):
        v = v.astype(np.float64)
    return quantise_levels(v.dtype.type(255) * v)


def binarise(hires, threshold=.5):
    lo, hi = hires.min(), hires.max()
    return hires >= lo + (hi - lo) * threshold


def neighbourhoods(bitmap):
    """the neighbourhood index of every pixel of a boolean image (zero padded): int64 [H, W]"""
    p = np.pad(np.asarray(bitmap, dtype=np.int64), 1)
    H, W = bitmap.shape
    return sum(p[r:r + H, c:c + W] * _BIT[r, c] for r in range(3) for c in range(3))


def squared_distance(bitmap):
    """exact integer d2 [H, W] of a boolean image with at least one background pixel"""
    return np.rint(ndimage.distance_transform_edt(bitmap) ** 2).astype(np.int64)


def thin(bitmap, d2, seed=0):
    """The sequential thinning: the skeleton (bool [H, W]) of ``bitmap`` under the keys of ``d2`` and ``seed``."""
    keep, corner = thin_tables()
    H, W = bitmap.shape
    ys, xs = np.nonzero(bitmap)
    lin = ys * W + xs
    tie = thin_reference(seed, H * W)[lin]
    order = np.lexsort((lin, tie, corner[neighbourhoods(bitmap)[ys, xs]], d2[ys, xs]))     # the last key sorts first
    cur = np.pad(np.asarray(bitmap, dtype=np.uint8), 1)
    P = W + 2
    flat = cur.reshape(-1)
    offsets = [(r - 1) * P + (c - 1) for r in range(3) for c in range(3)]
    for y, x in zip(ys[order].tolist(), xs[order].tolist()):
        at = (y + 1) * P + x + 1
        idx = 0
        for k, o in enumerate(offsets):
            idx |= int(flat[at + o]) << k
        flat[at] = keep[idx]
    return cur[1:-1, 1:-1].astype(bool)


def thin_wavefront(bitmap, d2, seed=0):
    """The schedule of the kernel (csrc/morpho.hip: ali_morpho_thin) in numpy: a pixel decides as soon as every
    neighbour with a smaller key has decided.  Returns (skeleton, rounds); the skeleton is ``thin``'s."""
    keep, corner = thin_tables()
    H, W = bitmap.shape
    ys, xs = np.nonzero(bitmap)
    lin = ys * W + xs
    tie = thin_reference(seed, H * W)[lin]
    order = np.lexsort((lin, tie, corner[neighbourhoods(bitmap)[ys, xs]], d2[ys, xs]))
    rank = np.full((H + 2, W + 2), -1, dtype=np.int64)               # -1: not foreground
    rank[ys[order] + 1, xs[order] + 1] = np.arange(len(order))
    shifts = [(r, c) for r in range(3) for c in range(3) if (r, c) != (1, 1)]
    nb = np.stack([rank[r:r + H, c:c + W] for r, c in shifts])       # the eight neighbours' ranks
    mine = rank[1:-1, 1:-1]
    waits = (nb >= 0) & (nb < mine)                                  # the neighbours a pixel waits for
    cur = np.asarray(bitmap, dtype=bool).copy()
    undecided = cur.copy()
    rounds = 0
    while undecided.any():
        u = np.pad(undecided, 1)
        pending = np.stack([u[r:r + H, c:c + W] for r, c in shifts])
        ready = undecided & ~(waits & pending).any(0)
        assert ready.any() and rounds <= len(order)
        cur[ready] = keep[neighbourhoods(cur)[ready]].astype(bool)
        undecided &= ~ready
        rounds += 1
    return cur, rounds


def skeleton_pairs(skel):
    """(straight, diagonal): the pairs (p, q) of skeleton pixels with q right of / below p, and below-left / -right"""
    s = np.pad(np.asarray(skel, dtype=np.int64), 1)
    c = s[1:-1, 1:-1]
    straight = (c * s[1:-1, 2:]).sum() + (c * s[2:, 1:-1]).sum()
    diagonal = (c * s[2:, :-2]).sum() + (c * s[2:, 2:]).sum()
    return int(straight), int(diagonal)


class ImageMorphology:
    """The processing pipeline of one image [H, W]: ``hires_image``, ``binary_image``, ``skeleton`` (bool) and
    ``distance_map`` (sqrt(d2); NaN everywhere when ``status`` is 1), with ``area``, ``stroke_length`` and
    ``mean_thickness``.  ``dtype`` is the precision of the expand product (float64: the statement; float32: the
    yardstick the tests hold the kernels against); the measures are formed in it too."""

    def __init__(self, image, threshold=.5, scale=1, seed=0, dtype=np.float64, binary=None):
        self.image = np.asarray(image)
        self.threshold, self.scale, self.seed = threshold, int(scale), seed
        self.hires_image = expand(self.image, self.scale, dtype)
        # (``binary``: continue from a given binary image, e.g. the one a kernel produced, instead of thresholding)
        if binary is not None:
            self.binary_image = np.asarray(binary, dtype=bool)
        elif self.image.max() == self.image.min():      # constant: so is hires, but for the rounding of the products
            self.binary_image = np.ones(self.hires_image.shape, dtype=bool)
        else:
            self.binary_image = binarise(self.hires_image, threshold)
        self.status = int(self.binary_image.all())
        self.dtype = dtype
        if self.status:
            self.squared_distance = None
            self.distance_map = np.full(self.binary_image.shape, np.nan)
            self.skeleton = np.zeros_like(self.binary_image)
        else:
            self.squared_distance = squared_distance(self.binary_image)
            self.distance_map = np.sqrt(self.squared_distance.astype(dtype))
            self.skeleton = thin(self.binary_image, self.squared_distance, seed)

    @property
    def area(self):
        return float("nan") if self.status else self.dtype(self.binary_image.sum()) / self.dtype(self.scale ** 2)

    @property
    def stroke_length(self):
        if self.status:
            return float("nan")
        straight, diagonal = skeleton_pairs(self.skeleton)
        return (self.dtype(straight) + np.sqrt(self.dtype(2)) * self.dtype(diagonal)) / self.dtype(self.scale)

    @property
    def mean_thickness(self):
        if self.status or not self.skeleton.any():
            return float("nan")
        return self.dtype(2) * np.mean(self.distance_map[self.skeleton]) / self.dtype(self.scale)

    def downscale(self, image):
        """``image`` [H s, W s] in the units of a bitmap (0 .. 1) -> [H, W] grey levels, float-valued integers in
        ``dtype``: ``quantise(reduce(image))``"""
        return quantise(reduce(np.asarray(image, dtype=self.dtype), self.scale, self.dtype))


class ImageMoments:
    """Mass, centroid and central second moments of an image; x runs along the second axis, y along the first."""

    def __init__(self, img, dtype=float):
        img = np.asarray(img, dtype=dtype)
        y, x = (g.astype(dtype) for g in np.mgrid[:img.shape[0], :img.shape[1]])
        with np.errstate(invalid="ignore", divide="ignore"):
            self.m00 = img.sum()
            self.m10, self.m01 = (x * img).sum() / self.m00, (y * img).sum() / self.m00
            self.u20 = (x * x * img).sum() / self.m00 - self.m10 ** 2
            self.u11 = (x * y * img).sum() / self.m00 - self.m10 * self.m01
            self.u02 = (y * y * img).sum() / self.m00 - self.m01 ** 2

    @property
    def centroid(self):
        return self.m10, self.m01

    @property
    def covariance(self):
        return self.u20, self.u11, self.u02

    @property
    def axis_lengths(self):
        mid, delta = .5 * (self.u20 + self.u02), .5 * np.hypot(2. * self.u11, self.u20 - self.u02)
        return np.sqrt(mid + delta), np.sqrt(mid - delta)

    @property
    def angle(self):
        return .5 * np.arctan2(2. * self.u11, self.u20 - self.u02)

    @property
    def horizontal_shear(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.u11 / self.u02

    @property
    def vertical_shear(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.u11 / self.u20


def quantile_loc(c, f, side):
    """Where the cdf ``c`` [n] crosses the level ``f``, interpolated as ``np.interp(f, c, arange(n))`` interpolates.
    ``c`` need not be monotone (the up-sampled image rings below zero), so the crossing is a definition:
    0 if f < c[0]; n - 1 if f >= c[-1]; otherwise the first j with c[j] <= f < c[j + 1] for ``side`` "left" (left, top)
    or the last such j for "right" (right, bottom), and np.interp's own formula on it -- the same bits as np.interp
    wherever the crossing is unique."""
    c = np.asarray(c, dtype=np.float64)
    n = len(c)
    f = np.float64(f)
    if not f >= c[0]:
        return np.float64(0)
    if f >= c[-1]:
        return np.float64(n - 1)
    hits = np.nonzero((c[:-1] <= f) & (f < c[1:]))[0]
    j = int(hits[0] if side == "left" else hits[-1])
    if f == c[j]:
        return np.float64(j)
    slope = (np.float64(j + 1) - np.float64(j)) / (c[j + 1] - c[j])
    return slope * (f - c[j]) + np.float64(j)


def horizontal_cdf(img, shear, middle):
    """hcdf [W]: the mass left of each sheared line t, sum((x + .5 < t + shear * (y - middle)) * img) / img.sum(), as
    the reference's ``_horz_cdf`` writes it"""
    img = np.asarray(img, dtype=float)
    height, width = img.shape
    x = np.arange(width)[None, :]
    y = np.arange(height)[:, None]
    counts = np.zeros(width)
    for t in range(width):
        counts[t] = ((x + .5 < t + shear * (y - middle)) * img).sum()
    return counts / img.sum()


def vertical_cdf(img):
    """vcdf [H]: the mass above each row t, sum((y < t) * img) / img.sum(), as the reference's ``_vert_cdf``"""
    img = np.asarray(img, dtype=float)
    y = np.arange(img.shape[0])[:, None]
    counts = np.zeros(img.shape[0])
    for t in range(img.shape[0]):
        counts[t] = ((y < t) * img).sum()
    return counts / img.sum()


def bounds_of(img, frac, moments=None):
    """(left, right, top, bottom, shear, middle, hcdf, vcdf) of ``bounding_parallelogram`` (float64; the four locations
    NaN when the mass is not positive or the shear not finite)"""
    img = np.asarray(img, dtype=float)
    if moments is None:
        moments = ImageMoments(img)
    middle = np.float64(moments.centroid[1])
    shear = np.float64(moments.horizontal_shear)
    with np.errstate(invalid="ignore", divide="ignore"):
        hcdf = horizontal_cdf(img, shear, middle)
        vcdf = vertical_cdf(img)
    if not (img.sum() > 0 and np.isfinite(shear)):
        nan = np.float64(np.nan)
        return nan, nan, nan, nan, shear, middle, hcdf, vcdf
    half = frac / 2                                                  # two-sided
    left, right = quantile_loc(hcdf, half, "left"), quantile_loc(hcdf, 1. - half, "right")
    top, bottom = quantile_loc(vcdf, half, "left"), quantile_loc(vcdf, 1. - half, "right")
    return left, right, top, bottom, shear, middle, hcdf, vcdf


def corners_of(left, right, top, bottom, shear, middle):
    """the parallelogram's corners as (x, y) arrays, clockwise from the top left (the reference's)"""
    top_left = np.array([left + shear * (top - middle), top])
    top_right = np.array([right + shear * (top - middle), top])
    bottom_left = np.array([left + shear * (bottom - middle), bottom])
    bottom_right = np.array([right + shear * (bottom - middle), bottom])
    return top_left, top_right, bottom_right, bottom_left


def bounding_parallelogram(img, frac, moments=None):
    """The corners (top left, top right, bottom right, bottom left; (x, y) arrays) of the parallelogram that leaves
    ``frac`` / 2 of the mass of ``img`` outside each side, its slanted sides along the image's horizontal shear through
    the centroid row.  ``moments``: any object with ``centroid`` and ``horizontal_shear``.  The crossings follow
    ``quantile_loc``; the corners are NaN when the mass is not positive or the shear not finite."""
    return corners_of(*bounds_of(img, frac, moments)[:6])


def measure_bounds(image, scale, bound_frac, dtype=np.float64):
    """The bounding-parallelogram half of ``measure_image``: hires = expand(image - image.min(), scale)
    with the product in ``dtype`` (float64: the statement; float32: the yardstick of the device), then the reference's
    fp64 moments and ``bounding_parallelogram``.  Returns {"bounds": float64 [6] = left, right, top, bottom, shear,
    middle; "corners": float64 [4, 2]; "width", "height": (right - left) / scale, (bottom - top) / scale; "slant":
    arctan(-shear); "hires"}."""
    image = np.asarray(image, dtype=dtype)
    hires = expand(image - image.min(), scale, dtype)
    moments = ImageMoments(hires)
    b = bounds_of(hires, bound_frac, moments)[:6]
    with np.errstate(invalid="ignore"):
        return {"bounds": np.array(b, dtype=np.float64), "corners": np.stack(corners_of(*b)),
                "width": (b[1] - b[0]) / scale, "height": (b[3] - b[2]) / scale, "slant": np.arctan(-b[4]),
                "hires": hires}


def intensity(image):
    """the median of the pixels in the upper half of the image's range (np.median: the mean of the two middle values
    for an even count), in the image's units"""
    image = np.asarray(image)
    lo, hi = image.min(), image.max()
    return np.median(image[image >= lo + (hi - lo) * .5])
