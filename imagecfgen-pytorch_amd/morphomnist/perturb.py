"""The perturbations the measured-counterfactual scripts and the data-set builders use -- ``SetThickness``, ``SetSlant``,
``SetIntensity``, ``SetWidth`` -- and the four of the published Morpho-MNIST data sets -- ``Thinning``, ``Thickening``,
``Swelling``, ``Fracture`` -- written on numpy and scipy alone, with the scripts' five-line chain for one image,
``counterfactual_image``, the data sets' chain, ``local_image``, and the width chain, ``width_image``.  This module is
the *statement* the kernels ``ali_morpho_reshape``, ``ali_morpho_shear_reduce``, ``ali_morpho_set_intensity``,
``ali_morpho_locate``, ``ali_morpho_local``, ``ali_morpho_width`` and ``ali_morpho_affine_reduce`` (csrc/morpho.hip) are
tested against; agreement with scikit-image's ``dilation`` / ``pyramid_reduce`` / ``warp`` / ``draw.line`` has not been
checked (DESIGN 3.17, 3.20 and 3.22 say why, and list the deviations).

  footprint  ``SetThickness`` dilates / erodes by a disk of 16 r made small again: the support of zoom(gaussian(disk(16 r),
             16 / 3), (2 r + 1) / (32 r + 1), order 1).  The 16 is the reference's constant in ``_get_disk``, not the
             image scale.  Every row of it is one centred run, so a footprint is its half widths.
  reshape    flat dilation by the footprint (outside the image is background), or erosion, its dual on the image's own
             pixels (outside the image does not constrain it).
  shear      row y of the bitmap read at column x + floor(0.5 - delta (y - cy)): nearest neighbour, constant 0.
  reduce     ``ImageMorphology.downscale``: quantise(RH bitmap RW^T) (morphomnist/morpho.py).
  intensity  clip(q * (target / median), 0, 255), the median of the pixels of q in the upper half of its range.
  thin       ``Thinning``: d2 > r^2, r = int(amount * scale * thickness / 2); ``Thickening``: the same of the complement.
  swell      ``Swelling``: the radial power warp around a location drawn on the skeleton, nearest neighbour, 0 outside.
  fracture   ``Fracture``: cuts of a disk brush along digital lines across the stroke, at locations drawn on the skeleton
             away from its tips and forks (``morphomnist.skeleton``), perpendicular to its local direction.
  width      ``SetWidth``: row y of the bitmap read at the column ``width_columns`` gives -- the horizontal scaling by
             factor = measured width / target about the bitmap's centroid that keeps its shear -- nearest neighbour,
             constant 0.  The width is the bounding parallelogram's, measured on the grey up-sampled image under the
             bitmap's shear and centroid row (``measure_width``).
"""
import functools

import numpy as np
from scipy import ndimage

from .morpho import (ImageMoments, ImageMorphology, binarise, bounds_of, expand, intensity, measure_bounds,
                     quantise_levels, reduce, squared_distance)

DISK_SCALE = 16                  # the reference's ``_get_disk(radius, scale=16)``
MAX_RADIUS = 64                  # the largest radius the kernels take (a 2049 x 2049 disk on the host, once)
RADIUS_CAP = 2.0 ** 30           # a radius is reported up to here (status 3 long before)

OK, NO_BACKGROUND, THIN_STUCK, RADIUS_TOO_LARGE, NOTHING_LEFT, BAD_TARGET = 0, 1, 2, 3, 4, 5


def disk(k):
    """x^2 + y^2 <= k^2: bool [2 k + 1, 2 k + 1]"""
    y, x = np.mgrid[-k:k + 1, -k:k + 1]
    return x * x + y * y <= k * k


@functools.lru_cache(maxsize=None)
def footprint(r):
    """the structuring element of ``SetThickness`` for radius r: bool [2 r + 1, 2 r + 1], read-only.  scikit-image hands
    the float disk to ``ndi.grey_dilation``, which casts it to bool: the support is the footprint."""
    r = int(r)
    if r == 0:
        f = np.ones((1, 1), dtype=bool)
    else:
        big = ndimage.gaussian_filter(disk(DISK_SCALE * r).astype(np.float64), DISK_SCALE / 3, mode="reflect")
        z = ndimage.zoom(big, (2 * r + 1) / (2 * DISK_SCALE * r + 1), order=1, mode="mirror", grid_mode=True)
        f = z > 0
    assert f.shape == (2 * r + 1, 2 * r + 1)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def half_widths(r):
    """int64 [2 r + 1]: row dy of ``footprint(r)`` is the run of columns -h .. h around the centre, h = half_widths[dy]"""
    f = footprint(r)
    n = f.sum(1)
    h = (n - 1) // 2
    cols = np.arange(-int(r), int(r) + 1)
    assert (n % 2 == 1).all() and (f == (np.abs(cols)[None, :] <= h[:, None])).all(), r   # one centred run, none empty
    h.setflags(write=False)
    return h


def half_width_table(max_radius=MAX_RADIUS):
    """int16 [max_radius + 1, 2 * max_radius + 1]: row r holds ``half_widths(r)`` in its first 2 r + 1 entries, -1 behind
    them (what ``ali_morpho_reshape`` takes)"""
    table = np.full((max_radius + 1, 2 * max_radius + 1), -1, dtype=np.int16)
    for r in range(max_radius + 1):
        table[r, :2 * r + 1] = half_widths(r)
    return table


def _row_dilate(bitmap, h):
    """out(y, x) = any of bitmap(y, x - h .. x + h) inside the image"""
    H, W = bitmap.shape
    c = np.concatenate([np.zeros((H, 1), dtype=np.int64), np.cumsum(bitmap, axis=1, dtype=np.int64)], axis=1)
    x = np.arange(W)
    return c[:, np.minimum(x + h + 1, W)] - c[:, np.maximum(x - h, 0)] > 0


def dilate(bitmap, r):
    """flat dilation of a boolean image by ``footprint(r)``; outside the image is background"""
    bitmap = np.asarray(bitmap, dtype=bool)
    H, W = bitmap.shape
    out = np.zeros((H, W), dtype=bool)
    rows = {}
    for k, h in enumerate(half_widths(r).tolist()):
        dy = k - int(r)
        if h not in rows:
            rows[h] = _row_dilate(bitmap, h)
        lo, hi = max(0, -dy), min(H, H - dy)                         # out rows y with 0 <= y + dy < H
        if lo < hi:
            out[lo:hi] |= rows[h][lo + dy:hi + dy]
    return out


def erode(bitmap, r):
    """flat erosion by ``footprint(r)``; outside the image does not constrain it: ~dilate(~bitmap)"""
    return ~dilate(~np.asarray(bitmap, dtype=bool), r)


def signed_radius(thickness, target, scale):
    """``SetThickness``'s radius with the sign of delta (dilate >= 0 > erode), formed in fp64 from the two values as
    given: int(scale * |target - thickness| / 2), reported up to 2^30.  None for a NaN."""
    delta = np.float64(target) - np.float64(thickness)
    if np.isnan(delta):
        return None
    r = int(min(np.float64(scale) * abs(delta) / 2.0, RADIUS_CAP))
    return r if delta >= 0 else -r


def reshape(bitmap, radius):
    """``dilate`` for radius >= 0, ``erode`` by -radius below"""
    return dilate(bitmap, radius) if radius >= 0 else erode(bitmap, -radius)


def moment_sums(bitmap):
    """the six integer sums of a boolean image: count, sum x, sum y, sum x^2, sum x y, sum y^2 (int64 [6])"""
    ys, xs = np.nonzero(bitmap)
    return np.array([len(ys), xs.sum(), ys.sum(), (xs * xs).sum(), (xs * ys).sum(), (ys * ys).sum()], dtype=np.int64)


def one_row(sums):
    """u02 == 0: every set pixel lies in one row (count * sum y^2 == (sum y)^2, in integers)"""
    n, _, sy, _, _, syy = (int(v) for v in sums)
    return n * syy == sy * sy


def horizontal_shear(sums):
    """u11 / u02 of a bitmap from its integer sums, in fp64: bit for bit what ``ImageMoments(bitmap).horizontal_shear``
    gives (its sums are integers below 2^53).  Returns (shear, cy)."""
    n, sx, sy, _, sxy, syy = (np.float64(v) for v in sums)
    m10, m01 = sx / n, sy / n
    u11, u02 = sxy / n - m10 * m01, syy / n - m01 * m01
    return u11 / u02, m01


def shear_shifts(delta, cy, Hh, Wh):
    """int64 [Hh]: floor(0.5 - delta * (y - cy)) in fp64 -- one subtraction, one product, one subtraction, one floor,
    none fused -- held to -Wh .. Wh (a shift of Wh already reads outside the image everywhere)"""
    y = np.arange(Hh, dtype=np.float64)
    return np.clip(np.floor(np.float64(0.5) - np.float64(delta) * (y - np.float64(cy))), -Wh, Wh).astype(np.int64)


def shift_rows(bitmap, shifts):
    """out(y, x) = bitmap(y, x + shifts[y]), 0 outside the image"""
    bitmap = np.asarray(bitmap, dtype=bool)
    H, W = bitmap.shape
    src = np.arange(W)[None, :] + np.asarray(shifts, dtype=np.int64)[:, None]
    inside = (src >= 0) & (src < W)
    return inside & bitmap[np.arange(H)[:, None], np.clip(src, 0, W - 1)]


def set_intensity(q, target, dtype=np.float64):
    """(clip(q * (target / median), 0, 255), median): the median of the pixels of q in the upper half of its range, the
    factor and the product in ``dtype``"""
    q = np.asarray(q, dtype=dtype)
    median = dtype(intensity(q))
    if target is None:
        return q, median
    return np.clip(q * (dtype(target) / median), 0, 255), median


class Perturbation:
    def __call__(self, morph):
        """the perturbed hi-res image [H s, W s] of ``morph``; ``morph.downscale`` brings it back"""
        raise NotImplementedError


def _disk_erode(bitmap, radius):
    """erosion by the exact ``disk(radius)``: d2 > r^2 (outside the image does not constrain it)"""
    if bitmap.all():
        return bitmap.copy()
    return squared_distance(bitmap) > radius * radius


class Thinning(Perturbation):
    """thin a digit by ``amount`` of its thickness: erosion by the exact disk"""

    def __init__(self, amount=.7):
        self.amount = amount

    def __call__(self, morph):
        radius = int(self.amount * morph.scale * morph.mean_thickness / 2.)
        return _disk_erode(morph.binary_image, radius)


class Thickening(Perturbation):
    """thicken a digit by ``amount`` of its thickness: dilation by the exact disk"""

    def __init__(self, amount=1):
        self.amount = amount

    def __call__(self, morph):
        radius = int(self.amount * morph.scale * morph.mean_thickness / 2.)
        return ~_disk_erode(~morph.binary_image, radius)


class SetThickness(Perturbation):
    def __init__(self, target_thickness):
        self.target_thickness = target_thickness

    def __call__(self, morph):
        radius = signed_radius(morph.mean_thickness, self.target_thickness, morph.scale)
        if radius is None:
            raise ValueError("SetThickness: the image has no thickness (no skeleton, or no background)")
        return reshape(morph.binary_image, radius)


class SetSlant(Perturbation):
    """``transform.warp`` of the boolean image under the shear that brings its slant to the target: nearest neighbour,
    constant 0, so a horizontal shift per row.  (scikit-image before 0.17 interpolated a bool image linearly: not
    built.)"""

    def __init__(self, target_slant_rad):
        self.target_shear = -np.tan(np.float64(target_slant_rad))

    def __call__(self, morph):
        binary = morph.binary_image
        delta = self.target_shear - ImageMoments(binary).horizontal_shear
        return shift_rows(binary, shear_shifts(delta, ImageMoments(binary).m01, *binary.shape))


class SetIntensity(Perturbation):
    """as the reference has it, on top of ``downscale``: the median is the hi-res image's, the product the low-res one's"""

    def __init__(self, target_intensity):
        self.target_intensity = target_intensity

    def __call__(self, morph):
        mult = self.target_intensity / intensity(morph.hires_image)
        return np.clip(morph.downscale(morph.hires_image) * mult, 0, 255)


def reshape_stage(binary, thickness, target_thickness, scale, status=OK, max_radius=MAX_RADIUS):
    """``SetThickness`` with its corners, as ``ali_morpho_reshape`` has it: (bitmap, signed radius, moment sums,
    status); with a status the bitmap and the sums are 0, and the radius too unless the status is 3"""
    zero, none = np.zeros(np.shape(binary), dtype=bool), np.zeros(6, dtype=np.int64)
    if status:
        return zero, 0, none, int(status)
    radius = signed_radius(thickness, thickness if target_thickness is None else target_thickness, scale)
    if radius is None:
        return zero, 0, none, NOTHING_LEFT
    if abs(radius) > max_radius:
        return zero, radius, none, RADIUS_TOO_LARGE
    reshaped = reshape(binary, radius)
    sums = moment_sums(reshaped)
    if sums[0] == 0 or one_row(sums):
        return zero, radius, none, NOTHING_LEFT
    return reshaped, radius, sums, OK


def shear_stage(reshaped, sums, target_shear, scale, dtype=np.float64):
    """``SetSlant`` and the reduce of a bitmap with status 0, as ``ali_morpho_shear_reduce`` has them: (u11 / u02,
    shifts, warped bitmap, raw = 255 * reduce in ``dtype``, quantised).  ``target_shear`` = -tan(slant), or None."""
    Hh, Wh = reshaped.shape
    shear, cy = horizontal_shear(sums)
    delta = np.float64(0) if target_shear is None else np.float64(target_shear) - shear
    shifts = shear_shifts(delta, cy, Hh, Wh)
    warped = shift_rows(reshaped, shifts)
    raw = dtype(255) * reduce(warped, scale, dtype)
    return shear, shifts, warped, raw, quantise_levels(raw)


def continue_from(binary, thickness, H, W, target_thickness=None, target_shear=None, target_intensity=None, scale=16,
                  status=OK, dtype=np.float64, max_radius=MAX_RADIUS):
    """The chain from a binary image [H s, W s] and its measured thickness on (the tests hand it the device's own):
    the dict of ``counterfactual_image``.  ``target_shear`` = -tan(slant)."""
    Hh, Wh = H * scale, W * scale
    out = dict(thickness=thickness, shear=np.float64("nan"), shifts=np.zeros(Hh, dtype=np.int64),
               warped=np.zeros((Hh, Wh), dtype=bool), raw=np.zeros((H, W), dtype=dtype),
               quantised=np.zeros((H, W), dtype=dtype), median=dtype("nan"), image=np.zeros((H, W), dtype=dtype))
    out["reshaped"], out["radius"], out["sums"], out["status"] = reshape_stage(binary, thickness, target_thickness, scale,
                                                                               status, max_radius)
    if out["status"]:
        return out
    out["shear"], out["shifts"], out["warped"], out["raw"], q = shear_stage(out["reshaped"], out["sums"], target_shear,
                                                                            scale, dtype)
    if q.max() == 0:
        out["status"] = NOTHING_LEFT
        return out
    out["quantised"] = q
    out["image"], out["median"] = set_intensity(q, target_intensity, dtype)
    return out


def counterfactual_image(image, thickness=None, slant=None, intensity=None, scale=16, threshold=.5, seed=0,
                         dtype=np.float64, max_radius=MAX_RADIUS):
    """The scripts' chain for one image [H, W]:

        morph   = ImageMorphology(im, scale=16)
        new_img = np.float32(SetThickness(th)(morph))
        new_img = morph.downscale(np.float32(SetSlant(sl)(ImageMorphology(new_img))))
        cur     = np.median(new_img[new_img >= mn + (mx - mn) * .5])
        new_img = np.clip(new_img * (in_ / cur), 0, 255)

    ``thickness`` / ``slant`` / ``intensity`` of None: radius 0 / delta 0 / no rescale.  Returns a dict: ``image`` [H, W]
    in 0 .. 255 and the intermediates -- ``thickness`` (measured), ``radius`` (signed), ``reshaped`` (the bitmap before
    the shear), ``sums`` (its six integer moment sums), ``shear`` (its u11 / u02), ``shifts`` [H s], ``warped``, ``raw``
    (255 * reduce), ``quantised``, ``median``, ``status``: 0, or 1 (no background) / 2 (thinning) as ``ImageMorphology``
    has them, 3 for a radius above ``max_radius``, 4 when nothing is left to work with (no skeleton, erosion removed
    every pixel, every pixel in one row, or the quantised image is 0 everywhere).  A non-zero status: ``image`` is 0."""
    image = np.asarray(image, dtype=dtype)
    H, W = image.shape
    morph = ImageMorphology(image, threshold, scale, seed, dtype)
    return continue_from(morph.binary_image, morph.mean_thickness, H, W, thickness,
                         None if slant is None else -np.tan(np.float64(slant)), intensity, scale, morph.status, dtype,
                         max_radius)


# ------------------------------------------------------------ the local perturbations: thin, thick, swell, fracture
KINDS = ("plain", "thin", "thick", "swell", "fracture")              # the five Morpho-MNIST data sets, by kind number
PLAIN, THIN, THICK, SWELL, FRACTURE = range(5)
RADIUS_LIMIT = 2 ** 15           # a disk radius is held to this (its square exceeds every d2 of a 512 x 512 image)
ANGLE_WINDOW, FRAC_EXTENSION = 2, .5                                 # the reference's ``Fracture`` constants


def disk_radius(thickness, amount, scale):
    """``Thinning`` / ``Thickening``'s radius in fp64 from the thickness as given: int(amount * scale * thickness / 2),
    held to RADIUS_LIMIT.  None for a NaN."""
    v = np.float64(amount) * np.float64(scale) * np.float64(thickness) / np.float64(2)
    return None if np.isnan(v) else int(min(v, np.float64(RADIUS_LIMIT)))


def swelling_radius(thickness, radius, scale):
    """R = (radius * sqrt(thickness) / 2) * scale in fp64 from the thickness as given"""
    return (np.float64(radius) * np.sqrt(np.float64(thickness)) / np.float64(2)) * np.float64(scale)


def swell(bitmap, centre, R, strength=3):
    """The radial warp: output pixel (y, x) reads column floor(cx + w dx + 0.5) and row floor(cy + w dy + 0.5), dx = x -
    cx, dy = y - cy, w = (d2 / R^2) ** ((strength - 1) / 2) where d2 = dx^2 + dy^2 <= R^2 and 1 beyond; nearest
    neighbour, 0 outside the image.  fp64, every operation rounded once; an exponent of 1 takes no ``pow``.
    Returns (bool [H, W], the source coordinates before the floor: float64 [2, H, W] = row, column)."""
    bitmap = np.asarray(bitmap, dtype=bool)
    H, W = bitmap.shape
    cy, cx = int(centre[0]), int(centre[1])
    y, x = np.mgrid[:H, :W]
    dy, dx = (y - cy).astype(np.float64), (x - cx).astype(np.float64)
    d2 = ((y - cy) ** 2 + (x - cx) ** 2).astype(np.float64)
    RR = np.float64(R) * np.float64(R)
    e = (np.float64(strength) - np.float64(1)) / np.float64(2)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = d2 / RR
        w = np.where(d2 > RR, np.float64(1), q if e == 1 else np.power(q, e))
    fy, fx = np.float64(cy) + w * dy + np.float64(.5), np.float64(cx) + w * dx + np.float64(.5)
    sy, sx = np.floor(fy), np.floor(fx)
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    src = bitmap[np.clip(sy, 0, H - 1).astype(np.int64), np.clip(sx, 0, W - 1).astype(np.int64)]
    return inside & src, np.stack([fy, fx])


def line(p0, p1):
    """The digital line from p0 to p1, both (row, column) and both included: int64 [m + 1, 2], m = max(|dr|, |dc|).
    Pixel t has major coordinate major0 + sign * t (the major axis is the row when |dr| > |dc|, else the column) and
    minor coordinate minor0 + sign * ((2 t |dminor| + m) // (2 m)), in integers."""
    r0, c0, r1, c1 = int(p0[0]), int(p0[1]), int(p1[0]), int(p1[1])
    dr, dc = r1 - r0, c1 - c0
    m = max(abs(dr), abs(dc))
    if m == 0:
        return np.array([[r0, c0]], dtype=np.int64)
    t = np.arange(m + 1, dtype=np.int64)
    sr, sc = (dr > 0) - (dr < 0), (dc > 0) - (dc < 0)
    if abs(dr) > abs(dc):
        rows, cols = r0 + sr * t, c0 + sc * ((2 * t * abs(dc) + m) // (2 * m))
    else:
        rows, cols = r0 + sr * ((2 * t * abs(dr) + m) // (2 * m)), c0 + sc * t
    return np.stack([rows, cols], axis=1)


def fracture_radius(thickness, scale):
    """the brush radius of ``Fracture``: max(ceil((thickness * scale - 1) / 2), 0)"""
    return max(int(np.ceil((np.float64(thickness) * np.float64(scale) - 1) / 2)), 0)


def fracture_endpoints(skeleton, d2, centre, scale):
    """(r0, c0, r1, c1): the ends of the cut through ``centre``, perpendicular to the skeleton's local direction, as long
    as the stroke is wide there plus FRAC_EXTENSION * scale to either side; truncated toward zero"""
    from .skeleton import direction, window_sums
    i, j = int(centre[0]), int(centre[1])
    c, s = direction(window_sums(skeleton, i, j, ANGLE_WINDOW * int(scale)))
    L = np.sqrt(np.float64(d2[i, j])) + np.float64(FRAC_EXTENSION * int(scale))
    nr, nc = L * c, -(L * s)
    fi, fj = np.float64(i), np.float64(j)
    return tuple(int(np.trunc(v)) for v in (fi + nr, fj + nc, fi - nr, fj - nc))


def cut(bitmap, lines, r):
    """``bitmap`` without the pixels within squared distance r^2 of a pixel of one of ``lines`` (each [n, 2], inside the
    image or not)"""
    out = np.asarray(bitmap, dtype=bool).copy()
    H, W = out.shape
    r = int(r)
    for pixels in lines:
        for i, j in np.asarray(pixels).tolist():
            lo_i, hi_i, lo_j, hi_j = max(i - r, 0), min(i + r + 1, H), max(j - r, 0), min(j + r + 1, W)
            if lo_i >= hi_i or lo_j >= hi_j:
                continue
            y, x = np.mgrid[lo_i:hi_i, lo_j:hi_j]
            out[lo_i:hi_i, lo_j:hi_j] &= (y - i) ** 2 + (x - j) ** 2 > r * r
    return out


class Swelling(Perturbation):
    """A local swelling at a location drawn along the (unpruned) skeleton: the radial power warp of ``swell`` with R =
    ``swelling_radius(thickness, radius, scale)``.  ``centre``: use this (row, column) instead of drawing."""

    def __init__(self, strength=3, radius=7):
        if not strength >= 1:
            raise ValueError("Swelling: strength >= 1")
        self.strength, self.radius = strength, radius

    def __call__(self, morph, seed=0, counter=0, row=0, centre=None):
        from .skeleton import LocationSampler
        if centre is None:
            centre = LocationSampler().sample(morph, None, seed, counter, row)
        R = swelling_radius(morph.mean_thickness, self.radius, morph.scale)
        return swell(morph.binary_image, centre, R, self.strength)[0]


class Fracture(Perturbation):
    """``num_frac`` cuts across the stroke at locations drawn along the skeleton away from its tips and forks (from the
    whole skeleton if that leaves none), each perpendicular to the skeleton's local direction.  ``centres``: use these
    [n, 2] (row, column) instead of drawing."""

    def __init__(self, thickness=1.5, prune=2, num_frac=3):
        from ali_hip.rng import MAX_DRAWS
        if not 1 <= int(num_frac) <= MAX_DRAWS:
            raise ValueError(f"Fracture: num_frac in 1 .. {MAX_DRAWS}")
        self.thickness, self.prune, self.num_frac = thickness, prune, int(num_frac)

    def centres(self, morph, seed=0, counter=0, row=0):
        """(centres int64 [num_frac, 2], candidates drawn from, fallback)"""
        from .skeleton import LocationSampler
        for fallback, sampler in enumerate((LocationSampler(self.prune, self.prune), LocationSampler())):
            n = int(sampler.candidates(morph).sum())
            if n:
                return sampler.sample(morph, self.num_frac, seed, counter, row), n, fallback
        raise ValueError("Overpruned skeleton")

    def __call__(self, morph, seed=0, counter=0, row=0, centres=None):
        if centres is None:
            centres = self.centres(morph, seed, counter, row)[0]
        ends = [fracture_endpoints(morph.skeleton, morph.squared_distance, c, morph.scale) for c in centres]
        return cut(morph.binary_image, [line(e[:2], e[2:]) for e in ends], fracture_radius(self.thickness, morph.scale))


class _Given:
    """what a perturbation reads of an ``ImageMorphology``, from given intermediates (the thickness in fp64)"""

    def __init__(self, binary, d2, skeleton, thickness, scale):
        self.binary_image, self.skeleton = np.asarray(binary, dtype=bool), np.asarray(skeleton, dtype=bool)
        self.squared_distance = None if d2 is None else np.asarray(d2, dtype=np.int64)
        self.mean_thickness, self.scale = np.float64(thickness), int(scale)


def local_continue_from(binary, d2, skeleton, thickness, kind, H, W, scale=16, status=OK, dtype=np.float64, seed=0,
                        counter=0, row=0, thin_amount=.7, thick_amount=1., swell_strength=3., swell_radius=7.,
                        frac_thickness=1.5, frac_prune=2., num_frac=3):
    """The chain of ``local_image`` from a binary image [H s, W s], its squared distance map, skeleton and measured
    thickness on (the tests hand it the device's own): the dict of ``local_image``."""
    from ali_hip.rng import MAX_DRAWS
    if isinstance(kind, str) and kind not in KINDS:
        raise ValueError(f"local: kind is one of {KINDS} or a kind number")
    kind = KINDS.index(kind) if isinstance(kind, str) else int(kind)     # (a number that is no kind: status 4)
    Hh, Wh = H * scale, W * scale
    out = dict(bitmap=np.zeros((Hh, Wh), dtype=bool), raw=np.zeros((H, W), dtype=dtype),
               image=np.zeros((H, W), dtype=dtype), thickness=thickness, radius=0, n_candidates=0, fallback=0,
               centres=np.full((MAX_DRAWS, 2), -1, dtype=np.int64), endpoints=np.zeros((MAX_DRAWS, 4), dtype=np.int64),
               status=int(status))
    if status:
        return out
    m = _Given(binary, d2, skeleton, thickness, scale)
    nan = bool(np.isnan(m.mean_thickness))
    result = None
    if kind == PLAIN:
        result = m.binary_image
    elif kind in (THIN, THICK):
        if not nan:
            op = Thinning(thin_amount) if kind == THIN else Thickening(thick_amount)
            out["radius"] = disk_radius(thickness, op.amount, scale)
            result = op(m)
    elif kind == SWELL:
        from .skeleton import LocationSampler
        out["n_candidates"] = n = int(m.skeleton.sum())
        if n:
            out["centres"][0] = centre = LocationSampler().sample(m, None, seed, counter, row)
            if not nan:
                op = Swelling(swell_strength, swell_radius)
                out["radius"] = int(min(swelling_radius(thickness, swell_radius, scale), np.float64(RADIUS_LIMIT)))
                result = op(m, centre=centre)
    elif kind == FRACTURE:
        op = Fracture(frac_thickness, frac_prune, num_frac)
        if m.skeleton.any():
            centres, out["n_candidates"], out["fallback"] = op.centres(m, seed, counter, row)
            out["centres"][:op.num_frac] = centres
            out["endpoints"][:op.num_frac] = [fracture_endpoints(m.skeleton, m.squared_distance, c, scale)
                                              for c in centres]
            out["radius"] = fracture_radius(frac_thickness, scale)
            result = op(m, centres=centres)
    if result is None or not result.any():
        out["status"] = NOTHING_LEFT
        return out
    out["bitmap"] = result
    out["raw"] = dtype(255) * reduce(result, scale, dtype)
    out["image"] = quantise_levels(out["raw"])
    return out


def local_image(image, kind, scale=16, threshold=.5, seed=0, dtype=np.float64, counter=0, row=0, **params):
    """One image [H, W] through one of the five Morpho-MNIST data sets' perturbations (``kind``: a name of KINDS or its
    number) and ``morph.downscale``.  Returns a dict: ``bitmap`` (the perturbed hi-res image), ``image`` [H, W] in 0 ..
    255 (= ``morph.downscale(bitmap)``) and ``raw`` (255 * reduce, before the quantiser), ``thickness`` (measured),
    ``radius`` (the disk radius of thin / thick / fracture, int(R) of a swelling, 0 for plain), ``n_candidates`` (the
    skeleton pixels the locations were drawn from; 0 for plain / thin / thick), ``fallback`` (1: pruning left none, the
    whole skeleton was used), ``centres`` int64 [8, 2] (-1 where unused), ``endpoints`` int64 [8, 4] = r0, c0, r1, c1 (0
    where unused), ``status``: 0, or 1 / 2 as ``ImageMorphology`` has them, or 4 when nothing is left -- no skeleton for
    any kind but plain, or an empty result.  A non-zero status: ``bitmap`` and ``image`` are 0.  ``params``: those of
    ``local_continue_from``.  The draws are those of image ``row`` under (seed, counter)."""
    image = np.asarray(image, dtype=dtype)
    H, W = image.shape
    morph = ImageMorphology(image, threshold, scale, seed, dtype)
    return local_continue_from(morph.binary_image, morph.squared_distance, morph.skeleton, morph.mean_thickness, kind, H,
                               W, scale, morph.status, dtype, seed, counter, row, **params)


# --------------------------------------------------------------------------------------------------- SetWidth
WIDTH_TOLERANCE = 1.             # the reference's ``SetWidth._tolerance``, in pixels of the low-resolution image
WIDTH_MAX_DEPTH = 4              # re-applications ``SetWidth(validate=True)`` makes at most (the reference: unbounded)


class SumMoments:
    """what ``bounding_parallelogram`` reads of an ``ImageMoments``, formed from a bitmap's six integer sums as
    ``horizontal_shear`` forms them: ``centroid`` = (sx / n, sy / n), ``horizontal_shear`` = u11 / u02 -- the bits of
    ``ImageMoments(bitmap)``"""

    def __init__(self, sums):
        with np.errstate(invalid="ignore", divide="ignore"):
            self.horizontal_shear, cy = horizontal_shear(sums)
            self.centroid = (np.float64(sums[1]) / np.float64(sums[0]), cy)


def measure_width(morph, frac=.02, moments=None):
    """The reference's ``_measure_width``: (right - left) / morph.scale of the bounding parallelogram of the grey
    up-sampled image, ``moments`` (any object with ``centroid`` and ``horizontal_shear``; None: the image's own)
    giving the shear and the middle row of the horizontal cdf.  The up-sampled image is expand(image - image.min(),
    scale), DESIGN 3.21's rule: for an image whose minimum is 0 it is the reference's ``morph.hires_image`` (the same
    deviation, for the same reason: an image in -1 .. 1 and the same image in 0 .. 255 measure alike).  The reference
    subtracts the two top corners' x, which carry the same offset shear * (top - middle); the difference is taken of
    left and right themselves here."""
    image = np.asarray(morph.image, dtype=morph.dtype)
    hires = expand(image - image.min(), morph.scale, morph.dtype)
    left, right = bounds_of(hires, frac, moments)[:2]
    return (right - left) / morph.scale


def affine_columns(a, k, cx, cy, Hh, Wh):
    """int64 [Hh, Wh]: floor(((cx + a * (x - cx)) + k * (y - cy)) + 0.5) held to -1 .. Wh, in fp64 with every operation
    rounded on its own and in this order:

        dx = x - cx;  p = a * dx;  u = cx + p;          (by column)
        dy = y - cy;  v = k * dy;                       (by row)
        w = u + v;  z = w + 0.5;  f = floor(z);  column = min(max(f, -1), Wh)     (a NaN: -1)

    -1 and Wh both lie outside the image.  The row read is y itself."""
    a, k, cx, cy = (np.float64(v) for v in (a, k, cx, cy))
    with np.errstate(invalid="ignore", over="ignore"):
        u = cx + a * (np.arange(Wh, dtype=np.float64) - cx)
        v = k * (np.arange(Hh, dtype=np.float64) - cy)
        f = np.floor((u[None, :] + v[:, None]) + np.float64(0.5))
        f = np.where(f == f, np.minimum(np.maximum(f, -1.0), np.float64(Wh)), -1.0)
    return f.astype(np.int64)


def width_columns(factor, shear, cx, cy, Hh, Wh):
    """int64 [Hh, Wh]: the source column of output pixel (y, x) under ``SetWidth``'s matrix [[factor, shear * (1 -
    factor)], [0, 1]] about the centroid (cx, cy) -- ``LinearDeformation.warp`` followed by the rounding of a nearest
    neighbour warp: floor(((cx + factor * (x - cx)) + (shear * (1 - factor)) * (y - cy)) + 0.5), held to -1 .. Wh
    before the conversion.  Order of operations, each rounded to fp64 on its own, none fused:

        g = 1 - factor;  k = shear * g;  then ``affine_columns(factor, k, cx, cy, Hh, Wh)``.

    factor = source width / target width: a factor above 1 reads farther from the centroid, so the digit narrows."""
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.float64(shear) * (np.float64(1) - np.float64(factor))
    return affine_columns(factor, k, cx, cy, Hh, Wh)


def read_columns(bitmap, columns):
    """out(y, x) = bitmap(y, columns[y, x]), 0 where the column lies outside the image"""
    bitmap = np.asarray(bitmap, dtype=bool)
    H, W = bitmap.shape
    inside = (columns >= 0) & (columns < W)
    return inside & bitmap[np.arange(H)[:, None], np.clip(columns, 0, W - 1)]


class SetWidth(Perturbation):
    """``transform.warp`` of the boolean image under the horizontal scaling about its centroid that brings its
    measured width to the target and keeps its shear: nearest neighbour, constant 0 (``width_columns``).
    ``validate``: the reference's check -- the result is brought down, its width measured under its own grey moments,
    and when that is more than ``WIDTH_TOLERANCE`` from the target the reference's message is printed and the
    perturbation applied once more to the morphology of the downscaled result.  The reference recurses without a
    bound; here at most ``WIDTH_MAX_DEPTH`` re-applications are made (``depth`` counts them)."""

    _tolerance = WIDTH_TOLERANCE

    def __init__(self, target_width, validate=False):
        self.target_width = target_width
        self._validate = validate

    def __call__(self, morph, depth=0):
        binary = np.asarray(morph.binary_image, dtype=bool)
        sums = moment_sums(binary)
        moments = SumMoments(sums)
        with np.errstate(invalid="ignore", divide="ignore"):
            factor = measure_width(morph, moments=moments) / np.float64(self.target_width)
        warped = read_columns(binary, width_columns(factor, moments.horizontal_shear, *moments.centroid, *binary.shape))
        if self._validate and depth < WIDTH_MAX_DEPTH:
            pert_morph = ImageMorphology(morph.downscale(warped), morph.threshold, morph.scale, morph.seed, morph.dtype)
            width = measure_width(pert_morph)
            if abs(width - self.target_width) > self._tolerance:
                print(f"!!! Incorrect width after transformation: {width:.1f}, expected {self.target_width:.1f}.")
                warped = self(pert_morph, depth + 1)
        return warped


WIDTH_VALUES = ("left", "right", "shear", "cx", "cy", "factor")      # the six fp64 values ``ali_morpho_width`` leaves


def width_stage(binary, hires, target_width, scale, frac=.02, status=OK):
    """The measuring half of ``SetWidth`` with its corners, as ``ali_morpho_width`` has it.  ``binary``: the bitmap [H s,
    W s]; ``hires``: expand(image - image.min(), scale); ``status``: 0, or 1 for a bitmap without background.  Returns a
    dict: ``sums`` (the bitmap's six integer moment sums), ``shear``, ``cx``, ``cy`` (of the sums, as
    ``horizontal_shear`` forms them), ``left``, ``right`` (``bounds_of`` under that shear and cy), ``source_width`` =
    (right - left) / scale, ``factor`` = source_width / target_width, ``hcdf`` and ``status``, decided in this order: the
    status given; 5 for a target that is NaN, infinite or <= 0; 4 for an empty bitmap or one with every set pixel in one
    row; 4 for a grey mass <= 0 or a width that is not finite or <= 0.  With a status the sums are 0 and the floats
    NaN."""
    nan = np.float64("nan")
    out = dict(sums=np.zeros(6, dtype=np.int64), shear=nan, cx=nan, cy=nan, left=nan, right=nan, source_width=nan,
               factor=nan, hcdf=None, status=int(status))
    if status:
        return out
    target = np.float64(target_width)
    if not (target > 0 and np.isfinite(target)):
        out["status"] = BAD_TARGET
        return out
    sums = moment_sums(binary)
    if sums[0] == 0 or one_row(sums):
        out["status"] = NOTHING_LEFT
        return out
    moments = SumMoments(sums)
    left, right, _, _, shear, cy, hcdf, _ = bounds_of(hires, frac, moments)
    out["hcdf"] = hcdf
    with np.errstate(invalid="ignore"):
        width = (right - left) / np.float64(scale)
    if not (np.isfinite(width) and width > 0):                      # (a mass <= 0 makes left and right NaN)
        out["status"] = NOTHING_LEFT
        return out
    with np.errstate(over="ignore"):                                 # (a denormal target: the factor is infinite)
        factor = width / target
    out.update(sums=sums, shear=shear, cx=moments.centroid[0], cy=cy, left=left, right=right, source_width=width,
               factor=factor)
    return out


def affine_stage(binary, factor, shear, cx, cy, scale, dtype=np.float64):
    """The warp of ``SetWidth`` and the reduce of a bitmap with status 0, as ``ali_morpho_affine_reduce`` has them:
    (warped bitmap, raw = 255 * reduce in ``dtype``, quantised)"""
    warped = read_columns(binary, width_columns(factor, shear, cx, cy, *np.shape(binary)))
    raw = dtype(255) * reduce(warped, scale, dtype)
    return warped, raw, quantise_levels(raw)


def width_continue_from(binary, hires, H, W, target_width, target_intensity=None, scale=16, status=OK,
                        dtype=np.float64, frac=.02):
    """The chain of ``width_image`` from a binary image [H s, W s] and the grey up-sampled image on (the tests hand it
    the device's own bitmap): the dict of ``width_image``."""
    Hh, Wh = H * scale, W * scale
    out = width_stage(binary, hires, target_width, scale, frac, status)
    out.update(warped=np.zeros((Hh, Wh), dtype=bool), raw=np.zeros((H, W), dtype=dtype),
               quantised=np.zeros((H, W), dtype=dtype), median=dtype("nan"), image=np.zeros((H, W), dtype=dtype))
    if out["status"]:
        return out
    out["warped"], out["raw"], q = affine_stage(binary, out["factor"], out["shear"], out["cx"], out["cy"], scale, dtype)
    if q.max() == 0:
        out["status"] = NOTHING_LEFT
        return out
    out["quantised"] = q
    out["image"], out["median"] = set_intensity(q, target_intensity, dtype)
    return out


def width_image(image, width, intensity=None, scale=16, threshold=.5, dtype=np.float64, frac=.02, validate=False):
    """``SetWidth(width)`` and ``morph.downscale`` for one image [H, W], then the scripts' intensity rescale when
    ``intensity`` is given:

        bitmap, sums -> shear, cx, cy -> left, right -> source_width, factor -> warped -> raw = 255 * reduce ->
        quantised -> image

    Returns a dict with all of these (``width_stage``'s keys, ``binary``, ``warped``, ``raw``, ``quantised``, ``median``,
    ``image`` [H, W] in 0 .. 255) and ``status``: 0; 1: the bitmap has no background; 4 (NOTHING_LEFT): the bitmap is
    empty, every set pixel lies in one row, the grey mass is <= 0, the measured width is not finite or <= 0, or the
    quantised image is 0 everywhere; 5 (BAD_TARGET): the target is NaN, infinite or <= 0.  A non-zero status: ``image``
    is 0.  ``validate``: ``width_after`` (the width of ``quantised`` under its own grey moments, ``measure_bounds``)
    and ``off_target`` (|width_after - width| > WIDTH_TOLERANCE) are added, and an image that is off target is put
    through the chain once more, from ``quantised``, exactly once (what ``MorphoPerturb.set_width`` does; the class
    ``SetWidth`` recurses as the reference does); ``first`` then holds the first round's dict."""
    image = np.asarray(image, dtype=dtype)
    H, W = image.shape
    hires = expand(image, scale, dtype)
    binary = np.ones(hires.shape, dtype=bool) if image.max() == image.min() else binarise(hires, threshold)
    grey = expand(image - image.min(), scale, dtype)
    out = width_continue_from(binary, grey, H, W, width, None if validate else intensity, scale, int(binary.all()),
                              dtype, frac)
    out["binary"] = binary
    if not validate:
        return out
    with np.errstate(invalid="ignore", divide="ignore"):
        after = measure_bounds(out["quantised"], scale, frac, dtype)["width"]
        off = bool(abs(after - np.float64(width)) > WIDTH_TOLERANCE)
    if off:
        first, out = out, width_image(out["quantised"], width, None, scale, threshold, dtype, frac)
        out["first"] = first
    out["width_after"], out["off_target"] = after, off
    if not out["status"]:
        out["image"], out["median"] = set_intensity(out["quantised"], intensity, dtype)
    return out
