"""The statement of ``SetWidth`` on the CPU (``morphomnist.perturb``: ``width_columns``, ``measure_width``,
``SetWidth``, ``width_stage`` / ``width_continue_from`` / ``width_image``): the source columns against a
per-pixel loop in Python floats, the identity and ``SetSlant``'s matrix, bars widened and narrowed, the reference's
validation, the status corners, and ``ali_hip.morpho.MorphoPerturb.set_width`` on CPU tensors against ``width_image``."""
import math

import numpy as np
import pytest
import torch

import morpho_cases as mc

BAR = 8                          # the bars' width: the targets 2 w = 16 and w / 2 = 4 are whole pixels, and bar and
                                 # results lie centred and whole inside 28 x 28


def _m():
    from morphomnist import morpho
    return morpho


def _p():
    from morphomnist import perturb
    return perturb


def _morph(image, s, binary=None):
    return _m().ImageMorphology(np.asarray(image, dtype=np.float64), scale=s, binary=binary)


_MORPHS = {}


def bar_morph(s, w=BAR):
    if (s, w) not in _MORPHS:
        _MORPHS[s, w] = _morph(255 * mc.bar(w), s)
    return _MORPHS[s, w]


# ------------------------------------------------------------------------------------------------------- the columns
def _loop_columns(factor, shear, cx, cy, Hh, Wh):
    """``width_columns`` pixel by pixel in Python floats (IEEE doubles, one rounding per operation)"""
    out = np.empty((Hh, Wh), dtype=np.int64)
    k = shear * (1.0 - factor)
    for y in range(Hh):
        for x in range(Wh):
            z = ((cx + factor * (float(x) - cx)) + k * (float(y) - cy)) + 0.5
            out[y, x] = -1 if z != z else min(max(math.floor(z), -1), Wh) if math.isfinite(z) else (-1 if z < 0 else Wh)
    return out


@pytest.mark.parametrize("factor,shear,cx,cy,Hh,Wh", [
    (0.5, 0.0, 9.5, 6.25, 13, 20), (2.0, 0.3, 10.1, 5.7, 12, 23), (1.37, -0.81, 31.3, 40.9, 70, 65),
    (0.731, 1.9, 3.3, 8.8, 20, 9), (1e6, 0.2, 7.4, 3.1, 8, 16), (1e-6, -0.4, 7.4, 3.1, 8, 16),
    (float("inf"), 0.25, 7.4, 3.1, 8, 16), (float("inf"), 0.0, 7.0, 3.0, 8, 16), (float("nan"), 0.1, 7.4, 3.1, 5, 6)])
def test_width_columns_against_a_pixel_loop(factor, shear, cx, cy, Hh, Wh):
    p = _p()
    got = p.width_columns(factor, shear, cx, cy, Hh, Wh)
    assert got.dtype == np.int64 and got.shape == (Hh, Wh)
    assert np.array_equal(got, _loop_columns(factor, shear, cx, cy, Hh, Wh))
    assert got.min() >= -1 and got.max() <= Wh


def test_factor_one_is_the_identity():
    p = _p()
    bitmap = mc.blobs(37, 70, 3)
    for shear, cx, cy in ((0.0, 30.2, 17.7), (0.83, 35.0, 18.0), (-2.4, 1.9, 30.1)):
        cols = p.width_columns(1.0, shear, cx, cy, 37, 70)
        assert np.array_equal(cols, np.broadcast_to(np.arange(70), (37, 70)))
        assert np.array_equal(p.read_columns(bitmap, cols), bitmap)


@pytest.mark.parametrize("delta", [0.31, -0.31, 0.9, -1.7, 0.0])
def test_the_matrix_of_set_slant_reproduces_its_row_shifts(delta):
    """factor 1 with the off-diagonal entry -delta is ``SetSlant``'s matrix: the columns are x + shift(y)"""
    p = _p()
    bitmap = mc.blobs(41, 70, 5)
    sums = p.moment_sums(bitmap)
    _, cy = p.horizontal_shear(sums)
    cx = np.float64(sums[1]) / np.float64(sums[0])
    cols = p.affine_columns(1.0, -delta, cx, cy, 41, 70)
    assert np.array_equal(p.read_columns(bitmap, cols), p.shift_rows(bitmap, p.shear_shifts(delta, cy, 41, 70)))


# ----------------------------------------------------------------------------------------------------------- the bars
@pytest.mark.parametrize("s", [4, 16])
@pytest.mark.parametrize("ratio", [2.0, 0.5])
def test_a_bar_widened_and_narrowed(s, ratio):
    """an upright bar of width 8 brought to 16 and to 4: the width measured on the downscaled result is within the
    reference's tolerance of 1 pixel of the target, and the result stays upright"""
    p, m = _p(), _m()
    morph = bar_morph(s)
    target = BAR * ratio
    out = p.SetWidth(target)(morph)
    assert out.dtype == bool and out.shape == (28 * s, 28 * s)
    after = m.measure_bounds(morph.downscale(out), s, .02)["width"]
    print(f"bar {BAR} -> {target} at s={s}: measured {p.measure_width(morph):.3f} before, {after:.3f} after")
    assert abs(after - target) <= p.WIDTH_TOLERANCE
    rows = out.any(1)
    assert np.array_equal(rows, morph.binary_image.any(1))           # the rows are read in place
    runs = out[rows].sum(1)
    assert runs.min() >= 1 and abs(p.horizontal_shear(p.moment_sums(out))[0]) <= 1 / rows.sum()


@pytest.mark.parametrize("s", [4, 16])
@pytest.mark.parametrize("ratio", [2.0, 0.5])
def test_a_sheared_bar_keeps_its_shear(s, ratio):
    """a bar built on the up-sampled grid along the line x = c + shear (y - cy): every row of the result is one run whose
    middle lies within one column of that line (nearest neighbour moves a run's ends by at most 1 / (2 factor) <= 1
    column each), and u11 / u02 moves by less than one column over half the bar's height"""
    p, m = _p(), _m()
    Hh = Wh = 28 * s
    shear, half = 0.35, 4 * s
    y, x = np.mgrid[:Hh, :Wh]
    line = Wh / 2 + shear * (y - Hh / 2)
    bitmap = (np.abs(x + .5 - line) <= half) & (y >= 6 * s) & (y < 22 * s)
    image = m.quantise(m.reduce(bitmap.astype(np.float64), s))
    morph = _morph(image, s, binary=bitmap)
    sums = p.moment_sums(bitmap)
    before, cy = p.horizontal_shear(sums)
    cx = sums[1] / sums[0]
    out = p.SetWidth(p.measure_width(morph, moments=p.SumMoments(sums)) * ratio)(morph)
    rows = np.nonzero(out.any(1))[0]
    assert np.array_equal(rows, np.arange(6 * s, 22 * s))
    for r in rows:
        cols = np.nonzero(out[r])[0]
        assert len(cols) == cols[-1] - cols[0] + 1, r               # one run
        assert abs((cols[0] + cols[-1]) / 2 - (cx + before * (r - cy))) <= 1, r
        assert abs(len(cols) - ratio * (2 * half)) <= 2, (r, len(cols))
    after = p.horizontal_shear(p.moment_sums(out))[0]
    assert abs(after - before) * (8 * s) < 1, (before, after)


def test_measure_width_is_the_width_column_of_measure_image():
    from morphomnist.measure import measure_image
    p = _p()
    for b, im in enumerate(mc.image_batch(4, 28, 28)):
        morph = _morph(255 * im, 4)
        assert p.measure_width(morph) == measure_image(255 * im, scale=4, verbose=False).width, b
    # ... and with the bitmap's moments it is the statement under them
    m = _m()
    morph = bar_morph(4)
    mom = p.SumMoments(p.moment_sums(morph.binary_image))
    assert mom.horizontal_shear == m.ImageMoments(morph.binary_image).horizontal_shear
    assert mom.centroid == m.ImageMoments(morph.binary_image).centroid
    left, right = m.bounds_of(m.expand(morph.image - morph.image.min(), 4), .02, mom)[:2]
    assert p.measure_width(morph, moments=mom) == (right - left) / 4


# -------------------------------------------------------------------------------------------------------- validation
def _first_round(w, target, s=4):
    p, m = _p(), _m()
    morph = bar_morph(s, w)
    first = p.SetWidth(target)(morph)
    pert = m.ImageMorphology(morph.downscale(first), morph.threshold, s, morph.seed, morph.dtype)
    return morph, first, pert, p.measure_width(pert)


def test_validate_reapplies_exactly_when_off_target(capsys):
    """a bar of 6 brought to 3 measures more than 1 pixel off (the blur of the downscaled result is a larger share of a
    narrow bar): the message is printed and the result is that of the perturbation applied to the downscaled first
    result; a bar of 8 brought to 4 is within 1: nothing is printed and the result is the first"""
    p = _p()
    morph, first, pert, width = _first_round(6, 3.0)
    assert abs(width - 3.0) > 1
    capsys.readouterr()
    got = p.SetWidth(3.0, validate=True)(morph)
    said = capsys.readouterr().out
    assert said.startswith(f"!!! Incorrect width after transformation: {width:.1f}, expected 3.0.")
    again = p.SetWidth(3.0, validate=True)(pert, depth=1)
    assert np.array_equal(got, again) and not np.array_equal(got, first)
    # at the depth limit nothing is measured any more
    capsys.readouterr()
    assert np.array_equal(p.SetWidth(3.0, validate=True)(morph, depth=p.WIDTH_MAX_DEPTH), first)
    assert capsys.readouterr().out == ""
    assert said.count("!!!") <= p.WIDTH_MAX_DEPTH

    morph, first, pert, width = _first_round(8, 4.0)
    assert abs(width - 4.0) <= 1
    assert np.array_equal(p.SetWidth(4.0, validate=True)(morph), first)
    assert capsys.readouterr().out == ""


def test_width_image_validates_once():
    p, m = _p(), _m()
    off = p.width_image(255 * mc.bar(6), 3.0, scale=4, validate=True)
    plain = p.width_image(255 * mc.bar(6), 3.0, scale=4)
    assert off["off_target"] and abs(off["width_after"] - 3.0) > 1
    assert off["width_after"] == m.measure_bounds(plain["image"], 4, .02)["width"]
    assert np.array_equal(off["first"]["quantised"], plain["image"])
    assert np.array_equal(off["image"], p.width_image(plain["image"], 3.0, scale=4)["image"])
    fine = p.width_image(255 * mc.bar(8), 4.0, scale=4, validate=True)
    assert not fine["off_target"] and "first" not in fine
    assert np.array_equal(fine["image"], p.width_image(255 * mc.bar(8), 4.0, scale=4)["image"])
    # the intensity rescale comes after the selection
    lit = p.width_image(255 * mc.bar(6), 3.0, 200.0, scale=4, validate=True)
    want, med = p.set_intensity(off["quantised"], 200.0)
    assert np.array_equal(lit["image"], want) and lit["median"] == med


# ------------------------------------------------------------------------------------------------------ status corners
def test_chain_intermediates():
    p, m = _p(), _m()
    im = 255 * mc.image_batch(1, 28, 28)[0]
    r = p.width_image(im, 7.5, 180.0, scale=4)
    assert r["status"] == 0
    morph = _morph(im, 4)
    assert np.array_equal(r["binary"], morph.binary_image)
    assert r["sums"].tolist() == p.moment_sums(r["binary"]).tolist()
    mom = m.ImageMoments(r["binary"])
    assert (r["shear"], r["cx"], r["cy"]) == (mom.horizontal_shear, mom.m10, mom.m01)
    assert r["source_width"] == p.measure_width(morph, moments=mom) == (r["right"] - r["left"]) / 4
    assert r["factor"] == r["source_width"] / 7.5
    assert np.array_equal(r["warped"], p.SetWidth(7.5)(morph))
    assert np.array_equal(r["raw"], 255.0 * m.reduce(r["warped"], 4))
    assert np.array_equal(r["quantised"], morph.downscale(r["warped"]))
    want, med = p.set_intensity(r["quantised"], 180.0)
    assert np.array_equal(r["image"], want) and r["median"] == med


def test_status_corners():
    p, m = _p(), _m()
    assert (p.OK, p.NO_BACKGROUND, p.NOTHING_LEFT, p.BAD_TARGET) == (0, 1, 4, 5)
    im = 255 * mc.image_batch(1, 28, 28)[0]

    def dead(r, status):
        assert r["status"] == status, (r["status"], status)
        assert not r["image"].any() and not r["quantised"].any() and r["image"].shape == (28, 28)
        return True

    assert dead(p.width_image(np.full((28, 28), 3.0), 6.0, scale=4), 1)              # no background
    assert dead(p.width_image(np.full((28, 28), 3.0), -6.0, scale=4), 1)             # ... comes before the target
    for bad in (0.0, -2.0, float("nan"), float("inf"), -float("inf")):
        r = p.width_image(im, bad, scale=4)
        assert dead(r, 5) and not r["sums"].any() and np.isnan(r["factor"])
    grey = m.expand(im, 4)
    binary = np.zeros((112, 112), dtype=bool)
    assert dead(p.width_continue_from(binary, grey, 28, 28, 6.0, scale=4), 4)        # an empty bitmap
    assert dead(p.width_continue_from(binary, grey, 28, 28, 0.0, scale=4), 5)        # ... comes after the target
    binary[50, 20:90] = True
    assert dead(p.width_continue_from(binary, grey, 28, 28, 6.0, scale=4), 4)        # one row
    binary[51, 20:90] = True
    assert p.width_continue_from(binary, grey, 28, 28, 6.0, scale=4)["status"] == 0
    assert dead(p.width_continue_from(binary, np.zeros_like(grey), 28, 28, 6.0, scale=4), 4)     # no grey mass
    assert dead(p.width_continue_from(binary, -grey, 28, 28, 6.0, scale=4), 4)
    assert dead(p.width_continue_from(binary, np.full_like(grey, np.nan), 28, 28, 6.0, scale=4), 4)   # a NaN width
    r = p.width_image(im, 1e-3, scale=4)                             # a factor of thousands: nothing left of the result
    assert dead(r, 4) and r["factor"] > 1000 and r["sums"][0] > 0
    assert dead(p.width_image(im, 1e-320, scale=4), 4)               # an infinite factor


# ---------------------------------------------------------------------------------------------------------- executor
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_set_width_on_cpu_tensors(dtype):
    from ali_hip.morpho import MorphoPerturb
    p = _p()
    npdt = np.float64 if dtype == torch.float64 else np.float32
    x = torch.from_numpy(mc.image_batch(5, 28, 28)).to(dtype)
    x[3] = 0.25                                                      # status 1
    width = torch.tensor([9.0, 6.0, 12.0, 5.0, 0.0], dtype=torch.float64)               # the last: status 5
    inten = torch.tensor([200.0, 120.0, 255.0, 90.0, 100.0], dtype=torch.float32)
    mp = MorphoPerturb(scale=4)
    for t_i in (None, inten):
        for validate in (False, True):
            got = mp.set_width(x[:, None], width, t_i, validate=validate)
            assert got["status"].tolist() == [0, 0, 0, 1, 5]
            for b in range(5):
                want = p.width_image(x[b].numpy(), width[b].item(), None if t_i is None else t_i[b].item(), 4, .5, npdt,
                                     .02, validate)
                first = want.get("first", want)
                assert np.array_equal(got["images"][b].numpy(), want["image"].astype(npdt)), (b, validate)
                for k, w in (("width_before", npdt(first["source_width"])), ("factor", first["factor"]),
                             ("shear_before", first["shear"]), ("intensity_before", npdt(want["median"]))):
                    assert np.array_equal(got[k][b].numpy(), w, equal_nan=True), (b, k)
                assert np.array_equal(got["bounds_before"][b].numpy(), [first["left"], first["right"]], equal_nan=True)
                if validate:
                    assert got["off_target"][b].item() == want["off_target"]
                    assert np.array_equal(got["width_after"][b].numpy(), npdt(want["width_after"]), equal_nan=True)
            assert got["images"].dtype == dtype and got["images"].shape == (5, 28, 28)
            assert ("width_after" in got) == validate


def test_refusals():
    from ali_hip.morpho import MorphoPerturb, width_image_bytes, width_scratch_bytes
    mp = MorphoPerturb(scale=4)
    x = torch.zeros(2, 28, 28)
    w = torch.ones(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="width"):
        mp.set_width(x, None)
    with pytest.raises(ValueError, match="width"):
        mp.set_width(x, torch.ones(3))
    with pytest.raises(ValueError, match="intensity"):
        mp.set_width(x, w, torch.ones(3))
    for frac in (0.0, 1.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="bound_frac"):
            mp.set_width(x, w, bound_frac=frac)
    with pytest.raises(ValueError, match="exceed the limit"):
        mp.set_width(torch.zeros(1, 129, 28), torch.ones(1))
    with pytest.raises(ValueError, match="float images"):
        mp.set_width(torch.zeros(2, 28, 28, dtype=torch.int32), w)
    # the chunk counts this chain's scratch: affine_reduce's fp64 T is the largest at 28 x 28, bounds' T at 32 x 32 x 16
    assert width_scratch_bytes(28, 28, 16) == 8 * 28 * 28 * 16 and width_scratch_bytes(28, 28, 1) == 0
    assert width_scratch_bytes(32, 32, 16) == 8 * 32 * 32 * 16
    assert width_image_bytes(28, 28, 16) > width_scratch_bytes(28, 28, 16) + 2 * 4 * 448 * 14
    assert MorphoPerturb(scale=16).width_chunk_for(28, 28) >= 1000 and MorphoPerturb(scale=16, chunk=7).width_chunk_for(28, 28) == 7
