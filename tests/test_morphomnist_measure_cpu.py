"""The bounding parallelogram and ``morphomnist.measure`` on the CPU: the statement against the
reference's loops written out here, the crossing rule of ``quantile_loc`` on a built image with two upward crossings,
synthetic cdfs, degenerate and affine-invariance cases, bars of known width, and ``measure_image`` /
``measure_batch`` / ``MorphoMeasure(bound_frac=...)`` on CPU tensors."""
import numpy as np
import pytest
import torch

import morpho_cases as mc


def _m():
    from morphomnist import morpho
    return morpho


# ------------------------------------------------------------------------------------------- the reference's loops
def _horz_cdf(img, shear, x, y, y_mid):
    locs = np.arange(0, img.shape[1], step=1)
    counts = np.zeros(len(locs))
    for i, t in enumerate(locs):
        counts[i] = ((x + .5 < t + shear * (y - y_mid)) * img).sum()
    return locs, counts / img.sum()


def _vert_cdf(img, y):
    counts = np.zeros(img.shape[0])
    for t in range(img.shape[0]):
        counts[t] = ((y < t) * img).sum()
    return counts / img.sum()


def _reference(img, frac):
    """(hcdf, vcdf, left, right, top, bottom) of the reference's bounding_parallelogram, np.interp and all"""
    from morphomnist.morpho import ImageMoments
    img = np.asarray(img, dtype=float)
    height, width = img.shape
    x = np.arange(width)[None, :]
    y = np.arange(height)[:, None]
    moments = ImageMoments(img)
    middle = moments.centroid[1]
    shear = moments.horizontal_shear
    hloc, hcdf = _horz_cdf(img, shear, x, y, middle)
    vcdf = _vert_cdf(img, y)
    frac /= 2
    left, right = np.interp([frac, 1. - frac], hcdf, hloc)
    top, bottom = np.interp([frac, 1. - frac], vcdf, np.arange(len(vcdf)))
    return hcdf, vcdf, left, right, top, bottom


def _crossings(c, f):
    """the intervals j where the cdf c crosses the level f upward; -1 and len(c) - 1 stand for f below the first entry
    and f at or above the last (c held at -inf before it and +inf after it)"""
    p = np.concatenate([[-np.inf], c, [np.inf]])
    return [j - 1 for j in range(len(p) - 1) if p[j] <= f < p[j + 1]]


@pytest.mark.parametrize("s,B", [(1, 70), (2, 70), (4, 70), (16, 3)])
def test_statement_against_the_reference_loops(s, B):
    """where every level is crossed upward exactly once, the statement is the reference bit for bit"""
    m = _m()
    frac = .02
    unique = 0
    for b, im in enumerate(mc.image_batch(B, 28, 28)):
        hires = m.expand(im - im.min(), s)
        want = _reference(hires, frac)
        got = m.bounds_of(hires, frac)
        hcdf, vcdf = want[0], want[1]
        once = all(len(_crossings(c, f)) == 1 for c in (hcdf, vcdf) for f in (frac / 2, 1 - frac / 2))
        unique += once
        assert once, (s, b, [len(_crossings(c, f)) for c in (hcdf, vcdf) for f in (frac / 2, 1 - frac / 2)])
        assert np.array_equal(got[6], hcdf) and np.array_equal(got[7], vcdf), (s, b)
        assert [float(v) for v in got[:4]] == [float(v) for v in want[2:]], (s, b, got[:4], want[2:])
    print(f"s={s}: {unique}/{B} rows crossed once at every level")


def _dot_and_bar():
    im = np.zeros((12, 16))
    im[2:10, 9:12] = 1
    im[5, 2] = 1
    return im


@pytest.mark.parametrize("frac,side,first,second,want", [(.072, "left", 6, 17, 6), (.002, "right", 24, 27, 27)])
def test_crossing_rule_on_a_built_image(frac, side, first, second, want):
    """the dot's ringing makes hcdf cross the level twice upward; left takes the first interval, right the last"""
    m = _m()
    hires = m.measure_bounds(_dot_and_bar(), 2, frac)["hires"]
    got = m.bounds_of(hires, frac)
    hcdf = got[6]
    f = frac / 2 if side == "left" else 1 - frac / 2
    hits = _crossings(hcdf, f)
    assert hits == [first, second], hits
    margin = min(min(abs(hcdf[j] - f), abs(hcdf[j + 1] - f)) for j in hits)
    print(f"frac {frac}: crossings {hits}, smallest margin {margin:.3g}")
    assert margin > 1e-5
    loc = got[0] if side == "left" else got[1]
    assert want <= loc < want + 1, loc
    slope = (np.float64(want + 1) - np.float64(want)) / (hcdf[want + 1] - hcdf[want])
    assert loc == slope * (f - hcdf[want]) + want


def test_quantile_loc_on_synthetic_cdfs():
    m = _m()
    ql = m.quantile_loc
    c = np.array([.1, .2, .2, .2, .5, 1.0])
    for side in ("left", "right"):
        assert ql(c, .05, side) == 0 and ql(c, 1.0, side) == 5 and ql(c, 2.0, side) == 5
        assert ql(c, .1, side) == 0                                  # f == c[0]: the first interval, at its start
        assert ql(c, .2, side) == 3                                  # the flat run: only [3, 4) holds .2 <= f < .5
        assert ql(c, .5, side) == 4                                  # f == c[j] exactly
        assert ql(c, .35, side) == np.interp(.35, c, np.arange(6)) == 3.5
    up = np.array([0., .5, .2, .6, 1.])
    assert ql(up, .3, "left") == np.interp(.3, up[:2], [0., 1.])    # the first upward crossing, j = 0
    assert ql(up, .3, "right") == 2 + .1 / .4                        # the last, j = 2
    g = np.random.default_rng(5)
    for _ in range(200):                                             # monotone: np.interp's bits
        c = np.sort(g.uniform(-.1, 1.1, size=g.integers(2, 40)))
        for f in g.uniform(-.2, 1.2, size=5):
            for side in ("left", "right"):
                assert ql(c, f, side) == np.interp(f, c, np.arange(len(c)))


def test_constant_image_is_nan():
    m = _m()
    for s in (1, 4):
        got = m.measure_bounds(np.full((9, 7), 0.3), s, .02)
        assert np.isnan(got["bounds"][:4]).all() and np.isnan(got["corners"]).all()
        assert np.isnan(got["width"]) and np.isnan(got["height"]) and np.isnan(got["slant"])


def test_affine_invariance():
    """0 .. 1, 0 .. 255 and the Generator's -1 .. 1: the same hires up to a factor, so the same width, height and slant to
    1e-9 relative.  Strokes of 24 x 24: at 28 x 28 the batch holds the symmetric bar and ring, whose slant is rounding
    noise of some 1e-15 with no relative precision in any of the three forms."""
    m = _m()
    g = mc.generator_images(6, 24, 24, seed=4).astype(np.float64)
    forms = [(g + 1) / 2, 255 * (g + 1) / 2, g]
    rows = [[m.measure_bounds(im, 4, .02) for im in form] for form in forms]
    for k in ("width", "height", "slant"):
        base = np.array([r[k] for r in rows[0]])
        assert np.isfinite(base).all() and (np.abs(base) > 1e-3).all(), (k, base)
        for other in rows[1:]:
            v = np.array([r[k] for r in other])
            assert np.allclose(v, base, rtol=1e-9, atol=0), (k, v, base)


@pytest.mark.parametrize("s", [4, 16])
def test_bars(s):
    m = _m()
    widths = []
    for w in (2, 3, 4):
        got = m.measure_bounds(mc.bar(w), s, .02)
        print(f"bar {w} at s={s}: width {got['width']:.4f}, height {got['height']:.4f}")
        assert abs(got["height"] - 16) <= .2 and abs(got["width"] - w) <= .6
        widths.append(got["width"])
    assert widths[0] < widths[1] < widths[2]


# ---------------------------------------------------------------------------------------------- measure_image, batch
def test_measure_image_fields_and_print(capsys):
    from morphomnist.measure import Morphometrics, measure_image
    assert Morphometrics._fields == ("area", "length", "thickness", "slant", "width", "height")
    im = mc.image_batch(1, 28, 28)[0]
    r = measure_image(im, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert out == [f"Area: {r.area:.1f}", f"Length: {r.length:.1f}", f"Thickness: {r.thickness:.2f}",
                   f"Slant: {np.rad2deg(r.slant):.0f}°", f"Dimensions: {r.width:.1f} x {r.height:.1f}"]
    m = _m()
    morph = m.ImageMorphology(im, .5, 4, 0)
    b = m.measure_bounds(im, 4, .02)
    assert tuple(r) == (morph.area, morph.stroke_length, morph.mean_thickness, b["slant"], b["width"], b["height"])
    measure_image(im, verbose=False)
    assert capsys.readouterr().out == ""


def test_measure_batch_pool_and_the_executor():
    from multiprocessing.pool import ThreadPool

    from ali_hip.morpho import MorphoMeasure
    from morphomnist.measure import measure_batch, measure_image
    ims = mc.image_batch(7, 20, 24, seed=3)
    seq = measure_batch(ims, scale=2)
    assert list(seq.columns) == ["area", "length", "thickness", "slant", "width", "height"] and len(seq) == 7
    with ThreadPool(2) as pool:
        par = measure_batch(ims, scale=2, pool=pool, chunksize=3)
    assert seq.equals(par)
    assert seq.equals(measure_batch(torch.from_numpy(ims), scale=2))
    rows = [measure_image(im, scale=2, verbose=False) for im in ims]
    assert np.array_equal(seq.to_numpy(), np.array(rows, dtype=np.float64), equal_nan=True)
    mm = MorphoMeasure(scale=2, bound_frac=.02)
    out = mm.measure(torch.from_numpy(ims))
    for k, j in (("area", 0), ("length", 1), ("thickness", 2), ("slant_measure", 3), ("width", 4), ("height", 5)):
        assert out[k].dtype == torch.float64
        assert np.array_equal(out[k].numpy(), np.array([r[j] for r in rows]), equal_nan=True), k
    m = _m()
    for b, im in enumerate(ims):
        want = m.measure_bounds(im, 2, .02)
        assert np.array_equal(out["bounds"][b].numpy(), want["bounds"])
        assert np.array_equal(out["corners"][b].numpy(), want["corners"])
    tab = mm.table()
    assert tab["bounds"].shape == (7, 6) and tab["corners"].shape == (7, 4, 2)
    assert np.array_equal(tab["width"], out["width"].numpy())
    plain = MorphoMeasure(scale=2).measure(torch.from_numpy(ims))
    assert set(plain) == {"area", "length", "thickness", "intensity", "slant", "slant_hires", "counts", "status"}
    for k in plain:
        assert torch.equal(plain[k], out[k]), k
    with pytest.raises(ValueError, match="bound_frac"):
        MorphoMeasure(bound_frac=1.0)
