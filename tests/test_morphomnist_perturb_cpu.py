"""The statement of the perturbation half, ``morphomnist.perturb`` and the reduce / quantise additions of
``morphomnist.morpho``, on the CPU: the operators, the guard of ``quantise``, the footprints against scipy's binary
morphology, ``SetSlant`` against a per-pixel loop, the status corners, and ``ali_hip.morpho.MorphoPerturb`` on CPU tensors
against ``counterfactual_image`` and the scripts' loop body."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import morpho_cases as mc
import perturb_cases as pc


def _m():
    from morphomnist import morpho
    return morpho


def _p():
    from morphomnist import perturb
    return perturb


# ---------------------------------------------------------------------------------------------------- reduce, quantise
@pytest.mark.parametrize("n,scale", [(28, 16), (28, 4), (5, 2), (9, 4), (7, 1)])
def test_reduce_operator(n, scale):
    m = _m()
    R = m.reduce_operator(n, scale)
    assert R.shape == (n, n * scale) and R.dtype == np.float64 and not R.flags.writeable
    assert np.abs(R.sum(1) - 1).max() <= 1e-14
    assert m.reduce_operator(n, scale) is R                          # cached
    if scale == 1:
        assert np.array_equal(R, np.eye(n))
    x = np.full((n, n + 1), 0.37)
    back = m.reduce(m.expand(x, scale) / (255 if scale > 1 else 1), scale)
    assert back.shape == x.shape and np.abs(back - 0.37).max() <= 1e-13


@pytest.mark.parametrize("H,W,scale", [(5, 9, 4), (7, 6, 2), (28, 28, 4)])
def test_reduce_is_the_2d_scipy_composition(H, W, scale):
    """``reduce`` = RH image RW^T against ``gaussian_filter`` then ``zoom`` of the whole image, as ``pyramid_reduce``
    composes them (both are separable), on a random non-square image: a transposed or mis-indexed operator with unit row
    sums would miss it.  Both sides are fp64 evaluations of one linear map, with weights of magnitude below 2 on pixels
    in 0 .. 1 over at most (H s)(W s) = 12 544 terms: n eps = 3e-12 bounds the rounding of either, and the bound is
    1e-11."""
    m = _m()
    x = np.random.default_rng(H * W + scale).random((H * scale, W * scale))
    want = ndimage.zoom(ndimage.gaussian_filter(x, 2 * scale / 6.0, mode="reflect"), (1 / scale, 1 / scale), order=3,
                        mode="mirror", grid_mode=True)
    got = m.reduce(x, scale)
    assert got.shape == want.shape == (H, W)
    print(f"reduce {H}x{W} s={scale}: max difference from the 2-D composition {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= 1e-11
    assert np.abs(m.reduce(x.T, scale) - want.T).max() <= 1e-11
    assert np.abs(got - want[::-1, ::-1]).max() > 1e-3               # (the image tells a flipped operator apart)


def test_quantise_plate_and_clamp():
    m = _m()
    plate = m.reduce(np.ones((448, 448), dtype=np.float32), 16, np.float32)
    assert plate.dtype == np.float32
    levels = np.float32(255) * plate
    assert levels.min() < 255                                       # the reason for the guard: 254.99997 occurs
    q = m.quantise(plate)
    assert q.dtype == np.float32 and (q == 255).all()
    assert (m.quantise(np.zeros((28, 28), dtype=np.float32)) == 0).all()
    assert m.quantise_levels(np.array([300., -3., 0., 254.99, 254.995, 17.5])).tolist() == [255, 0, 0, 254, 255, 17]
    assert m.quantise(np.array([300 / 255., -3 / 255.])).tolist() == [255, 0]
    morph = m.ImageMorphology(np.zeros((28, 28)), scale=16, binary=np.zeros((448, 448), dtype=bool))
    assert (morph.downscale(np.ones((448, 448))) == 255).all()
    one = m.ImageMorphology(mc.bar(3), scale=1)
    assert np.array_equal(one.downscale(mc.bar(3)), 255 * mc.bar(3))


# ---------------------------------------------------------------------------------------------------------- footprints
def test_footprints():
    p = _p()
    assert p.footprint(0).tolist() == [[True]]
    for r, n, n_disk in zip(pc.RADII, pc.SET_PIXELS, pc.DISK_PIXELS):
        f = p.footprint(r)
        assert f.shape == (2 * r + 1, 2 * r + 1) and f.dtype == bool
        assert int(f.sum()) == n and int(p.disk(r).sum()) == n_disk, (r, int(f.sum()))
        assert np.array_equal(f, f[::-1]) and np.array_equal(f, f[:, ::-1]) and np.array_equal(f, f.T)
        h = p.half_widths(r)                                         # (asserts one centred run per row, none empty)
        assert h.shape == (2 * r + 1,) and (h >= 0).all() and int((2 * h + 1).sum()) == n
    table = p.half_width_table(3)
    assert table.shape == (4, 7) and table.dtype == np.int16
    assert table[0].tolist() == [0] + [-1] * 6 and table[1].tolist() == [1, 1, 1] + [-1] * 4


@pytest.mark.parametrize("r", [0, 1, 4, 9])
def test_dilate_erode_against_scipy(r):
    p = _p()
    f = p.footprint(r)
    for name, b in mc.binary_cases(20, 36).items():
        assert np.array_equal(p.dilate(b, r), ndimage.binary_dilation(b, structure=f, border_value=0)), (name, r)
        assert np.array_equal(p.erode(b, r), ndimage.binary_erosion(b, structure=f, border_value=1)), (name, r)


def test_exact_disk_thinning_and_thickening():
    p, m = _p(), _m()
    morph = m.ImageMorphology(mc.stroke(seed=2), scale=4)
    for amount in (0.3, 0.7):
        r = int(amount * 4 * morph.mean_thickness / 2.)
        d = p.disk(r)
        assert np.array_equal(p.Thinning(amount)(morph), ndimage.binary_erosion(morph.binary_image, d, border_value=1))
        assert np.array_equal(p.Thickening(amount)(morph), ndimage.binary_dilation(morph.binary_image, d))


def test_set_thickness_is_nested():
    p, m = _p(), _m()
    morph = m.ImageMorphology(mc.stroke(seed=1), scale=4)
    t = float(morph.mean_thickness)
    maps = [p.SetThickness(t + d)(morph) for d in (-1.2, -0.6, 0.0, 0.7, 1.9)]
    assert np.array_equal(maps[2], morph.binary_image)
    for a, b in zip(maps, maps[1:]):
        assert not (a & ~b).any() and a.sum() < b.sum()


# ------------------------------------------------------------------------------------------------------------- SetSlant
def _warp_loop(binary, delta, cy):
    """nearest-neighbour warp of (x, y) -> (x - delta * (y - cy), y), pixel by pixel: rint with ties up"""
    H, W = binary.shape
    out = np.zeros_like(binary)
    for y in range(H):
        for x in range(W):
            src = int(np.floor(x - delta * (y - cy) + 0.5))
            if 0 <= src < W:
                out[y, x] = binary[y, src]
    return out


@pytest.mark.parametrize("slant", [0.0, 0.35, -0.8])
def test_set_slant_against_a_pixel_loop(slant):
    p, m = _p(), _m()
    binary = mc.blobs(24, 40, seed=4, fill=0.3)
    morph = m.ImageMorphology(binary.astype(float), scale=1, binary=binary)
    mo = m.ImageMoments(binary)
    delta = -np.tan(slant) - mo.horizontal_shear
    got = p.SetSlant(slant)(morph)
    assert got.dtype == bool and np.array_equal(got, _warp_loop(binary, delta, mo.m01))
    sums = p.moment_sums(binary)
    shear, cy = p.horizontal_shear(sums)
    assert shear == mo.horizontal_shear and cy == mo.m01            # the integer sums give ImageMoments' bits
    assert np.array_equal(p.shift_rows(binary, p.shear_shifts(0.0, cy, 24, 40)), binary)   # delta == 0: the identity


@pytest.mark.parametrize("k", [0.4, -0.25])
def test_a_sheared_bar_comes_back_upright(k):
    """Row y of the bar sits at x0 + round(k d), d = y - cy.  Every row has the same mass, so the measured shear is
    k + sum(e d) / sum(d^2) with |e| <= 1 / 2 the rounding of the row's position: off by at most eps = sum |d| / (2
    sum d^2).  SetSlant(0) moves row y back by round(shear d), so it ends within eps * max |d| + 1 columns of x0."""
    p, m = _p(), _m()
    binary, x0, rows = pc.sheared_bar(k)
    morph = m.ImageMorphology(binary.astype(float), scale=1, binary=binary)
    d = rows - rows.mean()
    eps = np.abs(d).sum() / (2 * (d * d).sum())
    shear = m.ImageMoments(binary).horizontal_shear
    assert abs(shear - k) <= eps
    bound = int(np.floor(eps * np.abs(d).max())) + 1
    up = p.SetSlant(0.0)(morph)
    start = np.array([np.nonzero(up[y])[0].min() for y in rows])
    assert (up[rows].sum(1) == 9).all() and up.sum() == binary.sum()
    print(f"sheared bar k={k}: measured {shear:.4f}, rows within {np.abs(start - x0).max()} of upright, bound {bound}")
    assert np.abs(start - x0).max() <= bound and bound <= 2


# --------------------------------------------------------------------------------------------------------------- chain
def test_status_corners_and_none_targets():
    p = _p()
    im = mc.stroke(seed=3)
    base = p.counterfactual_image(im, scale=4)
    assert base["status"] == 0 and base["radius"] == 0 and not base["shifts"].any()
    assert np.array_equal(base["image"], base["quantised"]) and 200 < base["image"].max() <= 255
    assert np.array_equal(base["reshaped"], base["warped"])
    far = p.counterfactual_image(im, thickness=base["thickness"] + 2 * 9.5 / 4, scale=4, max_radius=8)
    assert far["status"] == 3 and far["radius"] == 9 and not far["image"].any()
    gone = p.counterfactual_image(im, thickness=-3.0, scale=4)       # erosion removes every pixel
    assert gone["status"] == 4 and gone["radius"] < 0 and not gone["image"].any() and not gone["reshaped"].any()
    flat = p.counterfactual_image(np.full((28, 28), 0.5), 2.0, 0.1, 100., scale=4)
    assert flat["status"] == 1 and not flat["image"].any()
    row = np.zeros((28, 28))
    row[14, 4:24] = 1                                                # (its bitmap at scale 1 is one row: u02 == 0)
    line = p.counterfactual_image(row, None, 0.2, None, scale=1)
    assert line["status"] == 4
    both = p.counterfactual_image(im, None, None, 100.0, scale=4)
    assert both["status"] == 0
    assert abs(np.median(both["image"][both["image"] >= both["image"].max() / 2]) - 100.0) <= 1e-12


def test_executor_on_cpu_tensors_is_the_statement():
    from ali_hip.morpho import MorphoPerturb
    p = _p()
    x = mc.generator_images(4, seed=2)
    th, sl, it = np.array([2.0, 3.5, 9.0, 2.5]), np.array([0.3, -0.2, 0.0, 0.1]), np.array([120., 250., 90., 200.])
    for dtype, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        mp = MorphoPerturb(scale=4, max_radius=6)
        out = mp.apply(torch.from_numpy(x).to(tdt).reshape(4, 1, 28, 28), torch.from_numpy(th), torch.from_numpy(sl),
                       torch.from_numpy(it))
        assert out["images"].dtype == tdt and out["status"].tolist() == [0, 0, 3, 0]
        for b in range(4):
            want = p.counterfactual_image(x[b].astype(dtype), th[b], sl[b], it[b], 4, dtype=dtype, max_radius=6)
            assert np.array_equal(out["images"][b].numpy(), want["image"]) and out["radius"][b] == want["radius"]
            assert out["thickness_before"][b].item() == want["thickness"]
    none = MorphoPerturb(scale=4).apply(torch.from_numpy(x))
    assert none["status"].tolist() == [0] * 4 and none["radius"].tolist() == [0] * 4


def test_the_scripts_loop_body_is_apply():
    """mnist_vae_measured_cf.py's lines per image against one ``apply``: the same image, bit for bit (the scripts form
    ``mult = in_ / current_intensity`` first, as the statement does)"""
    from ali_hip.morpho import MorphoPerturb
    x = 255 * (mc.generator_images(3, seed=4).astype(np.float64) + 1) / 2
    th, sl, it = [3.1, 1.9, 2.6], [0.25, -0.3, 0.0], [180., 230., 110.]
    out = MorphoPerturb(scale=4).apply(torch.from_numpy(x), torch.tensor(th, dtype=torch.float64),
                                       torch.tensor(sl, dtype=torch.float64), torch.tensor(it, dtype=torch.float64))
    assert out["status"].tolist() == [0, 0, 0]
    for b in range(3):
        want = pc.script_loop_body(x[b], th[b], sl[b], it[b], 4)
        assert np.array_equal(out["images"][b].numpy(), want)
