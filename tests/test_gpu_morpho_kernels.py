"""The four kernels of csrc/morpho.hip on the device, stage by stage, against the statement ``morphomnist.morpho``:
``ops.morpho_binarise`` (bits outside the rounding band of the threshold, min / max / count to the band, moments to the
yardstick), ``ops.morpho_edt`` (exact integers), ``ops.morpho_thin`` (the sequential loop's skeleton, exactly) and
``ops.morpho_measure`` (counts and intensity exactly, values to the yardstick of ``flow_cases.within_yardstick``).

Shapes: 5 x 9 at scales 1, 2, 4 (up-sampled widths 9, 18, 36: no multiple of a bitmap word) and 28 x 28 at scale 4 with
B in {1, 3, 70}; 28 x 28 at scale 16 with B = 3; the thinning also at the limit, 512 x 512.  Every call is made twice
and must give the same bits."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import morpho_cases as mc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(H, W, s, B) for (H, W, s) in mc.SMALL for B in mc.BATCHES] + [(28, 28, 16, 3)]
HIRES = sorted({(H * s, W * s) for (H, W, s) in mc.SMALL})          # the up-sampled sizes of the built binary images


def _ops():
    from ali_hip import ops
    return ops


def _stmt():
    from morphomnist import morpho
    return morpho


def _mo():
    from ali_hip import morpho
    return morpho


def _twice(fn):
    """fn() twice; every tensor of the two results holds the same bits"""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        bits = {4: torch.int32, 8: torch.int64}[u.element_size()]
        assert torch.equal(u.view(bits), v.view(bits))               # (bits: a NaN equals itself)
    return a


def _raw_sums(h, dtype):
    """(sum v, sum x v, sum y v, sum x^2 v, sum x y v, sum y^2 v) of an image in ``dtype``"""
    h = np.asarray(h, dtype=dtype)
    y, x = (g.astype(dtype) for g in np.mgrid[:h.shape[0], :h.shape[1]])
    return np.array([h.sum(), (x * h).sum(), (y * h).sum(), (x * x * h).sum(), (x * y * h).sum(), (y * y * h).sum()],
                    dtype=dtype)


@functools.lru_cache(maxsize=None)
def _binarised(H, W, s, B):
    """one batch through ``ops.morpho_binarise`` (twice) and through the statement in fp64 and fp32"""
    ops, m, mo = _ops(), _stmt(), _mo()
    x = mc.image_batch(B, H, W, seed=H + s).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    AH, AW = mo.MorphoMeasure(scale=s).operators(H, W, torch.device(DEV))
    bits, fg, hstats = _twice(lambda: ops.morpho_binarise(xd, s, AH, AW, 0.5))
    x64 = x.astype(np.float64)
    h64 = np.stack([m.expand(im, s) for im in x64])
    h32 = np.stack([m.expand(im, s, np.float32) for im in x])
    return dict(x=x, xd=xd, bits=bits, fg=fg, hstats=hstats, h64=h64, h32=h32, Wh=W * s,
                bin=mo.unpack_bits(bits, W * s))


# ---------------------------------------------------------------------------------------------------------- binarise
@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_binarise(H, W, s, B):
    c = _binarised(H, W, s, B)
    h64, h32 = c["h64"], c["h32"]
    band = 8 * np.abs(h32 - h64).max()                              # 8 x the error of the same product in CPU fp32
    lo, hi = h64.min((1, 2)), h64.max((1, 2))
    thr = lo + (hi - lo) * 0.5
    want = h64 >= thr[:, None, None]
    near = np.abs(h64 - thr[:, None, None]) <= band
    # the inputs: the reference alone has at most 0.1 % of its foreground inside the band
    assert (near & want).sum() <= 1e-3 * want.sum(), ((near & want).sum(), want.sum())
    differ = c["bin"] != want
    print(f"binarise {H}x{W} s={s} B={B}: band {band:.3g}, {int(near.sum())} pixels inside it, {int(differ.sum())} "
          f"bits differ")
    assert not (differ & ~near).any()
    fg, hs = c["fg"].cpu().numpy(), c["hstats"].cpu().numpy()
    assert (fg == c["bin"].sum((1, 2))).all()                        # the count is the count of the bits written
    assert (np.abs(fg - want.sum((1, 2))) <= near.sum((1, 2))).all()
    assert (np.abs(hs[:, 0] - lo) <= band).all() and (np.abs(hs[:, 1] - hi) <= band).all()
    ref = np.stack([_raw_sums(h, np.float64) for h in h64])
    f32 = np.stack([_raw_sums(h, np.float32) for h in h32])
    within_yardstick(f"binarise moments {H}x{W} s={s} B={B}", torch.from_numpy(hs[:, 2:]), torch.from_numpy(ref),
                     torch.from_numpy(f32))
    pad = c["bits"].cpu().numpy().view(np.uint32)                    # the bits beyond the image are written as 0
    if c["Wh"] % 32:
        assert not (pad[:, :, -1] >> (c["Wh"] % 32)).any()


def test_binarise_constant_image_is_all_foreground():
    ops, mo = _ops(), _mo()
    for s in (1, 4):
        x = torch.full((2, 5, 9), 0.3, device=DEV)
        AH, AW = mo.MorphoMeasure(scale=s).operators(5, 9, torch.device(DEV))
        bits, fg, _ = _twice(lambda: ops.morpho_binarise(x, s, AH, AW, 0.5))
        assert fg.tolist() == [45 * s * s] * 2 and mo.unpack_bits(bits, 9 * s).all()
        d2, status = ops.morpho_edt(bits, 9 * s)
        assert status.tolist() == [1, 1]
        skel = ops.morpho_thin(bits, d2, fg, status, _stmt().keep_bits(), 0)
        assert int(skel.count_nonzero()) == 0 and status.tolist() == [1, 1]
        _, values, _ = ops.morpho_measure(x, s, skel, d2, fg, torch.zeros(2, 8, dtype=torch.float64, device=DEV), status)
        assert torch.isnan(values[:, :3]).all() and values[:, 3].tolist() == [np.float32(0.3)] * 2


def test_limits():
    ops = _ops()
    with pytest.raises(ValueError, match="exceed the limit"):
        ops.morpho_binarise(torch.zeros(1, 33, 28, device=DEV), 16, None, None)
    from ctypes import c_void_p
    from ali_hip import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = c_void_p(t.data_ptr())
    assert lib.ali_morpho_edt(p, 1, 513, 8, p, p, p, 1 << 30, None) != 0        # checked before any launch
    assert lib.ali_morpho_thin(p, p, p, 1, 8, 513, 0, p, p, p, p, 1 << 30, None) != 0
    ws = torch.zeros(4096 + 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.morpho_edt(torch.zeros(1, 8, 1, dtype=torch.int32, device=DEV), 9, ws=ws)


# --------------------------------------------------------------------------------------------------------------- edt
def _built(Hh, Wh, B):
    """B built binary images [B, Hh, Wh]: the cases of ``binary_cases`` in turn, with another seed each time round"""
    out = []
    while len(out) < B:
        out += list(mc.binary_cases(Hh, Wh, seed=len(out)).values())
    return np.stack(out[:B])


def _check_edt(name, images):
    ops, mo = _ops(), _mo()
    B, Hh, Wh = images.shape
    bits = mo.pack_bits(images).to(DEV)
    full = images.all((1, 2))
    d2, status = ops.morpho_edt(bits, Wh)
    d2b, statusb = ops.morpho_edt(bits, Wh)
    assert status.tolist() == full.astype(int).tolist() and torch.equal(status, statusb), name
    live = torch.from_numpy(~full).to(DEV)
    assert torch.equal(d2[live], d2b[live]), name                    # (an image without background: d2 is not written)
    got = d2.cpu().numpy()
    for b in np.nonzero(~full)[0]:
        want = np.rint(ndimage.distance_transform_edt(images[b]) ** 2).astype(np.int64)
        assert np.array_equal(got[b], want), (name, int(b), int((got[b] != want).sum()))
    return bits, d2, status


@pytest.mark.parametrize("Hh,Wh", HIRES)
@pytest.mark.parametrize("B", [9, 70])
def test_edt_built_images(Hh, Wh, B):
    images = _built(Hh, Wh, B)
    images[0, :, :] = True                                           # the first: no background at all -> status 1
    _check_edt(f"edt built {Hh}x{Wh} B={B}", images)


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_edt_device_images(H, W, s, B):
    _check_edt(f"edt device {H}x{W} s={s} B={B}", _binarised(H, W, s, B)["bin"])


def test_edt_large_distances():
    """448 x 448: a single background pixel (every distance up to the diagonal), blobs, full rows"""
    cases = mc.binary_cases(448, 448)
    _check_edt("edt 448", np.stack([cases[k] for k in ("hole", "blobs", "rows", "frame")]))


# -------------------------------------------------------------------------------------------------------------- thin
def _check_thin(name, images, seeds=(0,)):
    ops, m, mo = _ops(), _stmt(), _mo()
    B, Hh, Wh = images.shape
    assert not images.all((1, 2)).any()
    bits, d2, status = _check_edt(name, images)
    fg = torch.from_numpy(images.sum((1, 2)).astype(np.int32)).to(DEV)
    d2h = d2.cpu().numpy().astype(np.int64)
    for seed in seeds:
        (skel,) = _twice(lambda: (ops.morpho_thin(bits, d2, fg, status, m.keep_bits(), seed),))
        assert status.tolist() == [0] * B, name
        got = mo.unpack_bits(skel, Wh)
        for b in range(B):
            want = m.thin(images[b], d2h[b], seed)
            assert np.array_equal(got[b], want), (name, seed, b, int((got[b] != want).sum()))


@pytest.mark.parametrize("Hh,Wh", HIRES)
def test_thin_built_images(Hh, Wh):
    """random blobs (large plateaus), one-pixel lines, two-wide bars, foreground on the border, a single background
    pixel, one pixel, the empty image; B = 27 with three seeds of blobs, thinning seeds 0 and 5"""
    _check_thin(f"thin built {Hh}x{Wh}", _built(Hh, Wh, 27), seeds=(0, 5))


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_thin_device_images(H, W, s, B):
    _check_thin(f"thin device {H}x{W} s={s} B={B}", _binarised(H, W, s, B)["bin"])


def test_thin_at_the_limit():
    """512 x 512, the largest image: two bitmaps of 32 KB in LDS (the raised limit of the workgroup) and eight words per
    thread; blobs and a two-wide bar along the border"""
    blobs = mc.blobs(512, 512, seed=3, fill=0.2)
    bars = np.zeros((512, 512), dtype=bool)
    bars[:, 510:] = True
    bars[0:2, :] = True
    bars[100:104, 5:500] = True
    _check_thin("thin 512", np.stack([blobs, bars]))


# ----------------------------------------------------------------------------------------------------------- measure
def _dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def test_measure_hand_built_skeletons():
    """a straight run of n pixels has n - 1 straight pairs, a diagonal run n - 1 diagonal pairs; an L, a 2 x 2 block; the
    empty skeleton has a NaN thickness"""
    ops, mo = _ops(), _mo()
    cases = mc.skeleton_cases()
    names = list(cases)
    skels = np.stack([cases[k][0] for k in names])
    B, Hh, Wh = skels.shape
    g = np.random.default_rng(3)
    d2 = g.integers(1, 60, size=skels.shape)
    fg = g.integers(50, 200, size=B)
    x = torch.from_numpy(mc.image_batch(B, Hh, Wh, seed=2).astype(np.float32)).to(DEV)
    _, _, hstats = ops.morpho_binarise(x, 1)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    counts, values, slant = _twice(lambda: ops.morpho_measure(x, 1, mo.pack_bits(skels).to(DEV), _dev_i32(d2),
                                                              _dev_i32(fg), hstats, status))
    want = np.array([[fg[i], skels[i].sum(), cases[k][1], cases[k][2]] for i, k in enumerate(names)])
    assert np.array_equal(counts.cpu().numpy(), want), (counts, want)
    ref, f32 = [], []
    for dt, out in ((np.float64, ref), (np.float32, f32)):
        for i in range(B):
            n = max(skels[i].sum(), 1)
            out.append([dt(fg[i]), dt(want[i, 2]) + np.sqrt(dt(2)) * dt(want[i, 3]),
                        dt(2) * np.sqrt(d2[i][skels[i]].astype(dt)).sum(dtype=dt) / dt(n)])
    has = torch.from_numpy(skels.sum((1, 2)) > 0)
    got = values[:, :3].cpu()
    assert torch.isnan(got[~has][:, 2]).all() and (~has).sum() == 1
    ref, f32 = torch.tensor(np.array(ref)), torch.tensor(np.array(f32, dtype=np.float32))
    within_yardstick("measure area, length", got[:, :2], ref[:, :2], f32[:, :2])
    within_yardstick("measure thickness", got[has][:, 2], ref[has][:, 2], f32[has][:, 2])


def test_measure_scale_divides():
    """area / scale^2, length and thickness / scale: the skeletons of the run and the block at scale 2 (4 x 20 images)"""
    ops, mo = _ops(), _mo()
    cases = mc.skeleton_cases(8, 40)
    skels = np.stack([cases[k][0] for k in ("run", "block", "ell")])
    d2 = np.full(skels.shape, 9)
    fg = np.array([40, 80, 120])
    x = torch.from_numpy(mc.image_batch(3, 4, 20, seed=1).astype(np.float32)).to(DEV)
    AH, AW = mo.MorphoMeasure(scale=2).operators(4, 20, torch.device(DEV))
    _, _, hstats = ops.morpho_binarise(x, 2, AH, AW)
    counts, values, _ = ops.morpho_measure(x, 2, mo.pack_bits(skels).to(DEV), _dev_i32(d2), _dev_i32(fg), hstats,
                                           torch.zeros(3, dtype=torch.int32, device=DEV))
    pairs = np.array([[cases[k][1], cases[k][2]] for k in ("run", "block", "ell")])
    assert np.array_equal(counts[:, 2:].cpu().numpy(), pairs)
    want = np.stack([fg / 4, (pairs[:, 0] + np.sqrt(2.) * pairs[:, 1]) / 2, np.full(3, 2 * 3 / 2)], axis=1)
    assert np.allclose(values[:, :3].cpu().numpy(), want, rtol=2e-7, atol=0)


@pytest.mark.parametrize("H,W", [(2, 4), (5, 9), (28, 28), (7, 40)])
def test_measure_intensity_and_shear(H, W):
    """the median of the upper half, exactly: odd and even counts, ties (values on a grid of 8 levels), negative
    values; the shear of (image - min) to the yardstick"""
    ops, m, mo = _ops(), _stmt(), _mo()
    g = np.random.default_rng(H * W)
    ims = [mc.image_batch(2, H, W, seed=5)[i] for i in range(2)] if H >= 5 else []
    ims += [g.integers(0, 8, size=(H, W)) / 7.0, g.integers(0, 8, size=(H, W)) * 32.0 - 100.0,
            g.random((H, W)) * 2 - 1, g.random((H, W))]
    if (H, W) == (2, 4):
        ims += [np.array([[0., 10., 6., 8.], [1., 2., 9., 5.]]), np.array([[0., 10., 6., 8.], [1., 2., 9., 3.]]),
                np.array([[0., 10., 7., 7.], [7., 2., 10., 3.]])]
    x = np.stack(ims).astype(np.float32)
    B = len(x)
    xd = torch.from_numpy(x).to(DEV)
    bits, fg, hstats = ops.morpho_binarise(xd, 1)
    d2, status = ops.morpho_edt(bits, W)
    skel = ops.morpho_thin(bits, d2, fg, status, m.keep_bits(), 0)
    _, values, slant = _twice(lambda: ops.morpho_measure(xd, 1, skel, d2, fg, hstats, status))
    x64 = x.astype(np.float64)
    want = np.array([m.intensity(im) for im in x64])
    n_sel = [int((im >= im.min() + (im.max() - im.min()) * .5).sum()) for im in x64]
    assert {n % 2 for n in n_sel} == {0, 1} or B < 4, n_sel         # odd and even counts both occur
    assert np.array_equal(values[:, 3].cpu().numpy(), want.astype(np.float32)), (values[:, 3], want)
    ref = torch.tensor([-m.ImageMoments(im - im.min()).horizontal_shear for im in x64])
    f32 = torch.tensor([-m.ImageMoments(im - im.min(), np.float32).horizontal_shear for im in x])
    within_yardstick(f"shear {H}x{W}", values[:, 4], ref, f32)
    within_yardstick(f"slant_hires {H}x{W} (scale 1)", slant, torch.atan(ref), torch.atan(f32))
