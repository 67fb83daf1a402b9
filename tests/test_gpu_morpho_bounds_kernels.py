"""``ops.morpho_bounds`` (csrc/morpho.hip: ali_morpho_bounds) on the device against the statement
``morphomnist.morpho.measure_bounds`` / ``bounds_of``.

The yardstick is ``flow_cases.within_yardstick`` with its default multiplier.  The reference is the fp64 statement on
the images the device reads (fp32, widened); the yardstick is the same statement with the up-sampling product formed
in fp32 -- the one place where the kernel rounds to fp32 -- and everything after it in fp64, as the reference's
``bounding_parallelogram`` takes any image.
  shear, middle   against the statement's own moments.
  hcdf, vcdf and the four locations   against the statement continued from the device's shear and middle: bin
                  membership then rests on identical fp64 inputs, so a wrong comparison is a jump of a whole pixel's
                  mass, and the rounding of hires is all that is left to the yardstick.  The chosen intervals must be
                  the statement's exactly, and each location must be ``quantile_loc`` of the device's own cdf bit for
                  bit.

Shapes: ``mc.SMALL`` (5 x 9 at scales 1, 2, 4; 28 x 28 at 4) with B in {1, 3, 70}; 28 x 28 at 16 with B = 3 (T in LDS);
32 x 32 at 16 (512 x 512, the limit, T in the workspace) and 16 x 32 at 16 (512 wide, T in LDS)."""
import types

import numpy as np
import pytest
import torch

import morpho_cases as mc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAC = .02
SHAPES = [(H, W, s, B) for (H, W, s) in mc.SMALL for B in mc.BATCHES] + [(28, 28, 16, 3), (32, 32, 16, 1),
                                                                        (16, 32, 16, 1)]


def _m():
    from morphomnist import morpho
    return morpho


def _ops():
    from ali_hip import ops
    return ops


def _operators(H, W, s):
    from ali_hip.morpho import MorphoMeasure
    return MorphoMeasure(scale=s).operators(H, W, torch.device(DEV))


def _launch(x32, s, frac=FRAC, debug=True):
    """the kernel on fp32 images [B, H, W] (numpy); twice, the same bits; numpy results"""
    ops = _ops()
    B, H, W = x32.shape
    AH, AW = _operators(H, W, s)
    x = torch.from_numpy(np.ascontiguousarray(x32)).to(DEV)
    a = ops.morpho_bounds(x, s, AH, AW, frac, debug=debug)
    b = ops.morpho_bounds(x, s, AH, AW, frac, debug=debug)
    a, b = (a, b) if debug else ((a,), (b,))
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int64), v.view(torch.int64))            # (bits: a NaN equals itself)
    return [t.cpu().numpy() for t in a]


def _crossings(c, f):
    """the intervals j where c crosses f upward (-1: f below c[0]; len(c) - 1: f at or above c[-1])"""
    p = np.concatenate([[-np.inf], c, [np.inf]])
    return [j - 1 for j in range(len(p) - 1) if p[j] <= f < p[j + 1]]


def _interval(c, f, side):
    hits = _crossings(c, f)
    return hits[0] if side == "left" else hits[-1]


def _images(H, W, B):
    return mc.image_batch(B, H, W).astype(np.float32)


_CACHE = {}


def _statement(H, W, s, B):
    """per image: (hires64, hires32, (shear, middle) of each); computed once per shape"""
    key = (H, W, s, B)
    if key not in _CACHE:
        m = _m()
        x32 = _images(H, W, B)
        rows = []
        for im in x32:
            h = {dt: m.expand(im.astype(dt) - im.astype(dt).min(), s, dt) for dt in (np.float64, np.float32)}
            mo = {dt: m.ImageMoments(h[dt]) for dt in h}
            rows.append((h, {dt: (mo[dt].horizontal_shear, mo[dt].m01) for dt in mo}))
        _CACHE[key] = (x32, rows)
    return _CACHE[key]


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_shear_and_middle(H, W, s, B):
    x32, rows = _statement(H, W, s, B)
    bounds = _launch(x32, s, debug=False)[0]
    for j, name in ((0, "shear"), (1, "middle")):
        ref = torch.tensor([r[1][np.float64][j] for r in rows])
        f32 = torch.tensor([r[1][np.float32][j] for r in rows])
        within_yardstick(f"bounds {name} {H}x{W} s={s} B={B}", torch.from_numpy(bounds[:, 4 + j]), ref, f32)


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_cdfs_and_locations(H, W, s, B):
    m = _m()
    x32, rows = _statement(H, W, s, B)
    bounds, hcdf, vcdf = _launch(x32, s)
    assert hcdf.shape == (B, W * s) and vcdf.shape == (B, H * s)
    levels = ((0, hcdf, FRAC / 2, "left"), (1, hcdf, 1 - FRAC / 2, "right"), (2, vcdf, FRAC / 2, "left"),
              (3, vcdf, 1 - FRAC / 2, "right"))
    cont = []
    differ = 0
    for b, (h, _) in enumerate(rows):
        dev = types.SimpleNamespace(centroid=(np.nan, bounds[b, 5]), horizontal_shear=bounds[b, 4])
        c = {dt: m.bounds_of(h[dt], FRAC, dev) for dt in h}
        cont.append(c)
        for k, cdf, f, side in levels:
            ref_c = c[np.float64][6 if k < 2 else 7]
            j = _interval(ref_c, f, side)
            assert _interval(cdf[b], f, side) == j, (b, k, _interval(cdf[b], f, side), j)
            differ += _interval(c[np.float32][6 if k < 2 else 7], f, side) != j
            assert bounds[b, k] == m.quantile_loc(cdf[b], f, side), (b, k, bounds[b, k])   # the device's own cdf
    print(f"bounds {H}x{W} s={s} B={B}: {differ} intervals of the fp32 statement differ from the fp64 one's")
    tag = f"{H}x{W} s={s} B={B}"
    for name, got, k in (("hcdf", hcdf, 6), ("vcdf", vcdf, 7)):
        within_yardstick(f"bounds {name} {tag}", torch.from_numpy(got),
                         torch.from_numpy(np.stack([c[np.float64][k] for c in cont])),
                         torch.from_numpy(np.stack([c[np.float32][k] for c in cont])))
    within_yardstick(f"bounds locations {tag}", torch.from_numpy(bounds[:, :4]),
                     torch.tensor([[float(v) for v in c[np.float64][:4]] for c in cont]),
                     torch.tensor([[float(v) for v in c[np.float32][:4]] for c in cont]))


def test_rows_equal_single_image_launches():
    x32, _ = _statement(28, 28, 4, 70)
    whole = _launch(x32, 4)
    for b in range(70):
        one = _launch(x32[b:b + 1], 4)
        for u, v in zip(whole, one):
            assert np.array_equal(u[b:b + 1].view(np.int64), v.view(np.int64)), b


@pytest.mark.parametrize("frac,k,want", [(.072, 0, 6), (.002, 1, 27)])
def test_dot_and_bar_takes_the_right_crossing(frac, k, want):
    """hcdf crosses the level twice upward (at j = 6 and 17 for frac .072; at 24 and 27 for .002): left takes the
    first interval, right the last"""
    m = _m()
    im = np.zeros((1, 12, 16), dtype=np.float32)
    im[0, 2:10, 9:12] = 1
    im[0, 5, 2] = 1
    bounds, hcdf, _ = _launch(im, 2, frac)
    f = frac / 2 if k == 0 else 1 - frac / 2
    assert len(_crossings(hcdf[0], f)) == 2
    assert _interval(hcdf[0], f, "left" if k == 0 else "right") == want
    assert want <= bounds[0, k] < want + 1
    h = m.measure_bounds(im[0].astype(np.float64), 2, frac)["hires"]
    dev = types.SimpleNamespace(centroid=(np.nan, bounds[0, 5]), horizontal_shear=bounds[0, 4])
    ref = m.bounds_of(h, frac, dev)
    h32 = m.measure_bounds(im[0], 2, frac, np.float32)["hires"]
    f32 = m.bounds_of(h32, frac, dev)
    within_yardstick(f"dot and bar {frac}", torch.tensor(bounds[0, :4]), torch.tensor([float(v) for v in ref[:4]]),
                     torch.tensor([float(v) for v in f32[:4]]))


def test_nan_where_the_statement_has_it():
    """a constant image (no mass) among ordinary ones: its four locations are NaN, the others are not"""
    m = _m()
    x32 = _images(28, 28, 4)
    x32[2] = 0.4
    bounds, hcdf, vcdf = _launch(x32, 4)
    for b in range(4):
        want = m.measure_bounds(x32[b].astype(np.float64), 4, FRAC)["bounds"]
        assert np.array_equal(np.isnan(bounds[b]), np.isnan(want)), (b, bounds[b], want)
    assert np.isnan(bounds[2, :4]).all() and not np.isnan(bounds[[0, 1, 3], :4]).any()


def test_refusals_before_any_launch():
    from ctypes import c_void_p

    from ali_hip import _lib
    ops = _ops()
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    a = c_void_p(t.data_ptr())
    big = 1 << 30
    assert lib.ali_morpho_bounds(a, 33 * 28, 1, 33, 28, 16, a, a, .02, a, a, a, a, big, None) != 0   # side > 512
    assert lib.ali_morpho_bounds(a, 64, 1, 8, 8, 2, a, a, 0.0, a, a, a, a, big, None) != 0          # bound_frac
    assert lib.ali_morpho_bounds(a, 64, 1, 8, 8, 2, a, a, 1.0, a, a, a, a, big, None) != 0
    assert lib.ali_morpho_bounds(a, 64, 1, 8, 8, 2, a, a, float("nan"), a, a, a, a, big, None) != 0
    assert lib.ali_morpho_bounds(a, 64, 0, 8, 8, 2, a, a, .02, a, a, a, a, big, None) != 0          # B < 1
    assert lib.ali_morpho_bounds(a, 64, 1, 8, 8, 2, None, a, .02, a, a, a, a, big, None) != 0       # no operator
    assert lib.ali_morpho_bounds(a, 32 * 32, 1, 32, 32, 16, a, a, .02, a, a, a, a, 4096 + 16, None) != 0   # workspace
    torch.cuda.synchronize()
    assert not t.any()                                               # nothing ran
    x = torch.zeros(1, 33, 28, device=DEV)
    with pytest.raises(ValueError, match="exceed the limit"):
        ops.morpho_bounds(x, 16, *_operators(28, 28, 16))
    x = torch.zeros(1, 8, 8, device=DEV)
    for frac in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="bound_frac"):
            ops.morpho_bounds(x, 2, *_operators(8, 8, 2), frac)
    with pytest.raises(ValueError, match="expand operator"):
        ops.morpho_bounds(x, 2, None, None, .02)
