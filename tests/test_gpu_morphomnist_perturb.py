"""``ali_hip.morpho.MorphoPerturb`` on the device, end to end: chunks against single images bit for bit, the seven launches
replayed one by one from the device's own binary image and thickness against the statement ``morphomnist.perturb``, the
Generator's range against 0 .. 255, ``None`` targets, status rows, a HIP graph, and the round trip through
``MorphoMeasure``."""
import numpy as np
import pytest
import torch

import morpho_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("images", "status", "radius", "thickness_before", "shear_before", "intensity_before")


def _mo():
    from ali_hip import morpho
    return morpho


def _same_bits(a, b, name):
    assert a.dtype == b.dtype and a.shape == b.shape, name
    bits = {4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)), name


def _targets(B, seed=0):
    """thickness 1.5 .. 4.5 (either side of a stroke's 2 .. 3), slant -0.4 .. 0.4 rad, intensity 80 .. 250"""
    g = np.random.default_rng(50 + seed)
    return tuple(torch.from_numpy(g.uniform(lo, hi, size=B).astype(np.float32)).to(DEV)
                 for lo, hi in ((1.5, 4.5), (-0.4, 0.4), (80, 250)))


def test_chunks_and_single_images():
    mo = _mo()
    x = torch.from_numpy(mc.generator_images(5, seed=1)).to(DEV)
    t, s, i = _targets(5)
    mp = mo.MorphoPerturb(scale=4, chunk=2, max_radius=8)             # two chunks and a remainder of one
    out, again = mp.apply(x, t, s, i), mp.apply(x, t, s, i)
    whole = mo.MorphoPerturb(scale=4, max_radius=8).apply(x.reshape(5, 1, 28, 28), t, s, i)
    single = mo.MorphoPerturb(scale=4, max_radius=8)
    ones = [single.apply(x[b:b + 1], t[b:b + 1], s[b:b + 1], i[b:b + 1]) for b in range(5)]
    assert out["images"].shape == (5, 28, 28) and out["images"].dtype == torch.float32
    assert out["status"].tolist() == [0] * 5 and out["shear_before"].dtype == torch.float64
    for k in KEYS:
        _same_bits(out[k], again[k], k)
        _same_bits(out[k], whole[k], k)
        _same_bits(out[k], torch.cat([o[k] for o in ones]), k)
    assert 0 <= float(out["images"].min()) and float(out["images"].max()) <= 255


@pytest.mark.parametrize("scale,B", [(4, 6), (16, 3)])
def test_against_the_statement_stage_by_stage(scale, B):
    """The chain replayed launch by launch from the device's own bitmap and thickness gives ``apply``'s bits, and every
    stage is the statement's continued from there: radius, reshaped bitmap, sums, shear and shifts exactly; the
    quantised image within the rounding band (8 x the fp32 statement's error) of the fp64 statement's; the median that
    of the device's own quantised image; the image within 2 ulp of the fp32 product on it."""
    from ali_hip import ops
    from morphomnist import perturb as p
    mo = _mo()
    pred = mc.generator_images(B, seed=3 + scale)
    x = torch.from_numpy(pred).to(DEV)
    t, s, i = _targets(B, seed=scale)
    max_radius = 8 if scale == 4 else 24                             # |delta| <= 2.5: a radius up to 5, or 20
    mp = mo.MorphoPerturb(scale=scale, max_radius=max_radius)
    out = mp.apply(x, t, s, i)
    both = mp.apply(255 * (x + 1) / 2, t, s, i)                      # the scripts' range: the same arithmetic
    for k in KEYS:
        _same_bits(out[k], both[k], k)
    H = W = 28
    mm = mp.measure
    AH, AW = mm.operators(H, W, x.device)
    RH, RW = mp.reduce_operators(H, W, x.device)
    bits, fg, hstats = ops.morpho_binarise(x, scale, AH, AW, 0.5)
    d2, st = ops.morpho_edt(bits, W * scale)
    skel = ops.morpho_thin(bits, d2, fg, st, mm._keep, 0)
    _, values, _ = ops.morpho_measure(x, scale, skel, d2, fg, hstats, st)
    shear_t = -torch.tan(s.double())
    shaped, radius, sums, st2 = ops.morpho_reshape(bits, W * scale, values[:, 2], t, st, mp.half_table(x.device), scale)
    q, shear, raw, shifts = ops.morpho_shear_reduce(shaped, H, W, scale, sums, shear_t, st2, RH, RW, debug=True)
    img, median, st3 = ops.morpho_set_intensity(q, i, st2)
    for k, v in (("images", img), ("status", st3), ("radius", radius), ("thickness_before", values[:, 2]),
                 ("shear_before", shear), ("intensity_before", median)):
        _same_bits(out[k], v, k)
    assert st3.tolist() == [0] * B
    binary, reshaped = mo.unpack_bits(bits, W * scale), mo.unpack_bits(shaped, W * scale)
    thick, tt, ss, ii = (v.cpu().numpy() for v in (values[:, 2], t, shear_t, i))
    q, raw, img, median = (v.cpu().numpy() for v in (q, raw, img, median))
    for b in range(B):
        ref = {dt: p.continue_from(binary[b], thick[b], H, W, tt[b], ss[b], ii[b], scale, 0, dt, max_radius)
               for dt in (np.float64, np.float32)}
        r64, r32 = ref[np.float64], ref[np.float32]
        assert r64["status"] == 0 and int(radius[b]) == r64["radius"], (b, int(radius[b]), r64["radius"])
        assert np.array_equal(reshaped[b], r64["reshaped"]) and sums[b].tolist() == r64["sums"].tolist(), b
        assert float(shear[b]) == r64["shear"] and np.array_equal(shifts[b].cpu().numpy(), r64["shifts"]), b
        band = 8 * np.abs(r32["raw"].astype(np.float64) - r64["raw"]).max()
        guarded = np.clip(r64["raw"], 0, 255) + 2.0 ** -7
        near = np.abs(guarded - np.rint(guarded)) <= band
        differ = q[b] != r64["quantised"]
        assert np.abs(raw[b] - r64["raw"]).max() <= band
        assert np.abs(q[b] - r64["quantised"]).max() <= 1 and not (differ & ~near).any(), (b, int(differ.sum()))
        assert median[b] == np.float32(p.set_intensity(q[b].astype(np.float64), None)[1]), b
        want = np.clip(q[b] * (ii[b] / median[b]), np.float32(0), np.float32(255))
        assert (np.abs(img[b] - want) <= 2 * np.spacing(np.maximum(want, np.float32(1e-30)))).all(), b
        print(f"perturb s={scale} b={b}: thickness {thick[b]:.3f} -> {tt[b]:.3f} radius {int(radius[b])}, shear "
              f"{float(shear[b]):.3f} -> {ss[b]:.3f}, median {median[b]} -> {ii[b]:.1f}; {int(near.sum())} pixels in the "
              f"band, {int(differ.sum())} differ")


def test_none_targets_and_status_rows():
    mo = _mo()
    pred = mc.generator_images(4, seed=9)
    pred[2] = 0.25                                                   # a constant image: no background, status 1
    x = torch.from_numpy(pred).to(DEV)
    mp = mo.MorphoPerturb(scale=4, max_radius=12)
    plain = mp.apply(x)
    assert plain["status"].tolist() == [0, 0, 1, 0] and plain["radius"].tolist() == [0] * 4
    assert not plain["images"][2].any() and torch.isnan(plain["intensity_before"][2])
    live = [0, 1, 3]
    assert (plain["images"][live].amax((1, 2)) > 128).all()
    assert torch.equal(plain["images"], torch.floor(plain["images"]))        # quantised, not rescaled
    t = torch.tensor([3.0, 30.0, 3.0, -1.5], device=DEV)             # radius 54 > 12: status 3; erosion by 7 .. 9: 4
    out = mp.apply(x, thickness=t)
    assert out["status"].tolist() == [0, 3, 1, 4] and int(out["radius"][1]) > 12 and int(out["radius"][3]) < 0
    assert not out["images"][1:].any() and out["images"][0].any()
    only_i = mp.apply(x, intensity=torch.full((4,), 100.0, device=DEV))
    _same_bits(only_i["intensity_before"], plain["intensity_before"], "median")
    assert float(only_i["images"][live].amax()) <= 255 and not torch.equal(only_i["images"], plain["images"])
    only_s = mp.apply(x, slant=torch.tensor([0.3, -0.3, 0.0, 0.2], device=DEV))
    _same_bits(only_s["shear_before"], plain["shear_before"], "shear")
    assert only_s["status"].tolist() == [0, 0, 1, 0]
    with pytest.raises(ValueError, match="exceed the limit"):
        mo.MorphoPerturb(scale=16).apply(torch.zeros(1, 33, 28, device=DEV))
    with pytest.raises(ValueError, match="tensor on"):
        mp.apply(x, thickness=torch.zeros(4))


def test_graph_capture_is_a_single_chain():
    """``apply`` records into a HIP graph (a host read inside a capture is an error: every launch is on the one capturing
    stream) and the replay on new inputs gives the bits of a fresh eager call"""
    mo = _mo()
    x = torch.from_numpy(mc.generator_images(3, seed=2)).to(DEV)
    t, s, i = _targets(3, seed=1)
    mp = mo.MorphoPerturb(scale=4, max_radius=8)
    eager = mp.apply(x, t, s, i)                                      # (also builds the operators, table and workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mp.apply(x, t, s, i)
    x.copy_(torch.from_numpy(mc.generator_images(3, seed=6)))
    graph.replay()
    fresh = mo.MorphoPerturb(scale=4, max_radius=8).apply(x, t, s, i)
    for k in KEYS:
        _same_bits(captured[k], fresh[k], k)
    assert not torch.equal(captured["images"], eager["images"])


def test_round_trip_through_measure():
    """``MorphoMeasure`` on ``apply``'s output reports finite attributes with status 0.  How close the measured
    thickness lands is not promised (``SetThickness`` is approximate in the reference too): the values are printed."""
    mo = _mo()
    x = torch.from_numpy(mc.generator_images(4, seed=5)).to(DEV)
    t, s, i = _targets(4, seed=2)
    mp = mo.MorphoPerturb(scale=4, max_radius=8)
    out = mp.apply(x, t, s, i)
    assert out["status"].tolist() == [0] * 4
    back = mo.MorphoMeasure(scale=4).measure(out["images"])
    assert back["status"].tolist() == [0] * 4
    for k in ("thickness", "intensity", "slant"):
        assert torch.isfinite(back[k]).all(), k
    for b in range(4):
        print(f"round trip {b}: thickness {float(out['thickness_before'][b]):.3f} -> target {float(t[b]):.3f}, measured "
              f"{float(back['thickness'][b]):.3f}; slant target {float(s[b]):.3f}, measured "
              f"{float(torch.atan(back['slant'][b])):.3f}; intensity target {float(i[b]):.1f}, measured "
              f"{float(back['intensity'][b]):.1f}")
