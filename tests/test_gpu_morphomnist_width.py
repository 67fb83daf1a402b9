"""``ali_hip.morpho.MorphoPerturb.set_width`` on the device, end to end: chunks against one launch bit for
bit, the launches replayed one by one from the device's own intermediates against the statement
``morphomnist.perturb``, ``intensity`` given and not, the one re-application of ``validate``, a HIP graph, the
Generator's range against 0 .. 255, and the round trip through ``morphomnist.measure.measure_batch``."""
import numpy as np
import pytest
import torch

import morpho_cases as mc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("images", "status", "width_before", "factor", "bounds_before", "shear_before", "intensity_before")
VKEYS = KEYS + ("width_after", "off_target")
FACTORS = (0.45, 1.3, 0.45, 0.7, 1.5, 0.45)      # of each image's own width; with ``generator_images(6, seed=4)`` rows
                                                 # 3 and 4 come out more than 1 pixel off target, the others do not


def _mo():
    from ali_hip import morpho
    return morpho


def _same_bits(a, b, name):
    assert a.dtype == b.dtype and a.shape == b.shape, name
    bits = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)), name


def _case(B, seed, scale=4, factors=FACTORS):
    """(images in -1 .. 1, target widths float64, target intensities float32) on the device"""
    from morphomnist import morpho as m
    pred = mc.generator_images(B, seed=seed)
    own = np.array([m.measure_bounds(im.astype(np.float64), min(scale, 4), .02)["width"] for im in pred])
    width = own * np.array([factors[b % len(factors)] for b in range(B)])
    inten = np.random.default_rng(60 + seed).uniform(80, 250, size=B).astype(np.float32)
    return torch.from_numpy(pred).to(DEV), torch.from_numpy(width).to(DEV), torch.from_numpy(inten).to(DEV)


def test_chunks_against_one_launch():
    mo = _mo()
    x, w, i = _case(5, seed=4)
    for validate, keys in ((False, KEYS), (True, VKEYS)):
        mp = mo.MorphoPerturb(scale=4, chunk=2)                      # two chunks and a remainder of one
        out, again = mp.set_width(x, w, i, validate=validate), mp.set_width(x, w, i, validate=validate)
        whole = mo.MorphoPerturb(scale=4).set_width(x.reshape(5, 1, 28, 28), w, i, validate=validate)
        assert set(out) == set(keys)
        for k in keys:
            _same_bits(out[k], again[k], k)
            _same_bits(out[k], whole[k], k)
        assert out["images"].shape == (5, 28, 28) and out["images"].dtype == torch.float32
        assert out["status"].tolist() == [0] * 5 and out["factor"].dtype == torch.float64
        assert 0 <= float(out["images"].min()) and float(out["images"].max()) <= 255


@pytest.mark.parametrize("scale,B", [(4, 6), (16, 3)])
def test_against_the_statement_launch_by_launch(scale, B):
    """The chain replayed launch by launch gives ``set_width``'s bits, and every launch is the statement's continued
    from the device's own intermediates: sums, shear, cx, cy exactly on the device's bitmap; left and right to the
    yardstick of the kernel tests; the warped bitmap exactly from the device's wb; the quantised image within the
    rounding band (8 x the fp32 statement's error) of the fp64 statement's; the median that of the device's own
    quantised image; the image within 2 ulp of the fp32 product on it."""
    from ali_hip import ops
    from morphomnist import morpho as m
    from morphomnist import perturb as p
    mo = _mo()
    x, w, i = _case(B, seed=3 + scale, scale=scale)
    mp = mo.MorphoPerturb(scale=scale)
    out = mp.set_width(x, w, i)
    H = W = 28
    AH, AW = mp.measure.operators(H, W, x.device)
    RH, RW = mp.reduce_operators(H, W, x.device)
    bits, fg, _ = ops.morpho_binarise(x, scale, AH, AW, 0.5)
    sums, wb, st = ops.morpho_width(x, scale, bits, fg, w, AH, AW, .02)
    q, st2, raw, warped = ops.morpho_affine_reduce(bits, H, W, scale, sums, wb, st, RH, RW, debug=True)
    img, median, st3 = ops.morpho_set_intensity(q, i, st2)
    for k, v in (("images", img), ("status", st3), ("width_before", ((wb[:, 1] - wb[:, 0]) / float(scale)).float()),
                 ("factor", wb[:, 5]), ("bounds_before", wb[:, :2]), ("shear_before", wb[:, 2]),
                 ("intensity_before", median)):
        _same_bits(out[k], v, k)
    assert st3.tolist() == [0] * B
    binary, got = mo.unpack_bits(bits, W * scale), mo.unpack_bits(warped, W * scale)
    pred, ww, ii, wbh = (v.cpu().numpy() for v in (x, w, i, wb))
    q, raw, img, median = (v.cpu().numpy() for v in (q, raw, img, median))
    ends = {dt: [] for dt in (np.float64, np.float32)}
    for b in range(B):
        for dt in ends:
            im = pred[b].astype(dt)
            stage = p.width_stage(binary[b], m.expand(im - im.min(), scale, dt), ww[b], scale)
            ends[dt].append([stage["left"], stage["right"]])
        assert stage["status"] == 0 and sums[b].tolist() == stage["sums"].tolist(), b
        assert (wbh[b, 2], wbh[b, 3], wbh[b, 4]) == (stage["shear"], stage["cx"], stage["cy"]), b
        assert wbh[b, 5] == ((wbh[b, 1] - wbh[b, 0]) / np.float64(scale)) / ww[b], b
        r64, r32 = (p.affine_stage(binary[b], wbh[b, 5], wbh[b, 2], wbh[b, 3], wbh[b, 4], scale, dt) for dt in ends)
        assert np.array_equal(got[b], r64[0]), (b, int((got[b] != r64[0]).sum()))
        band = 8 * np.abs(r32[1].astype(np.float64) - r64[1]).max()
        guarded = np.clip(r64[1], 0, 255) + 2.0 ** -7
        near = np.abs(guarded - np.rint(guarded)) <= band
        differ = q[b] != r64[2]
        assert np.abs(raw[b] - r64[1]).max() <= band
        assert np.abs(q[b] - r64[2]).max() <= 1 and not (differ & ~near).any(), (b, int(differ.sum()))
        assert median[b] == np.float32(p.set_intensity(q[b].astype(np.float64), None)[1]), b
        want = np.clip(q[b] * (ii[b] / median[b]), np.float32(0), np.float32(255))
        assert (np.abs(img[b] - want) <= 2 * np.spacing(np.maximum(want, np.float32(1e-30)))).all(), b
        print(f"set_width s={scale} b={b}: width {(wbh[b, 1] - wbh[b, 0]) / scale:.3f} -> {ww[b]:.3f} factor "
              f"{wbh[b, 5]:.4f}, shear {wbh[b, 2]:.3f}, median {median[b]} -> {ii[b]:.1f}; {int(near.sum())} pixels in the "
              f"band, {int(differ.sum())} differ")
    within_yardstick(f"set_width left, right s={scale}", torch.from_numpy(wbh[:, :2]), torch.tensor(ends[np.float64]),
                     torch.tensor(ends[np.float32]))


def test_intensity_given_and_not_and_status_rows():
    mo = _mo()
    x, w, i = _case(5, seed=9)
    x[2] = 0.25                                                      # a constant image: no background, status 1
    w[3] = float("nan")                                              # status 5
    w[4] = 1e-3                                                      # a factor of thousands: nothing left, status 4
    mp = mo.MorphoPerturb(scale=4)
    plain = mp.set_width(x, w)
    assert plain["status"].tolist() == [0, 0, 1, 5, 4]
    assert not plain["images"][2:].any() and (plain["images"][:2].amax((1, 2)) > 128).all()
    assert torch.equal(plain["images"], torch.floor(plain["images"]))        # quantised, not rescaled
    assert torch.isnan(plain["intensity_before"]).all()              # (no launch selected a median)
    assert torch.isnan(plain["factor"][2:4]).all() and torch.isnan(plain["width_before"][2:4]).all()
    assert float(plain["factor"][4]) > 1000
    lit = mp.set_width(x, w, i)
    assert lit["status"].tolist() == [0, 0, 1, 5, 4]
    for k in ("width_before", "factor", "bounds_before", "shear_before"):
        _same_bits(lit[k], plain[k], k)
    from morphomnist.morpho import intensity
    for b in range(2):
        assert float(lit["intensity_before"][b]) == intensity(plain["images"][b].cpu().numpy()), b
    assert torch.isnan(lit["intensity_before"][2:]).all() and not lit["images"][2:].any()
    assert not torch.equal(lit["images"][:2], plain["images"][:2]) and float(lit["images"].max()) <= 255
    with pytest.raises(ValueError, match="exceed the limit"):
        mo.MorphoPerturb(scale=16).set_width(torch.zeros(1, 33, 28, device=DEV), torch.ones(1, device=DEV))
    with pytest.raises(ValueError, match="tensor on"):
        mp.set_width(x, torch.ones(5))
    with pytest.raises(ValueError, match="bound_frac"):
        mp.set_width(x, w, bound_frac=1.0)


def test_validate_measures_the_result_and_takes_the_second_round_where_off():
    mo = _mo()
    x, w, i = _case(6, seed=4)
    mp = mo.MorphoPerturb(scale=4)
    first = mp.set_width(x, w)
    out = mp.set_width(x, w, validate=True)
    off = out["off_target"]
    assert off.dtype == torch.bool and off.any() and not off.all()   # the case holds rows of both kinds
    measured = mo.MorphoMeasure(scale=4, bound_frac=.02).measure(first["images"])
    _same_bits(out["width_after"], measured["width"], "width_after")
    bounds = measured["bounds"]
    assert torch.equal(off, ((bounds[:, 1] - bounds[:, 0]) / 4.0 - w).abs() > 1.0)
    second = mp.set_width(first["images"], w)
    _same_bits(out["images"], torch.where(off[:, None, None], second["images"], first["images"]), "images")
    _same_bits(out["status"], torch.where(off, second["status"], first["status"]), "status")
    for k in ("width_before", "factor", "bounds_before", "shear_before"):
        _same_bits(out[k], first[k], k)                              # the first round's
    lit = mp.set_width(x, w, i, validate=True)                       # the rescale comes after the selection
    from ali_hip import ops
    want, median, _ = ops.morpho_set_intensity(out["images"], i, out["status"])
    _same_bits(lit["images"], want, "images")
    _same_bits(lit["intensity_before"], median, "median")
    print(f"validate: width_after {out['width_after'].tolist()} for targets {w.tolist()}, off target {off.tolist()}")


def test_graph_capture_against_eager():
    """``set_width`` records into a HIP graph (a host read inside a capture is an error: every launch is on the one
    capturing stream) and the replay on new inputs gives the bits of a fresh eager call"""
    mo = _mo()
    x, w, i = _case(6, seed=4)
    mp = mo.MorphoPerturb(scale=4)
    eager = mp.set_width(x, w, i, validate=True)                     # (also builds the operators and the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mp.set_width(x, w, i, validate=True)
    x2, w2, _ = _case(6, seed=6)
    x.copy_(x2)
    w.copy_(w2)
    graph.replay()
    fresh = mo.MorphoPerturb(scale=4).set_width(x, w, i, validate=True)
    for k in VKEYS:
        _same_bits(captured[k], fresh[k], k)
    assert not torch.equal(captured["images"], eager["images"])


def test_generator_range_against_0_255():
    """The bitmap, its sums and so shear, cx and cy do not depend on a positive affine map of the pixel values.  The
    grey cdf does, in its last bits: 255 (x + 1) / 2 is another fp32 image.  hires carries a relative error of about
    (28 + 28 + 2) 2^-24 = 3.5e-6, a cdf entry about 1e-5 at most, and a crossing is interpolated on an interval that
    holds 1e-3 or more of the mass where a stroke begins or ends: 2e-5 / 1e-3 = 0.02 columns, bounded here by 0.05.
    Where the factor comes out the same to the bit, so does the image."""
    mo = _mo()
    x, w, i = _case(6, seed=11)
    mp = mo.MorphoPerturb(scale=4)
    a, b = mp.set_width(x, w, i), mp.set_width(255 * (x + 1) / 2, w, i)
    for k in ("status", "shear_before"):
        _same_bits(a[k], b[k], k)
    assert a["status"].tolist() == [0] * 6
    gap = (a["bounds_before"] - b["bounds_before"]).abs().max().item()
    same = a["factor"] == b["factor"]
    print(f"-1 .. 1 against 0 .. 255: left and right differ by at most {gap:.3g} columns; {int(same.sum())} of 6 factors "
          f"hold the same bits; {int((a['images'] != b['images']).sum())} pixels differ")
    assert gap <= 0.05
    _same_bits(a["images"][same], b["images"][same], "images")
    _same_bits(a["intensity_before"][same], b["intensity_before"][same], "median")


def test_round_trip_through_measure_batch():
    """``measure_batch`` on the result: a row that ``validate`` found on target measures within the reference's tolerance
    of 1 pixel of it -- the width column is the check's own ``width_after``; the others are printed (the reference
    promises no more of one re-application)."""
    from morphomnist.measure import measure_batch
    mo = _mo()
    x, w, _ = _case(6, seed=4)
    out = mo.MorphoPerturb(scale=4).set_width(x, w, validate=True)
    assert out["status"].tolist() == [0] * 6
    table = measure_batch(out["images"], scale=4, bound_frac=.02)
    got = torch.from_numpy(table["width"].to_numpy()).to(DEV)
    assert torch.isfinite(got).all()
    on = ~out["off_target"]
    assert on.any()
    assert torch.equal(got[on].float(), out["width_after"][on])
    assert ((got[on] - w[on]).abs() <= 1.0).all()
    for b in range(6):
        print(f"round trip {b}: width {float(out['width_before'][b]):.3f} -> target {float(w[b]):.3f}, measured "
              f"{float(got[b]):.3f}{' (re-applied)' if out['off_target'][b] else ''}")
