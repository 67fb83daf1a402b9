"""``ali_hip.morpho.MorphoMeasure`` on the device, end to end: chunks against single images bit for bit, the statement
``morphomnist.morpho`` continued from the device's binary images (counts exactly, values to the yardstick of
``flow_cases.within_yardstick``), the three input layouts, the Generator's range against 0 .. 255, no host read before
``table()``, and the scripts' ``extract_observed_attributes`` on the same images."""
import numpy as np
import pytest
import torch

import morpho_cases as mc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOATS = ("thickness", "intensity", "slant", "area", "length", "slant_hires")


def _mo():
    from ali_hip import morpho
    return morpho


def _same_bits(a, b, name):
    assert a.dtype == b.dtype and a.shape == b.shape, name
    bits = {4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)), name


def _slant_floor(image64):
    """The absolute error a slant may carry where its terms cancel.  The device forms the up-sampled image in fp32, so
    every pixel v carries a rounding of up to half an fp32 ulp, independent from pixel to pixel; m11 / m00 = sum(x y v)
    / sum(v) then has a standard deviation of 2^-24 sqrt(sum (x y v)^2) / m00, which survives the subtraction in u11 =
    m11 / m00 - m10 m01 whatever is left of the terms.  The floor is four of those over u02 (d atan <= 1, so it covers
    ``slant_hires`` too).  For a symmetric image (the bar, the ring) everything cancels: the reference is 0 to 1e-15,
    the fp32 statement returns -0 exactly, and ``within_yardstick`` has neither a relative floor nor a yardstick."""
    from morphomnist.morpho import ImageMoments
    v = image64 - image64.min()
    y, x = np.mgrid[:v.shape[0], :v.shape[1]]
    mo = ImageMoments(v)
    return 4 * 2.0 ** -24 * np.sqrt(((x * y * v) ** 2).sum()) / (mo.m00 * mo.u02)


def _slants(name, got, ref, f32, floors):
    """``within_yardstick`` for the entries whose error exceeds their cancellation floor; the worst ratio"""
    got, ref, f32 = (v.detach().double().cpu().reshape(-1) for v in (got, ref, f32))
    over = (got - ref).abs() > torch.tensor(floors, dtype=torch.float64)
    print(f"{name}: {int(over.sum())} of {len(over)} entries above the cancellation floor; largest error "
          f"{float((got - ref).abs().max()):.3g}")
    return within_yardstick(name, got[over], ref[over], f32[over]) if over.any() else 0.0


def _against_statement(name, mm, x, out):
    """``out`` of ``mm.measure(x)`` (x [B, H, W] fp32 on the device) against the statement continued from the binary
    images the device made"""
    from ali_hip import ops
    mo = _mo()
    B, H, W = x.shape
    AH, AW = mm.operators(H, W, x.device)
    bits, fg, _ = ops.morpho_binarise(x, mm.scale, AH, AW, mm.threshold)
    binary = mo.unpack_bits(bits, W * mm.scale)
    host = x.cpu().numpy()
    rows = {dt: [mo.statement_row(host[b].astype(dt), mm.scale, mm.threshold, mm.seed, dt, binary=binary[b])
                 for b in range(B)] for dt in (np.float64, np.float32)}
    counts = np.stack([r[0] for r in rows[np.float64]])
    assert np.array_equal(out["counts"].cpu().numpy(), counts), name
    assert out["status"].tolist() == [r[3] for r in rows[np.float64]] == [0] * B, name
    worst = 0.0
    for j, k in enumerate(("area", "length", "thickness", "intensity")):
        ref, f32 = (torch.tensor(np.array([r[1][j] for r in rows[dt]], dtype=np.float64)) for dt in rows)
        worst = max(worst, within_yardstick(f"{name} {k}", out[k], ref, f32))
    from morphomnist.morpho import expand
    host64 = host.astype(np.float64)
    ref, f32 = (torch.tensor(np.array([r[1][4] for r in rows[dt]], dtype=np.float64)) for dt in rows)
    worst = max(worst, _slants(f"{name} slant", out["slant"], ref, f32, [_slant_floor(im) for im in host64]))
    ref, f32 = (torch.tensor(np.array([r[2] for r in rows[dt]], dtype=np.float64)) for dt in rows)
    worst = max(worst, _slants(f"{name} slant_hires", out["slant_hires"], ref, f32,
                               [_slant_floor(expand(im, mm.scale)) for im in host64]))
    assert torch.equal(out["intensity"].cpu(), torch.tensor([np.float32(r[1][3]) for r in rows[np.float64]]))
    return worst, rows


def test_chunks_single_images_and_the_statement():
    """B = 70 with chunk = 32 (two chunks and a remainder of 6) at scale 4"""
    mo = _mo()
    x = torch.from_numpy(255 * (mc.generator_images(70, seed=1) + 1) / 2).to(DEV)
    mm = mo.MorphoMeasure(scale=4, chunk=32)
    out = mm.measure(x)
    again = mm.measure(x)
    whole = mo.MorphoMeasure(scale=4).measure(x)                      # the default chunk: one launch of 70
    single = mo.MorphoMeasure(scale=4)
    ones = [single.measure(x[b:b + 1]) for b in range(70)]
    for k in FLOATS + ("counts", "status"):
        _same_bits(out[k], again[k], k)
        _same_bits(out[k], whole[k], k)
        _same_bits(out[k], torch.cat([o[k] for o in ones]), k)
    assert out["thickness"].shape == (70,) and out["counts"].shape == (70, 4) and out["counts"].dtype == torch.int32
    worst, _ = _against_statement("measure 70 x 28 x 28 s=4", mm, x, out)
    print(f"MorphoMeasure B=70 scale 4: worst yardstick ratio {worst:.3g}")
    tab = mm.table()
    assert tab["thickness"].shape == (140,) and tab["counts"].shape == (140, 4)
    assert np.array_equal(tab["thickness"][:70].astype(np.float32), out["thickness"].cpu().numpy())
    assert np.array_equal(tab["counts"][70:], out["counts"].cpu().numpy().astype(np.int64))


def test_scale_16_and_the_scripts_function():
    """the scripts' loop body, ``extract_observed_attributes(255 * (pred_image + 1) / 2)`` at scale 16, written out on
    the statement, against one ``measure`` of the same images.  The statement's own binary image must be the device's
    (no pixel of these images lies in the rounding band of the threshold); then the three columns agree to the
    yardstick, the fp32 statement being the yardstick."""
    from morphomnist import morpho as m
    mo = _mo()
    pred = mc.generator_images(3, seed=7)
    imgs = 255 * (pred + 1) / 2                                       # fp32, as the scripts' tensors are
    x = torch.from_numpy(imgs).to(DEV)
    mm = mo.MorphoMeasure()                                           # scale 16, threshold .5, seed 0
    out = mm.measure(x.reshape(3, 1, 28, 28))
    worst, rows = _against_statement("measure 3 x 28 x 28 s=16", mm, x, out)
    want = []
    for b, image in enumerate(imgs.astype(np.float64)):               # mnist_gan_measured_cf.py:15-25
        morph = m.ImageMorphology(image, scale=16)
        assert int(morph.binary_image.sum()) == int(out["counts"][b, 0]), b          # the precondition on the inputs
        thickness = morph.mean_thickness
        img_min, img_max = image.min(), image.max()
        intensity = np.median(image[image >= img_min + (img_max - img_min) * .5])
        slant = -m.ImageMoments(image).horizontal_shear
        want.append([thickness, intensity, slant])
    want = np.array(want)
    for j, k in enumerate(("thickness", "intensity", "slant")):
        yard = torch.tensor(np.array([r[1][(2, 3, 4)[j]] for r in rows[np.float32]], dtype=np.float64))
        worst = max(worst, within_yardstick(f"scripts {k}", out[k], torch.from_numpy(want[:, j]), yard))
    print(f"MorphoMeasure scale 16 against extract_observed_attributes: worst yardstick ratio {worst:.3g}")


def test_layouts():
    mo = _mo()
    x = torch.from_numpy(mc.generator_images(5, seed=3)).to(DEV)
    mm = mo.MorphoMeasure(scale=4)
    a, b, c = mm.measure(x), mm.measure(x.reshape(5, 1, 28, 28)), mm.measure(x.reshape(5, 784))
    d = mm.measure(torch.stack([x, x], dim=1)[:, 1])                  # a strided view of contiguous images
    e = mm.measure(x.double())
    for k in FLOATS + ("counts", "status"):
        for other in (b, c, d, e):
            _same_bits(a[k], other[k], k)
    with pytest.raises(ValueError, match="exceed the limit"):
        mo.MorphoMeasure(scale=16).measure(torch.zeros(1, 33, 28, device=DEV))


def test_generator_range_against_0_255():
    """-1 .. 1 against 255 * (x + 1) / 2: counts, thickness, area and length are equal; the slants agree to the rounding
    of the two fp32 inputs (the yardstick: the fp32 statement); intensity maps with the images"""
    mo = _mo()
    pred = mc.generator_images(6, seed=5)
    x = torch.from_numpy(pred).to(DEV)
    y = 255 * (x + 1) / 2
    a, b = mo.MorphoMeasure(scale=4).measure(x), mo.MorphoMeasure(scale=4).measure(y)
    _same_bits(a["counts"], b["counts"], "counts")
    _same_bits(a["status"], b["status"], "status")
    for k in ("thickness", "area", "length"):
        _same_bits(a[k], b[k], k)
    from morphomnist.morpho import expand
    host = y.cpu().numpy()
    f32 = [mo.statement_row(im, 4, .5, 0, np.float32) for im in host]
    _slants("range slant", a["slant"], b["slant"].double(), torch.tensor([float(r[1][4]) for r in f32]),
            [_slant_floor(im.astype(np.float64)) for im in host])
    _slants("range slant_hires", a["slant_hires"], b["slant_hires"].double(), torch.tensor([float(r[2]) for r in f32]),
            [_slant_floor(expand(im.astype(np.float64), 4)) for im in host])
    assert torch.allclose(255 * (a["intensity"] + 1) / 2, b["intensity"], rtol=1e-6, atol=0)


def test_no_host_read_before_table():
    """``measure`` records into a HIP graph (a host read or a synchronisation inside a capture is an error) and the replay
    gives the bits of the eager call; ``table`` is the read"""
    mo = _mo()
    x = torch.from_numpy(mc.generator_images(40, seed=2)).to(DEV)
    mm = mo.MorphoMeasure(scale=4, chunk=16)
    eager = mm.measure(x)                                             # (also builds the operators and the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mm.measure(x)
    x.copy_(torch.from_numpy(mc.generator_images(40, seed=6)))
    graph.replay()
    fresh = mo.MorphoMeasure(scale=4).measure(x)
    for k in FLOATS + ("counts", "status"):
        _same_bits(captured[k], fresh[k], k)
    assert not torch.equal(captured["counts"], eager["counts"])
    tab = mm.table()
    assert tab["status"].shape == (80,) and set(tab) == set(FLOATS) | {"counts", "status"}
