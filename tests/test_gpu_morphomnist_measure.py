"""``MorphoMeasure(bound_frac=...)`` and ``measure_batch`` of a CUDA tensor, end to end, at scale 4 with
B = 70 and at scale 16 with B = 3: the old columns unchanged, the new ones from the device's own bounds, the bounds
against the statement continued from the device's shear and middle (``flow_cases.within_yardstick``; the yardstick is
the statement with the up-sampling product in fp32), chunks, graph capture, ``table()`` and the Generator's range."""
import types

import numpy as np
import pytest
import torch

import morpho_cases as mc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAC = .02
CASES = [(4, 70), (16, 3)]
OLD = ("thickness", "intensity", "slant", "area", "length", "slant_hires", "counts", "status")
NEW = ("width", "height", "slant_measure", "bounds", "corners")


def _mo():
    from ali_hip import morpho
    return morpho


def _same_bits(a, b, name):
    assert a.dtype == b.dtype and a.shape == b.shape, name
    bits = {4: torch.int32, 8: torch.int64}[a.element_size()]
    assert torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)), name


_CACHE = {}


def _case(s, B):
    """(x [B, 28, 28] fp32 on the device in 0 .. 255, the output of MorphoMeasure(bound_frac) on it)"""
    if (s, B) not in _CACHE:
        x = torch.from_numpy(255 * (mc.generator_images(B, seed=s) + 1) / 2).to(DEV)
        _CACHE[(s, B)] = x, _mo().MorphoMeasure(scale=s, bound_frac=FRAC).measure(x)
    return _CACHE[(s, B)]


@pytest.mark.parametrize("s,B", CASES)
def test_old_columns_and_new_ones_from_the_bounds(s, B):
    x, out = _case(s, B)
    plain = _mo().MorphoMeasure(scale=s).measure(x)
    assert set(plain) == set(OLD) and set(out) == set(OLD) | set(NEW)
    for k in OLD:
        _same_bits(out[k], plain[k], k)
    b = out["bounds"].cpu().numpy()
    assert out["bounds"].dtype == torch.float64 and b.shape == (B, 6) and out["corners"].shape == (B, 4, 2)
    for k, want in (("width", (b[:, 1] - b[:, 0]) / s), ("height", (b[:, 3] - b[:, 2]) / s),
                    ("slant_measure", np.arctan(-b[:, 4]))):
        assert out[k].dtype == torch.float32
        assert np.array_equal(out[k].cpu().numpy(), want.astype(np.float32)), k
    from morphomnist.morpho import corners_of
    want = np.stack([np.stack(corners_of(*row)) for row in b])
    assert np.array_equal(out["corners"].cpu().numpy(), want)


@pytest.mark.parametrize("s,B", CASES)
def test_bounds_against_the_continued_statement(s, B):
    from morphomnist import morpho as m
    x, out = _case(s, B)
    b = out["bounds"].cpu().numpy()
    host = x.cpu().numpy()
    ref, f32 = [], []
    for i, im in enumerate(host):
        dev = types.SimpleNamespace(centroid=(np.nan, b[i, 5]), horizontal_shear=b[i, 4])
        for dt, acc in ((np.float64, ref), (np.float32, f32)):
            img = im.astype(dt)
            acc.append([float(v) for v in m.bounds_of(m.expand(img - img.min(), s, dt), FRAC, dev)[:4]])
    within_yardstick(f"measure bounds s={s} B={B}", torch.from_numpy(b[:, :4]), torch.tensor(ref), torch.tensor(f32))


@pytest.mark.parametrize("s,B", CASES)
def test_chunks_and_graph_capture(s, B):
    mo = _mo()
    x, out = _case(s, B)
    chunked = mo.MorphoMeasure(scale=s, bound_frac=FRAC, chunk=16 if B > 16 else 2).measure(x)
    for k in OLD + NEW:
        _same_bits(chunked[k], out[k], k)
    mm = mo.MorphoMeasure(scale=s, bound_frac=FRAC, chunk=16 if B > 16 else 2)
    y = x.clone()
    mm.measure(y)                                                     # (builds the operators and the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mm.measure(y)
    y.copy_(x.flip(0))
    graph.replay()
    fresh = mo.MorphoMeasure(scale=s, bound_frac=FRAC).measure(x.flip(0))
    for k in OLD + NEW:
        _same_bits(captured[k], fresh[k], k)


@pytest.mark.parametrize("s,B", CASES)
def test_table_and_measure_batch(s, B):
    import pandas as pd

    from morphomnist.measure import measure_batch
    mo = _mo()
    x, out = _case(s, B)
    mm = mo.MorphoMeasure(scale=s, bound_frac=FRAC)
    mm.measure(x)
    tab = mm.table()
    for k in ("width", "height", "slant_measure"):
        assert np.array_equal(tab[k], out[k].cpu().numpy().astype(np.float64)), k
    assert np.array_equal(tab["bounds"], out["bounds"].cpu().numpy())
    assert np.array_equal(tab["corners"], out["corners"].cpu().numpy())
    frame = measure_batch(x, scale=s, bound_frac=FRAC)
    assert list(frame.columns) == ["area", "length", "thickness", "slant", "width", "height"]
    want = pd.DataFrame({"area": tab["area"], "length": tab["length"], "thickness": tab["thickness"],
                         "slant": tab["slant_measure"], "width": tab["width"], "height": tab["height"]})
    assert frame.equals(want)


@pytest.mark.parametrize("s,B", CASES)
def test_generator_range_against_0_255(s, B):
    """both inputs against the fp64 statement on the same image; the yardstick is the statement with the up-sampling
    product in fp32 on that input"""
    from morphomnist import morpho as m
    mo = _mo()
    pred = mc.generator_images(B, seed=s)
    x = torch.from_numpy(pred).to(DEV)
    y = 255 * (x + 1) / 2
    ref = [m.measure_bounds(p.astype(np.float64), s, FRAC) for p in pred]
    for name, inp in (("-1 .. 1", x), ("0 .. 255", y)):
        got = mo.MorphoMeasure(scale=s, bound_frac=FRAC).measure(inp)
        f32 = [m.measure_bounds(im, s, FRAC, np.float32) for im in inp.cpu().numpy()]
        for k, rk in (("width", "width"), ("height", "height"), ("slant_measure", "slant")):
            within_yardstick(f"{name} {k} s={s}", got[k], torch.tensor([float(r[rk]) for r in ref]),
                             torch.tensor([float(r[rk]) for r in f32]))
