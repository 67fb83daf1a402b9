"""``ali_hip.morpho.MorphoLocal`` on the device, end to end: every kind and a mixed ``kind`` tensor against the statement
``morphomnist.perturb.local_continue_from`` continued from the device's own bitmap, distance map, skeleton and fp32
thickness; the low-resolution image to the family's yardstick and bit for bit from the device's own raw; chunks, the
counter, a fresh executor, a HIP graph, status rows, and the Generator's range against 0 .. 255."""
import gc

import numpy as np
import pytest
import torch

import local_cases as lc
import morpho_cases as mc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mo():
    from ali_hip import morpho
    return morpho


def _same(a, b, name=""):
    for k in _mo().LOCAL_KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (name, k)
        assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), (name, k)  # (NaN)


def _intermediates(mp, x, scale):
    from ali_hip import ops
    mo = _mo()
    B, H, W = x.shape
    mm = mp.measure
    AH, AW = mm.operators(H, W, x.device)
    bits, fg, hstats = ops.morpho_binarise(x, scale, AH, AW, 0.5)
    d2, st = ops.morpho_edt(bits, W * scale)
    skel = ops.morpho_thin(bits, d2, fg, st, mm._keep, mp.seed)
    _, values, _ = ops.morpho_measure(x, scale, skel, d2, fg, hstats, st)
    return bits, d2, skel, values[:, 2], st, (mo.unpack_bits(bits, W * scale), d2.cpu().numpy(),
                                              mo.unpack_bits(skel, W * scale), values[:, 2].cpu().numpy(),
                                              st.cpu().numpy())


@pytest.mark.parametrize("scale,B", [(4, 6), (16, 3)])
def test_every_kind_against_the_statement(scale, B):
    from ali_hip import ops
    mo = _mo()
    H = W = 28
    x = torch.from_numpy(mc.generator_images(B, seed=3 + scale)).to(DEV)
    mp = mo.MorphoLocal(scale=scale, seed=2)
    mixed = torch.tensor([(b + 1) % 5 for b in range(B)], dtype=torch.int32, device=DEV)
    *_, host = _intermediates(mp, x, scale)
    RH, RW = mp.reduce_operators(H, W, x.device)
    for call, kind in enumerate(lc.KINDS + (mixed,)):
        out = mp.apply(x, kind)
        kd = np.full(B, lc.KINDS.index(kind)) if isinstance(kind, str) else kind.cpu().numpy()
        want = {dt: lc.statement_rows(*host[:4], host[4], kd, H, W, scale, seed=2, counter=call, dtype=dt)
                for dt in (np.float64, np.float32)}
        lc.compare(f"s={scale} {kind if isinstance(kind, str) else 'mixed'}", out, want[np.float64], W * scale)
        assert np.array_equal(out["thickness_before"].cpu().numpy(), host[3], equal_nan=True)
        assert out["status"].tolist() == [0] * B
        sums = torch.from_numpy(np.stack([p_sums(w["bitmap"]) for w in want[np.float64]])).to(DEV)
        q, _, raw, _ = ops.morpho_shear_reduce(out["bits"], H, W, scale, sums, None, out["status"], RH, RW, debug=True)
        assert torch.equal(q, out["images"])
        r64, r32 = (torch.from_numpy(np.stack([w["raw"] for w in want[dt]])) for dt in (np.float64, np.float32))
        within_yardstick(f"raw s={scale} call {call}", raw, r64, r32)
        lifted = torch.floor(torch.clamp(raw, 0, 255) + 2.0 ** -7)   # the quantiser on the device's own raw, in fp32
        assert lifted.dtype == torch.float32 and torch.equal(lifted, out["images"])
        assert float(out["images"].min()) >= 0 and float(out["images"].max()) <= 255
    assert int(mp.counter(x.device)) == 6


def p_sums(bitmap):
    from morphomnist import perturb
    return perturb.moment_sums(bitmap)


def test_chunks_counter_and_fresh_executor():
    mo = _mo()
    x = torch.from_numpy(mc.generator_images(5, seed=1)).to(DEV)
    kind = torch.tensor([4, 3, 4, 3, 1], dtype=torch.int32, device=DEV)
    whole = mo.MorphoLocal(scale=4, seed=9)
    first, second = whole.apply(x, kind), whole.apply(x, kind)
    assert not torch.equal(first["centres"], second["centres"])      # the counter advanced: other draws
    assert torch.equal(first["radius"], second["radius"])
    for chunk in (1, 2):
        ml = mo.MorphoLocal(scale=4, seed=9, chunk=chunk)
        _same(ml.apply(x.reshape(5, 1, 28, 28), kind), first, f"chunk {chunk}")
        _same(ml.apply(x, kind), second, f"chunk {chunk}, second call")
    other = mo.MorphoLocal(scale=4, seed=10).apply(x, kind)
    assert not torch.equal(other["centres"], first["centres"])
    for name in ("fracture", "swell"):
        a, b = mo.MorphoLocal(scale=4, seed=9).apply(x, name), mo.MorphoLocal(scale=4, seed=9, chunk=2).apply(x, name)
        _same(a, b, name)


def test_graph_capture_against_eager():
    mo = _mo()
    x = torch.from_numpy(mc.generator_images(3, seed=2)).to(DEV)
    kind = torch.tensor([4, 3, 2], dtype=torch.int32, device=DEV)
    mp = mo.MorphoLocal(scale=4, seed=4)
    mp.apply(x, kind)                                                # (builds the operators and the workspace; counter 1)
    torch.cuda.synchronize()
    gc.collect()                                                     # (no dead cycle is finalised inside the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mp.apply(x, kind)
    new = torch.from_numpy(mc.generator_images(3, seed=6)).to(DEV)
    x.copy_(new)
    graph.replay()
    fresh = mo.MorphoLocal(scale=4, seed=4)
    fresh.apply(new, kind)
    eager = fresh.apply(new, kind)                                   # the second call of a fresh executor: counter 1
    _same(captured, eager, "replay")
    assert int(mp.counter(x.device)) == 2
    graph.replay()
    _same(captured, fresh.apply(new, kind), "second replay")


def test_status_rows_and_ranges():
    mo = _mo()
    pred = mc.generator_images(4, seed=9)
    pred[2] = 0.25                                                   # a constant image: no background, status 1
    x = torch.from_numpy(pred).to(DEV)
    for kind in lc.KINDS:
        mp = mo.MorphoLocal(scale=4, seed=1)
        out = mp.apply(x, kind)
        assert out["status"].tolist() == [0, 0, 1, 0], kind
        assert not out["images"][2].any() and not out["bits"][2].any() and int(out["n_candidates"][2]) == 0
        assert (out["images"][[0, 1, 3]].amax((1, 2)) > 0).all()
        both = mo.MorphoLocal(scale=4, seed=1).apply(255 * (x + 1) / 2, kind)    # the scripts' range: the same bitmaps
        _same(out, both, kind)
    away = mo.MorphoLocal(scale=4, thin_amount=3.).apply(x, "thin")  # a radius above every distance: thinned away
    assert away["status"].tolist() == [4, 4, 1, 4] and not away["images"].any() and (away["radius"][[0, 1, 3]] > 0).all()
    odd = mo.MorphoLocal(scale=4).apply(x, torch.tensor([0, 5, 0, -1], dtype=torch.int32, device=DEV))
    assert odd["status"].tolist() == [0, 4, 1, 4]                    # a number that is no kind
    mp = mo.MorphoLocal(scale=4)
    with pytest.raises(ValueError, match="kind"):
        mp.apply(x, "swollen")
    with pytest.raises(ValueError, match="kind"):
        mp.apply(x, torch.zeros(4, dtype=torch.int32))               # on the host
    with pytest.raises(ValueError, match="kind"):
        mp.apply(x, torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="exceed the limit"):
        mo.MorphoLocal(scale=16).apply(torch.zeros(1, 33, 28, device=DEV), "plain")
