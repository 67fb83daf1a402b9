"""``ops.morpho_width`` and ``ops.morpho_affine_reduce`` (csrc/morpho.hip: ali_morpho_width, ali_morpho_affine_reduce) on
the device against the statement ``morphomnist.perturb.width_stage`` / ``affine_stage``.

  sums, shear, cx, cy   exactly the statement's on the device's own bitmap (integers, and fp64 formed in one order).
  hcdf, left, right     against the statement under those moments, with the yardstick of
                        ``test_gpu_morpho_bounds_kernels.py``: the reference is the fp64 statement on the images the
                        device reads, the yardstick the same statement with the up-sampling product in fp32 and the
                        rest in fp64.  The crossing intervals are the statement's exactly, each location is
                        ``quantile_loc`` of the device's own cdf bit for bit, and the factor is formed from the device's
                        own left and right bit for bit.
  warped                exactly the statement continued from the device's wb; raw to the yardstick; q bit for bit the
                        quantised raw and within the rounding band of the fp64 statement's, as the perturb kernels'.

Targets: each image's own width (measured by the statement at scale <= 4) times a factor of ``FACTORS`` by row.
Shapes: ``mc.SMALL`` with B in {1, 3, 70}; 28 x 28 at 16 with B = 3 (T in LDS); 32 x 32 at 16 with B = 2 (T in the
workspace); 12 x 20 at 4."""
import numpy as np
import pytest
import torch

import morpho_cases as mc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAC = .02
FACTORS = (0.6, 0.8, 1.0, 1.25, 1.5)
SHAPES = [(H, W, s, B) for (H, W, s) in mc.SMALL for B in mc.BATCHES] + [(28, 28, 16, 3), (32, 32, 16, 2), (12, 20, 4, 3)]
LEVELS = ((0, FRAC / 2, "left"), (1, 1 - FRAC / 2, "right"))


def _ops():
    from ali_hip import ops
    return ops


def _p():
    from morphomnist import perturb
    return perturb


def _m():
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


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _interval(c, f, side):
    """the interval j where c crosses f upward, first or last (-1: f below c[0]; len(c) - 1: f at or above c[-1])"""
    p = np.concatenate([[-np.inf], c, [np.inf]])
    hits = [j - 1 for j in range(len(p) - 1) if p[j] <= f < p[j + 1]]
    return hits[0] if side == "left" else hits[-1]


def targets_for(x, s):
    """float64 [B]: each image's own width by the statement (at scale min(s, 4): cheap, and the same to a fraction of a
    pixel) times FACTORS by row"""
    m = _m()
    return np.array([m.measure_bounds(im.astype(np.float64), min(s, 4), FRAC)["width"] * FACTORS[b % len(FACTORS)]
                     for b, im in enumerate(x)])


def launch_width(x32, s, target, bits=None, fg=None, ws=None):
    """binarise (unless a bitmap is given) and ``morpho_width`` twice: (bits, fg, sums, wb, status, hcdf), tensors"""
    ops, mo = _ops(), _mo()
    B, H, W = x32.shape
    AH, AW = mo.MorphoMeasure(scale=s).operators(H, W, torch.device(DEV))
    x = _dev(x32, np.float32)
    if bits is None:
        bits, fg, _ = ops.morpho_binarise(x, s, AH, AW)
    out = _twice(lambda: ops.morpho_width(x, s, bits, fg, _dev(target, np.float64), AH, AW, FRAC, ws=ws, debug=True))
    plain = ops.morpho_width(x, s, bits, fg, _dev(target, np.float64), AH, AW, FRAC, ws=ws)   # without the test output
    for u, v in zip(out, plain):
        assert torch.equal(u.view(torch.int64) if u.element_size() == 8 else u, v.view(torch.int64)
                           if v.element_size() == 8 else v)
    return (bits, fg, *out)


_CACHE = {}


def case(H, W, s, B):
    """one launch per shape and the statement continued from the device's bitmap, computed once: (x32, target, binary,
    tensors of ``launch_width``, rows), rows[b] = {dtype: ``width_stage``} on hires in that dtype"""
    key = (H, W, s, B)
    if key not in _CACHE:
        m, p, mo = _m(), _p(), _mo()
        x32 = mc.image_batch(B, H, W).astype(np.float32)
        target = targets_for(x32, s)
        dev = launch_width(x32, s, target)
        binary = mo.unpack_bits(dev[0], W * s)
        rows = []
        for b, im in enumerate(x32):
            h = {dt: m.expand(im.astype(dt) - im.astype(dt).min(), s, dt) for dt in (np.float64, np.float32)}
            rows.append({dt: p.width_stage(binary[b], h[dt], target[b], s, FRAC, int(binary[b].all())) for dt in h})
        _CACHE[key] = (x32, target, binary, dev, rows)
    return _CACHE[key]


def test_the_statement_reaches_status_0_on_the_batch():
    """the condition the comparisons below rest on: on ``image_batch(70, 28, 28)`` at scale 4, with these targets, the
    statement alone has status 0 on at least 60 rows"""
    p = _p()
    x = mc.image_batch(70, 28, 28).astype(np.float32)
    target = targets_for(x, 4)
    ok = sum(p.width_image(im.astype(np.float64), t, scale=4, frac=FRAC)["status"] == 0 for im, t in zip(x, target))
    assert ok >= 60, ok


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_width(H, W, s, B):
    m = _m()
    x32, target, binary, (bits, fg, sums, wb, status, hcdf), rows = case(H, W, s, B)
    sums, wb, status, hcdf = (t.cpu().numpy() for t in (sums, wb, status, hcdf))
    live = np.array([r[np.float64]["status"] == 0 for r in rows])
    if (H, W, s, B) == (28, 28, 4, 70):
        assert live.sum() >= 60, int(live.sum())
    assert live.any()
    for b, r in enumerate(rows):
        want = r[np.float64]
        assert status[b] == want["status"], (b, status[b], want["status"])
        assert sums[b].tolist() == want["sums"].tolist(), b
        if not live[b]:
            assert np.isnan(wb[b]).all() and not hcdf[b].any(), b
            continue
        for k, name in ((2, "shear"), (3, "cx"), (4, "cy")):
            assert wb[b, k] == want[name], (b, name, wb[b, k], want[name])
        for k, f, side in LEVELS:
            assert _interval(hcdf[b], f, side) == _interval(want["hcdf"], f, side), (b, side)
            assert wb[b, k] == m.quantile_loc(hcdf[b], f, side), (b, side, wb[b, k])      # the device's own cdf
        assert wb[b, 5] == ((wb[b, 1] - wb[b, 0]) / np.float64(s)) / target[b], (b, wb[b, 5])
    tag = f"{H}x{W} s={s} B={B}"
    pick = lambda dt, k: torch.from_numpy(np.stack([np.atleast_1d(r[dt][k]) for r, ok in zip(rows, live) if ok]))
    within_yardstick(f"width hcdf {tag}", torch.from_numpy(hcdf[live]), pick(np.float64, "hcdf"), pick(np.float32, "hcdf"))
    for k, name in ((0, "left"), (1, "right")):
        within_yardstick(f"width {name} {tag}", torch.from_numpy(wb[live, k]), pick(np.float64, name),
                         pick(np.float32, name))


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_affine_reduce(H, W, s, B):
    ops, p, m, mo = _ops(), _p(), _m(), _mo()
    x32, target, binary, (bits, fg, sums, wb, status, _), rows = case(H, W, s, B)
    RH, RW = mo.MorphoPerturb(scale=s).reduce_operators(H, W, torch.device(DEV))
    q, st, raw, warped = _twice(lambda: ops.morpho_affine_reduce(bits, H, W, s, sums, wb, status, RH, RW, debug=True))
    q2, st2 = ops.morpho_affine_reduce(bits, H, W, s, sums, wb, status, RH, RW)            # without the test outputs
    assert torch.equal(q, q2) and torch.equal(st, st2)
    words = warped.cpu().numpy().view(np.uint32)
    if (W * s) % 32:
        assert not (words[:, :, -1] >> ((W * s) % 32)).any()         # the pad bits stay 0
    got = mo.unpack_bits(warped, W * s)
    q, st, raw, wbh, status = (t.cpu().numpy() for t in (q, st, raw, wb, status))
    stage = {dt: [p.affine_stage(binary[b], wbh[b, 5], wbh[b, 2], wbh[b, 3], wbh[b, 4], s, dt) if status[b] == 0 else
                  None for b in range(B)] for dt in (np.float64, np.float32)}
    live = status == 0
    for b in range(B):
        if not live[b]:
            assert st[b] == status[b] and not q[b].any() and not raw[b].any() and not got[b].any(), b
            continue
        want = stage[np.float64][b]
        assert np.array_equal(got[b], want[0]), (b, int((got[b] != want[0]).sum()))
        assert st[b] == (0 if want[2].max() > 0 else 4), (b, st[b])
    raw64 = np.stack([stage[np.float64][b][1] for b in range(B) if live[b]])
    raw32 = np.stack([stage[np.float32][b][1] for b in range(B) if live[b]])
    within_yardstick(f"affine_reduce raw {H}x{W} s={s} B={B}", torch.from_numpy(raw[live]), torch.from_numpy(raw64),
                     torch.from_numpy(raw32))
    assert np.array_equal(q, m.quantise_levels(raw))                 # bit for bit the quantised raw output (fp32)
    # the rounding band of the perturb kernels' tests: only a pixel whose fp64 level lies within 8 times the fp32
    # statement's worst error of an integer may come out one grey level away
    band = 8 * np.abs(raw32.astype(np.float64) - raw64).max()
    guarded = np.clip(raw64, 0, 255) + 2.0 ** -7
    near = np.abs(guarded - np.rint(guarded)) <= band
    q64 = m.quantise_levels(raw64)
    differ = q[live] != q64
    print(f"affine_reduce {H}x{W} s={s} B={B}: band {band:.3g}, {int(near.sum())} of {near.size} pixels inside it, "
          f"{int(differ.sum())} grey levels differ")
    assert band < 2.0 ** -7 / 4
    assert np.abs(q[live] - q64).max() <= 1 and not (differ & ~near).any()
    if s == 1:
        assert np.array_equal(q[live], 255.0 * np.stack([stage[np.float64][b][0] for b in range(B) if live[b]]))


def test_rows_equal_single_image_launches():
    ops, mo = _ops(), _mo()
    x32, target, _, (bits, fg, sums, wb, status, hcdf), _ = case(28, 28, 4, 70)
    RH, RW = mo.MorphoPerturb(scale=4).reduce_operators(28, 28, torch.device(DEV))
    q, st = ops.morpho_affine_reduce(bits, 28, 28, 4, sums, wb, status, RH, RW)
    for b in range(70):
        one = launch_width(x32[b:b + 1], 4, target[b:b + 1])
        for u, v in zip((bits, fg, sums, wb, status, hcdf), one):
            u = u[b:b + 1].contiguous()
            assert torch.equal(u.view(torch.int64) if u.element_size() == 8 else u,
                               v.view(torch.int64) if v.element_size() == 8 else v), b
        q1, st1 = ops.morpho_affine_reduce(one[0], 28, 28, 4, one[2], one[3], one[4], RH, RW)
        assert torch.equal(q1, q[b:b + 1]) and torch.equal(st1, st[b:b + 1]), b


def test_status_rows_and_bad_targets():
    """rows with a status among ordinary ones, each against the statement: 1 (a constant image: all foreground), 5 (a
    target of 0, below 0, NaN, infinite), 4 (an empty bitmap, one row of pixels, a constant image under a built bitmap:
    no grey mass; a factor so large that nothing is left of the result)"""
    ops, p, m, mo = _ops(), _p(), _m(), _mo()
    s, H, W = 4, 28, 28
    x32 = mc.image_batch(10, H, W).astype(np.float32)
    x32[1] = 0.4
    x32[8] = 0.0
    target = targets_for(x32, s)
    target[1] = 5.0
    target[2:6] = [0.0, -3.0, np.nan, np.inf]
    target[8] = 5.0
    target[9] = 1e-320                                            # (a denormal: the factor overflows)
    AH, AW = mo.MorphoMeasure(scale=s).operators(H, W, torch.device(DEV))
    bits, fg, _ = ops.morpho_binarise(_dev(x32, np.float32), s, AH, AW)
    binary = mo.unpack_bits(bits, W * s)
    binary[6] = False                                                # empty
    binary[7] = False
    binary[7, 40, 10:90] = True                                      # one row
    binary[8] = False
    binary[8, 30:60, 50:60] = True                                   # a built bitmap over an image without mass
    bits = mo.pack_bits(binary).to(DEV)
    fg = _dev(binary.reshape(10, -1).sum(1), np.int32)
    _, _, sums, wb, status, hcdf = launch_width(x32, s, target, bits, fg)
    RH, RW = mo.MorphoPerturb(scale=s).reduce_operators(H, W, torch.device(DEV))
    q, st = ops.morpho_affine_reduce(bits, H, W, s, sums, wb, status, RH, RW)
    want = []
    for b, im in enumerate(x32):
        im = im.astype(np.float64)
        want.append(p.width_continue_from(binary[b], m.expand(im - im.min(), s), H, W, target[b], None, s,
                                          int(binary[b].all()), np.float64, FRAC))
    assert status.tolist() == [0, 1, 5, 5, 5, 5, 4, 4, 4, 0]
    assert st.tolist() == [0, 1, 5, 5, 5, 5, 4, 4, 4, 4] == [w["status"] for w in want]
    assert np.isinf(wb[9, 5].item())
    for b in range(1, 10):
        assert not q[b].any(), b
        if b < 9:
            assert not sums[b].any() and torch.isnan(wb[b]).all() and not hcdf[b].any(), b
    assert q[0].any()


def test_refusals_before_any_launch():
    from ctypes import c_void_p

    from ali_hip import _lib
    ops, mo = _ops(), _mo()
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    a = c_void_p(t.data_ptr())
    big = 1 << 30
    width = lambda ld, B, H, W, s, AH, frac, n: lib.ali_morpho_width(a, ld, B, H, W, s, AH, a, a, a, frac, a, a, a, a, a,
                                                                     a, n, None)
    assert width(33 * 28, 1, 33, 28, 16, a, .02, big) != 0           # side > 512
    for frac in (0.0, 1.0, float("nan")):
        assert width(64, 1, 8, 8, 2, a, frac, big) != 0              # bound_frac
    assert width(64, 0, 8, 8, 2, a, .02, big) != 0                   # B < 1
    assert width(63, 1, 8, 8, 2, a, .02, big) != 0                   # ld < H * W
    assert width(64, 1, 8, 8, 2, None, .02, big) != 0                # no operator
    assert width(32 * 32, 1, 32, 32, 16, a, .02, 4096 + 16) != 0     # workspace
    assert lib.ali_morpho_width(a, 64, 1, 8, 8, 2, a, a, a, a, .02, None, a, a, a, a, a, big, None) != 0   # no target
    affine = lambda B, H, W, s, RH, n: lib.ali_morpho_affine_reduce(a, a, a, a, B, H, W, s, RH, a, a, a, a, a, a, n, None)
    assert affine(1, 33, 28, 16, a, big) != 0
    assert affine(0, 8, 8, 2, a, big) != 0
    assert affine(1, 8, 8, 2, None, big) != 0
    assert affine(1, 8, 8, 2, a, 4096 + 16) != 0                     # workspace
    assert lib.ali_morpho_affine_reduce(a, a, a, a, 1, 8, 8, 2, a, a, a, a, a, None, a, big, None) != 0    # no status_out
    torch.cuda.synchronize()
    assert not t.any()                                               # nothing ran
    AH, AW = mo.MorphoMeasure(scale=2).operators(8, 8, torch.device(DEV))
    x = torch.zeros(1, 8, 8, device=DEV)
    bits, fg = torch.zeros(1, 16, 1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    tgt = torch.ones(1, dtype=torch.float64, device=DEV)
    for frac in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="bound_frac"):
            ops.morpho_width(x, 2, bits, fg, tgt, AH, AW, frac)
    with pytest.raises(ValueError, match="expand operator"):
        ops.morpho_width(x, 2, bits, fg, tgt, None, None)
    with pytest.raises(ValueError, match="exceed the limit"):
        ops.morpho_width(torch.zeros(1, 33, 28, device=DEV), 16, bits, fg, tgt, AH, AW)
    with pytest.raises(ValueError, match="reduce operator"):
        ops.morpho_affine_reduce(bits, 8, 8, 2, torch.zeros(1, 6, dtype=torch.int64, device=DEV),
                                 torch.zeros(1, 6, dtype=torch.float64, device=DEV), fg)
