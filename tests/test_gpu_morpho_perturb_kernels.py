"""The three perturbation kernels of csrc/morpho.hip on the device, stage by stage, against the statement
``morphomnist.perturb``: ``ops.morpho_reshape`` (bitmap, radius, moment sums and status exactly), ``ops.morpho_shear_reduce``
(shifts and warped bitmap exactly, the raw reduce to the yardstick of ``flow_cases.within_yardstick``, the quantised
image bit for bit from the device's own raw and within the rounding band of the fp64 statement's) and
``ops.morpho_set_intensity`` (median exactly, the product to 2 ulp).

Shapes: those of tests/test_gpu_morpho_kernels.py -- 5 x 9 at scales 1, 2, 4 (up-sampled widths 9, 18, 36: no multiple of
a bitmap word) and 28 x 28 at scale 4 with B in {1, 3, 70}; 28 x 28 at scale 16 with B = 3.  Every call is made twice and
must give the same bits."""
import numpy as np
import pytest
import torch

import morpho_cases as mc
import perturb_cases as pc
from flow_cases import within_yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(H, W, s, B) for (H, W, s) in mc.SMALL for B in mc.BATCHES] + [(28, 28, 16, 3)]
MAX_R = 9                                                            # of the small shapes' half-width table
SHEARS = (0.0, 0.31, -0.31, 0.9, -0.9, 1000.0)                       # the last pushes every row off the canvas


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
        bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[u.element_size()]
        assert torch.equal(u.view(bits), v.view(bits))               # (bits: a NaN equals itself)
    return a


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ reshape
def _check_reshape(name, images, thick, target, scale, table, status_in=None):
    """``ops.morpho_reshape`` on built bitmaps against ``perturb.reshape_stage`` fed the same fp32 thickness and target"""
    ops, p, mo = _ops(), _p(), _mo()
    B, Hh, Wh = images.shape
    max_radius = table.shape[0] - 1
    status_in = np.zeros(B, dtype=np.int32) if status_in is None else status_in
    bits = mo.pack_bits(images).to(DEV)
    values = torch.zeros(B, 5, device=DEV)                           # the thickness as ``morpho_measure`` leaves it:
    values[:, 2] = _dev(thick, np.float32)                           # a column of pitch 5
    tgt = None if target is None else _dev(target, np.float32)
    out, radius, sums, status = _twice(lambda: ops.morpho_reshape(bits, Wh, values[:, 2], tgt, _dev(status_in, np.int32),
                                                                  _dev(table, np.int16), scale))
    got = mo.unpack_bits(out, Wh)
    words = out.cpu().numpy().view(np.uint32)
    if Wh % 32:
        assert not (words[:, :, -1] >> (Wh % 32)).any(), name        # the pad bits stay 0
    seen = []
    for b in range(B):
        want = p.reshape_stage(images[b], thick[b], None if target is None else target[b], scale, int(status_in[b]),
                               max_radius)
        assert int(radius[b]) == want[1] and int(status[b]) == want[3], (name, b, int(radius[b]), int(status[b]), want[1:])
        assert np.array_equal(got[b], want[0]), (name, b, want[1], int((got[b] != want[0]).sum()))
        assert sums[b].tolist() == want[2].tolist(), (name, b)
        seen.append((want[1], want[3]))
    return seen


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_reshape_built_images(H, W, s, B):
    """radii 0, +-1, +-2, +-5, +-max_radius and beyond it, on blobs, a hole, a frame and bars touching the border,
    one-pixel lines, one pixel (erosion removes it: status 4) and the empty image (status 4)"""
    p = _p()
    images = pc.built(H * s, W * s, B)
    if s == 16:                                                      # 448 x 448: the family's limit of 64
        table = pc.sparse_table(64, (0, 2, 64))
        thick = np.full(3, 2.5, dtype=np.float32)
        target = (2.5 + np.array([1, -1, 1]) * 2 * (np.array([64, 64, 2]) + 0.5) / 16).astype(np.float32)
        want = [64, -64, 2]
    else:
        table = p.half_width_table(MAX_R)
        thick, target, want = pc.radius_targets(B, s, MAX_R)
    seen = _check_reshape(f"reshape {H}x{W} s={s} B={B}", images, thick, target, s, table)
    assert [r for r, _ in seen] == list(want)
    if B == 70:
        assert {st for _, st in seen} == {0, 3, 4}
        _check_reshape(f"reshape {H}x{W} s={s} no target", images[:5], thick[:5], None, s, table)
        st_in = np.array([0, 1, 2, 0, 1], dtype=np.int32)            # a status passes through, the image is 0
        again = _check_reshape(f"reshape {H}x{W} s={s} status", images[:5], thick[:5], target[:5], s, table, st_in)
        assert [st for _, st in again][1:3] == [1, 2]
        nan = thick[:5].copy()
        nan[1] = np.nan                                              # no skeleton: no thickness
        assert _check_reshape(f"reshape {H}x{W} s={s} NaN", images[:5], nan, target[:5], s, table)[1] == (0, 4)


def test_reshape_total_erosion_and_a_full_image():
    """a bar 5 wide under erosion by 5 is gone (status 4); a full image stays full under any erosion (the outside does
    not constrain it) and under dilation"""
    p = _p()
    images = np.zeros((3, 40, 70), dtype=bool)
    images[0, 5:35, 30:35] = True
    images[1:] = True
    thick = np.full(3, 4.0, dtype=np.float32)
    target = np.array([4.0 - 2 * 5.5 / 4, 4.0 - 2 * 9.5 / 4, 4.0 + 2 * 9.5 / 4], dtype=np.float32)
    seen = _check_reshape("reshape corners", images, thick, target, 4, p.half_width_table(MAX_R))
    assert seen == [(-5, 4), (-9, 0), (9, 0)]


# ------------------------------------------------------------------------------------------------------- shear, reduce
def _shear_case(H, W, s, B):
    """built bitmaps through ``perturb.reshape_stage`` (radius 0: their sums and status) and the statement's shear stage
    in fp64 and fp32"""
    p = _p()
    images = pc.built(H * s, W * s, B)
    rows = []
    for b in range(B):
        bitmap, _, sums, status = p.reshape_stage(images[b], 1.0, None, s)
        shear = SHEARS[b % len(SHEARS)]
        st = {dt: p.shear_stage(bitmap, sums, shear, s, dt) if status == 0 else None for dt in (np.float64, np.float32)}
        rows.append((bitmap, sums, status, shear, st))
    return rows


@pytest.mark.parametrize("H,W,s,B", SHAPES)
def test_shear_reduce(H, W, s, B):
    ops, p, m, mo = _ops(), _p(), _m(), _mo()
    rows = _shear_case(H, W, s, B)
    Hh, Wh = H * s, W * s
    live = np.array([r[2] == 0 for r in rows])
    # the reference alone: at most 0.5 % of the batch's pixels lie inside the band of an integer grey level
    raw64 = np.stack([r[4][np.float64][3] if r[2] == 0 else np.zeros((H, W)) for r in rows])
    raw32 = np.stack([r[4][np.float32][3] if r[2] == 0 else np.zeros((H, W), dtype=np.float32) for r in rows])
    band = 8 * np.abs(raw32.astype(np.float64) - raw64).max()
    guarded = np.clip(raw64, 0, 255) + 2.0 ** -7
    near = np.abs(guarded - np.rint(guarded)) <= band
    q64 = m.quantise_levels(raw64)
    assert band < 2.0 ** -7 / 4 and near.sum() <= 0.005 * near.size, (band, int(near.sum()), near.size)

    mp = mo.MorphoPerturb(scale=s)
    RH, RW = mp.reduce_operators(H, W, torch.device(DEV))
    bits = mo.pack_bits(np.stack([r[0] for r in rows])).to(DEV)
    sums = _dev(np.stack([r[1] for r in rows]), np.int64)
    status = _dev([r[2] for r in rows], np.int32)
    target = _dev([r[3] for r in rows], np.float64)
    q, shear, raw, shifts = _twice(lambda: ops.morpho_shear_reduce(bits, H, W, s, sums, target, status, RH, RW,
                                                                   debug=True))
    q2, shear2 = ops.morpho_shear_reduce(bits, H, W, s, sums, target, status, RH, RW)      # without the test outputs
    assert torch.equal(q, q2) and torch.equal(shear[torch.from_numpy(live).to(DEV)],
                                              shear2[torch.from_numpy(live).to(DEV)])
    q, shear, raw, shifts = (t.cpu().numpy() for t in (q, shear, raw, shifts))
    off_canvas = 0
    for b, (bitmap, _, st, _, stage) in enumerate(rows):
        if st:
            assert not q[b].any() and not raw[b].any() and not shifts[b].any() and np.isnan(shear[b]), b
            continue
        want_shear, want_shifts, want_warped = stage[np.float64][:3]
        assert shear[b] == want_shear, (b, shear[b], want_shear)
        assert np.array_equal(shifts[b], want_shifts), (b, int((shifts[b] != want_shifts).sum()))
        assert np.array_equal(p.shift_rows(bitmap, shifts[b]), want_warped), b
        off_canvas += not want_warped.any()
    if B >= 6:
        assert off_canvas >= 1                                       # the shear of 1000 leaves an empty canvas, q = 0
    within_yardstick(f"shear_reduce raw {H}x{W} s={s} B={B}", torch.from_numpy(raw[live]), torch.from_numpy(raw64[live]),
                     torch.from_numpy(raw32[live]))
    assert np.array_equal(q, m.quantise_levels(raw))                 # bit for bit the quantised raw output (fp32)
    differ = q != q64
    print(f"shear_reduce {H}x{W} s={s} B={B}: band {band:.3g}, {int(near.sum())} of {near.size} pixels inside it, "
          f"{int(differ.sum())} grey levels differ")
    assert np.abs(q - q64).max() <= 1 and not (differ & ~near).any()


def test_shear_reduce_without_a_target_is_the_reduce():
    ops, p, mo = _ops(), _p(), _mo()
    rows = _shear_case(28, 28, 4, 3)
    mp = mo.MorphoPerturb(scale=4)
    RH, RW = mp.reduce_operators(28, 28, torch.device(DEV))
    bits = mo.pack_bits(np.stack([r[0] for r in rows])).to(DEV)
    sums, status = _dev(np.stack([r[1] for r in rows]), np.int64), _dev([r[2] for r in rows], np.int32)
    q, _, raw, shifts = ops.morpho_shear_reduce(bits, 28, 28, 4, sums, None, status, RH, RW, debug=True)
    assert not shifts.any()
    for b, r in enumerate(rows):
        want = p.shear_stage(r[0], r[1], None, 4)
        within_yardstick(f"plain reduce {b}", raw[b], torch.from_numpy(want[3]),
                         torch.from_numpy(p.shear_stage(r[0], r[1], None, 4, np.float32)[3]))


# ---------------------------------------------------------------------------------------------------------- intensity
@pytest.mark.parametrize("H,W", [(2, 4), (5, 9), (28, 28)])
def test_set_intensity(H, W):
    """the median of the upper half exactly (odd and even counts, ties); the product within 2 ulp of the fp32 formula on
    the device's own q; a target that makes every pixel clip; an image of zeros gets status 4; a status passes through"""
    ops, p = _ops(), _p()
    g = np.random.default_rng(H * W)
    ims = [g.integers(0, 256, size=(H, W)), g.integers(0, 8, size=(H, W)) * 32, g.integers(100, 103, size=(H, W)),
           np.full((H, W), 17), np.zeros((H, W)), g.integers(0, 256, size=(H, W)), g.integers(0, 256, size=(H, W))]
    for k in (4, 5):                                                 # an even and an odd count, for certain
        im = np.zeros(H * W)
        im[:k] = 200 + np.arange(k)
        ims.append(im.reshape(H, W))
    if (H, W) == (2, 4):
        ims += [np.array([[0, 10, 6, 8], [1, 2, 9, 5]]), np.array([[0, 10, 6, 8], [1, 2, 9, 3]])]
    q = np.stack(ims).astype(np.float32)
    B = len(q)
    target = g.uniform(60, 250, size=B).astype(np.float32)
    target[5] = 1e6                                                  # every pixel above 0 clips to 255
    st_in = np.zeros(B, dtype=np.int32)
    st_in[6] = 3
    qd = _dev(q, np.float32)
    out, median, status = _twice(lambda: ops.morpho_set_intensity(qd, _dev(target, np.float32), _dev(st_in, np.int32)))
    out, median = out.cpu().numpy(), median.cpu().numpy()
    assert status.tolist() == [0, 0, 0, 0, 4, 0, 3] + [0] * (B - 7)
    n_sel = []
    for b in range(B):
        if status[b] != 0:
            assert not out[b].any() and np.isnan(median[b])
            continue
        want = p.set_intensity(q[b].astype(np.float64), None)[1]
        assert median[b] == np.float32(want), (b, median[b], want)
        n_sel.append(int((q[b] >= q[b].min() + (q[b].max() - q[b].min()) * .5).sum()))
        ref = np.clip(q[b] * (target[b] / median[b]), np.float32(0), np.float32(255))      # fp32 throughout
        assert ref.dtype == np.float32
        assert (np.abs(out[b] - ref) <= 2 * np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))).all(), b
    assert {n % 2 for n in n_sel} == {0, 1}, n_sel
    assert set(np.unique(out[5]).tolist()) <= {0.0, 255.0}
    plain, med2, _ = ops.morpho_set_intensity(qd, None, _dev(st_in, np.int32))
    assert torch.equal(plain[:4], qd[:4]) and torch.equal(med2.view(torch.int32), torch.from_numpy(median).to(DEV).view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- limits
def test_limits():
    """each argument error returns its code without a launch"""
    from ctypes import c_void_p
    from ali_hip import _lib
    ops, p = _ops(), _p()
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    a = c_void_p(t.data_ptr())
    big = 1 << 30
    assert lib.ali_morpho_reshape(a, a, 1, a, a, a, 4, 1, 513, 8, 1, a, a, a, a, a, big, None) != 0     # side > 512
    assert lib.ali_morpho_reshape(a, a, 1, a, a, a, 65, 1, 8, 8, 1, a, a, a, a, a, big, None) != 0      # max_radius > 64
    assert lib.ali_morpho_reshape(a, a, 1, a, a, a, 4, 0, 8, 8, 1, a, a, a, a, a, big, None) != 0       # B < 1
    assert lib.ali_morpho_reshape(a, a, 1, a, a, None, 4, 1, 8, 8, 1, a, a, a, a, a, big, None) != 0    # no table
    assert lib.ali_morpho_reshape(a, a, 1, a, a, a, 4, 1, 8, 8, 1, a, a, a, a, a, 4096 + 16, None) != 0  # workspace
    assert lib.ali_morpho_shear_reduce(a, a, a, a, 1, 33, 28, 16, a, a, a, a, a, a, a, big, None) != 0  # side > 512
    assert lib.ali_morpho_shear_reduce(a, a, a, a, 1, 8, 8, 2, None, a, a, a, a, a, a, big, None) != 0  # no operator
    assert lib.ali_morpho_shear_reduce(a, a, a, a, 1, 8, 8, 2, a, a, a, a, a, a, a, 4096 + 16, None) != 0
    assert lib.ali_morpho_set_intensity(a, a, a, 0, 8, a, a, a, None) != 0
    assert lib.ali_morpho_set_intensity(a, a, a, 1, 512 * 512 + 1, a, a, a, None) != 0
    assert lib.ali_morpho_set_intensity(a, a, None, 1, 8, a, a, a, None) != 0
    assert not t.any()                                               # nothing ran
    bits = torch.zeros(1, 8, 1, dtype=torch.int32, device=DEV)
    one = torch.zeros(1, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="max_radius"):
        ops.morpho_reshape(bits, 9, one, None, st, torch.zeros(66, 131, dtype=torch.int16, device=DEV), 1)
    with pytest.raises(ValueError, match="words per row"):
        ops.morpho_reshape(bits, 40, one, None, st, _dev(p.half_width_table(2), np.int16), 1)
    with pytest.raises(ValueError, match="exceed the limit"):
        ops.morpho_shear_reduce(bits, 33, 28, 16, torch.zeros(1, 6, dtype=torch.int64, device=DEV), None, st)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.morpho_reshape(bits, 9, one, None, st, _dev(p.half_width_table(2), np.int16), 1,
                           ws=torch.zeros(4096 + 16, dtype=torch.uint8, device=DEV))
