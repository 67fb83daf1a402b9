"""Rectangular maps and kernels on the fp16 routes of the convolution kernels (csrc/gconv.hip, csrc/wgrad.hip):
gconv_kernel<.., 2, 1> (operands rounded to fp16 in flight), gconv_kernel<.., 2, 2> (fp16 twins read from memory, 64-deep
k-tiles), gconv_kernel512<256, 256, .., 3> (twins by LDS-DMA), wgrad_fast_kernel<.., F16 = 1 / 2> and
conv_s2_first_kernel<4 | 8, true> -- the fp16 counterpart of test_gpu_conv_geometry.py, whose Case, check, pack,
padded_nhwc and forced_tile it shares.  Every other fp16 test (test_gpu_kernels.py) hands these kernels squares.

Operand rounding is kept out of the comparison: x, w, the pre-activation gradient and the previous layer's output are
rounded to fp16 ONCE on the host; the device gets fp32 tensors that hold those values (and their fp16 twins where the
route reads twins), the reference is the layer in CPU fp64 on the same values, the yardstick the same in CPU fp32.  A
product of two fp16 values is exact in fp32, so device and yardstick differ from the reference by the rounding of their
sums alone, and the bounds are those of test_gpu_conv_geometry.py, unchanged:
    e(device) <= 4 * e(cpu fp32)        e(device) <= 2e-4 * max|ref64|
printed per output (lines ``GEOM16 case=.. out=.. e_dev=.. e_cpu=.. ratio=..``) before they are asserted.  DESIGN.md 4
has the measured ratios per route; CAP_ONLY would list an output held by the 2e-4 cap alone (none is).
The gradient stages are fed the fp16 rounding of the REFERENCE's pre-activation gradient, so that a sign tie of one
stage cannot leak into the next.

Every route also runs an EXACT leg: x in [-4, 4], w in {-2..2}/8, gpre in {-2..2}/4, bias in {-4..4}/8, LeakyReLU slopes
of 0.5 and a mask of {0, 1.25}.  Every partial sum of every output is then a multiple of its grid unit below 2^24 units
(checked on the CPU, test_exact_leg_sums_fit_fp32), i.e. exactly representable in fp32 whatever the summation order, and
the device output must EQUAL the fp64 reference cast to fp32: a wrong index is an O(1) difference, no tolerance.

The host queries (ali_conv_mtiles, ali_conv_uses_f16, ali_conv_writes_out16, ali_wgrad_deferrable) are asserted under
precision("f16") so that a change of pick_tile cannot move a case onto another route unnoticed; whether a launch reads
the twins (which no query reports) is proven by poisoning them.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv_geometry as geo
from test_gpu_conv_geometry import FORCED_TILES, RTOL, Case, check, forced_tile, nan, nchw, nhwc, pack, padded_nhwc  # noqa: F401

gpu = pytest.mark.gpu
LEGS = ("random", "exact")

# (case id, output) -> why the 4x yardstick does not apply (the 2e-4 cap still does); see DESIGN.md 4
CAP_ONLY = {}

B32 = geo.BY_ID
# case -> what the host queries say under precision("f16") at the library's own tile: fwd / bwd = ali_conv_mtiles of the
# layer's forward / data-gradient launch, uses = ali_conv_uses_f16 of the two (1: the GEMM's input channels % 32 == 0)
CASES = [
    # --- convert-in-flight GEMM (F16 = 1): geometries of test_gpu_conv_geometry.py.  uni-img's data gradient gathers 72
    # channels and ct-phase's 24: those two launches fall back to fp32 arithmetic (asserted bit for bit)
    (B32["uni-img"], dict(fwd=(3, 64, False), bwd=(6, 128, False), uses=(1, 0))),
    (B32["uni-pix"], dict(fwd=(69, 64, True), bwd=(50, 64, True), uses=(1, 1))),
    (B32["same3"], dict(fwd=(60, 64, True), bwd=(30, 128, True), uses=(1, 1))),
    (B32["ct-phase"], dict(fwd=(4, 128, False), bwd=(1, 128, False), uses=(1, 0))),
    (B32["ct-pix"], dict(fwd=(9, 128, True), bwd=(3, 64, True), uses=(1, 1))),
    # --- fall-back under f16: gathers of 6 / 20 / 8 channels keep fp32 arithmetic
    (B32["scalar"], dict(fwd=(4, 128, False), bwd=(3, 128, False), uses=(0, 0))),
    (B32["vec"], dict(fwd=(3, 64, False), bwd=(3, 128, False), uses=(0, 0))),
    (B32["pow2"], dict(fwd=(2, 128, False), bwd=(8, 128, False), uses=(0, 0))),
    # --- twins in memory (F16 = 2) and the LDS-DMA kernel (F16 = 3): C and K multiples of 64
    # image-major, 405 rows: ragged M for every tile height, K = 128 is half an N-tile of the 256 x 256 kernel
    (Case("t-img", (3, 64, 9, 14, 128, 3, 2, 1, 1)), dict(fwd=(7, 64, False), bwd=(6, 64, False), uses=(1, 1))),
    # stride 2, 5 x 3, ragged N: K = 160 = 2 * 64 + 32.  Its data gradient gathers 160 channels (no multiple of 64): that
    # launch converts in flight although both twins are there
    (Case("t-s2", (4, 64, 13, 10, 160, 5, 3, 2, 1)), dict(fwd=(2, 64, False), bwd=(10, 64, False), uses=(1, 1))),
    # transposed, four sub-pixel phases of 5 x 7 / 5 x 6 pixels with 2 x 1 / 2 x 2 / 3 x 1 / 3 x 2 taps
    (Case("t-ct", (3, 64, 4, 7, 64, 5, 3, 2, 1), kind="convT", opad=(1, 0)), dict(fwd=(8, 64, False), bwd=(2, 64, False), uses=(1, 1))),
    # pixel-major with B = 70 no multiple of any tile height, pad = R - 1 on a 2 x 3 map: taps skipped tile-wide.
    # Weight gradient: 840 pixels in 13 slabs of 96, the last four empty -- the twin-reading loop left their rows of the
    # bias-gradient slabs unwritten and the fold added what the workspace held (db came out wrong here and in `tail`,
    # 19200 pixels in 128 slabs of 160, before the kernel zeroed them)
    (Case("t-pix", (70, 64, 2, 3, 128, 3, 5, 1, 2)), dict(fwd=(14, 64, True), bwd=(7, 64, True), uses=(1, 1))),
    # --- the fp32 module's `tail` does NOT reach the tail split under f16: its forward takes 150 tiles of 128 x 128 under
    # the fp16 tile rule, its data gradient 352 of 64 x 64 -- both below 2 blocks per CU, so both launches split K over
    # ALL their tiles (plan_conv: the tail split needs S == 1).  Kept as the deep split-K case of the fp16 loops
    (B32["tail"], dict(fwd=(150, 128, True), bwd=(352, 64, True), uses=(1, 1))),
    # --- tail split under f16: 64 output channels both ways keep pick_tile at 64 x 64 and one N-tile.  Forward: 64 * 19 *
    # 30 rows = 570 blocks, 512 run whole, 58 left over; data gradient: 64 * 18 * 30 rows = 540 blocks, 28 left over;
    # both cut Sr = 2 ways along K (12 k-tiles of 32: a third cut would leave fewer than 4 each)
    (Case("tail16", (64, 64, 18, 30, 64, 2, 3, 1, 1)), dict(fwd=(570, 64, True), bwd=(540, 64, True), uses=(1, 1))),
    # --- conv_s2_first_kernel<4 | 8, true> (needs R = S = 5).  fwd / bwd speak of the general GEMM, which the forward
    # does not launch (see test_gpu_conv_geometry.py); P = 19 / 35 / 13: the last of the (P + 3) / 4 grid rows is ragged,
    # with three live rows in the first two and ONE in the third
    (B32["s2first-c4"], dict(fwd=(21, 64, False), bwd=(46, 128, False), uses=(1, 1))),
    (B32["s2first-c8"], dict(fwd=(55, 64, False), bwd=(110, 128, False), uses=(1, 1))),
    (Case("s2first-p13", (2, 3, 26, 69, 64, 5, 5, 2, 2), cpad=4), dict(fwd=(15, 64, False), bwd=(30, 128, False), uses=(1, 1))),
]
BY_ID = {c.id: c for c, _ in CASES}
ROUTE = {c.id: r for c, r in CASES}
SQUARE_OK = ("same3", "s2first-c4", "s2first-c8", "s2first-p13")       # routes / geometries that need R == S
CONVERTING = ["uni-img", "uni-pix", "same3", "ct-phase", "ct-pix"]
FALLBACK = ["scalar", "vec", "pow2"]
TWINS = ["t-img", "t-s2", "t-ct", "t-pix"]
S2FIRST = ["s2first-c4", "s2first-c8", "s2first-p13"]

# exact leg: the grid unit of every output (x integer, w /8, gpre /4, bias /8; slopes 0.5, mask 1.25 = 5/4)
GRID = {"y": 1 / 16, "dx": 1 / 32, "dx_epi": 1 / 256, "dw": 1 / 4, "db": 1 / 4}
SLOPE = {"random": (0.2, 0.1), "exact": (0.5, 0.5)}       # LeakyReLU of the layer, act' of the layer in front


def _ops():
    from ali_hip import ops
    return ops


def is_conv(c):
    return c.kind == "conv"


def gemm_cin(c):
    """input channels of the (forward, data-gradient) GEMM of the layer"""
    return (c.cpad, c.K)


# ----------------------------------------------------------------------------------------------------------------------
# references (computed once per case and leg, shared by every test; never modified)

def _inputs(c, leg):
    g = torch.Generator().manual_seed(zlib.crc32((c.id + "/f16/" + leg).encode()))
    wshape = (c.K, c.C, c.R, c.S) if is_conv(c) else (c.C, c.K, c.R, c.S)
    t = {}
    if leg == "exact":
        t["x"] = torch.randint(-4, 5, (c.B, c.C, c.H, c.W), generator=g).float()
        t["w"] = torch.randint(-2, 3, wshape, generator=g).float() / 8
        t["b"] = torch.randint(-4, 5, (c.K,), generator=g).float() / 8
        t["gpre"] = torch.randint(-2, 3, (c.B, c.K, c.P, c.Q), generator=g).float() / 4
    else:
        fan = c.C * c.R * c.S / (1 if is_conv(c) else c.stride ** 2)
        t["x"] = torch.randn(c.B, c.C, c.H, c.W, generator=g).half().float()
        t["w"] = (torch.randn(wshape, generator=g) / fan ** 0.5).half().float()
        t["b"] = torch.randn(c.K, generator=g)                       # (added in the fp32 epilogue: not an MFMA operand)
        t["gy"] = torch.randn(c.B, c.K, c.P, c.Q, generator=g)
    t["mask"] = (torch.rand(c.B, c.cpad, generator=g) > 0.3).float() * 1.25
    t["yprev_raw"] = torch.randn(c.B, c.cpad, c.H, c.W, generator=g)
    t["yprev"] = t["yprev_raw"].half().float()        # the device takes act' from the twin: the reference from the same
    return t


def _stages(c, t, dt, leg, gpre_in=None, absolute=False):
    """the layer in dtype ``dt``; gpre_in: the reference's fp16-rounded pre-activation gradient.  ``absolute``: every
    operand replaced by its modulus, no activation -- the outputs then bound every partial sum of the true ones."""
    pick = (lambda k: t[k].abs()) if absolute else (lambda k: t[k])
    x, w = (pick(k).to(dt).requires_grad_(True) for k in ("x", "w"))
    pre = geo._pre(c, x, w, pick("b").to(dt))
    slope, dslope = SLOPE[leg]
    if absolute:
        y = pre
    elif is_conv(c):
        y = F.leaky_relu(pre, slope)
    else:
        y = pre if leg == "exact" else torch.tanh(pre)
    out = {"y": y.detach()}
    if gpre_in is None:
        if leg == "exact":
            gpre_in = t["gpre"]
        else:
            yd, one = out["y"], torch.ones((), dtype=dt)
            dact = torch.where(yd > 0, one, torch.tensor(slope).to(dt)) if is_conv(c) else 1 - yd * yd
            gpre_in = (t["gy"].to(dt) * dact).float().half().float()
    gp = (gpre_in.abs() if absolute else gpre_in).to(dt)
    out["db"] = gp.sum(dim=(0, 2, 3))
    out["dx"], out["dw"] = torch.autograd.grad(pre, (x, w), gp)
    m = t["mask"][:, :c.C, None, None].to(dt)
    one = torch.ones((), dtype=dt)
    dact = one if absolute else torch.where(t["yprev"][:, :c.C] > 0, one, torch.tensor(dslope).to(dt))
    out["dx_epi"] = out["dx"] * m * dact
    return out, gpre_in


_REF = {}


def reference(c, leg):
    """{"in": inputs, "gpre_in": the gradient the backward stages consume, "ref": fp64 outputs, "f32": CPU fp32 outputs}"""
    hit = _REF.get((c.id, leg))
    if hit is None:
        t = _inputs(c, leg)
        ref, gpre_in = _stages(c, t, torch.float64, leg)
        f32, _ = _stages(c, t, torch.float32, leg, gpre_in)
        hit = _REF[(c.id, leg)] = {"leg": leg, "in": t, "gpre_in": gpre_in, "ref": ref, "f32": f32}
    return hit


def verify(c, r, name, got, what=None):
    """random leg: both bounds of the module docstring; exact leg: equality with the fp64 reference cast to fp32"""
    if r["leg"] == "random":
        check(c, r, name, got, what, prefix="GEOM16", cap_only=CAP_ONLY)
        return
    ref = r["ref"][name].float()
    got = got.detach().float().cpu()
    assert got.shape == ref.shape, (c.id, name, got.shape, ref.shape)
    diff = (got - ref).abs().max().item()
    print(f"GEOM16 case={c.id} tile={geo._tile_name()} out={what or name} leg=exact max|dev-ref|={diff:g} "
          f"grid={GRID[name]:g} max|ref|={ref.abs().max().item():g}")
    assert torch.equal(got, ref), f"{c.id} {what or name}: differs from the exact reference by {diff:g}"


# ----------------------------------------------------------------------------------------------------------------------
# routes: what the host side says about every case under precision("f16") (runs without a GPU)

def _which(c):
    """ali_conv_fwd (0) / ali_conv_bwd_data (1) that serves the layer's (forward, data gradient)"""
    return (0, 1) if is_conv(c) else (1, 0)


def uses_f16(ops, c, stage):
    import ali_hip
    geom, ep = c.geom(ops), ops.epilogue()
    return int(ali_hip.load().ali_conv_uses_f16(ctypes.byref(geom), _which(c)[stage], ctypes.byref(ep)))


def assert_route(ops, c):
    import ali_hip
    route, geom = ROUTE[c.id], c.geom(ops)
    with ops.precision("f16"):
        for stage, key in enumerate(("fwd", "bwd")):
            w = _which(c)[stage]
            assert ops.conv_mtiles(geom, w) == route[key], (c.id, key, ops.conv_mtiles(geom, w))
            assert uses_f16(ops, c, stage) == route["uses"][stage], (c.id, key, "uses_f16")
            assert ali_hip.load().ali_conv_writes_out16(ctypes.byref(geom), w) == 1, (c.id, key, "writes_out16")
        assert ops.wgrad_deferrable(geom) == 0, (c.id, "fp16 weight gradients are never deferred")
    # ali_conv_uses_f16 of the general GEMM = its gathered channels % 32 == 0 (the s2first forward is the row-walking kernel)
    if c.id not in S2FIRST:
        assert route["uses"] == tuple(int(n % 32 == 0) for n in gemm_cin(c)), c.id


CUS = 256        # kNumCU of csrc/ali_common.h


def plan16(ops, c, stage, twins=False, **env):
    """ops.conv_plan of the layer's forward (0) / data-gradient (1) launch under precision("f16"), with fp16 twins of
    both operands or without (the plan only asks whether the pointers are null)"""
    with ops.tuning(**env), ops.precision("f16"):
        ep = ops.epilogue()
        if twins:
            ep.in16 = ep.w16 = ep.out16 = 0x1000
        return ops.conv_plan(c.geom(ops), _which(c)[stage], ep)


def tail_split_ways(blocks, max_nkt):
    """Sr of plan_conv (gconv.hip) for a uniform-tap launch with a workspace and no ALI_SPLITK: 1 = no tail
    split.  The split needs S == 1, i.e. a grid the split-K rule leaves alone (at least two blocks per CU, or fewer than
    8 k-tiles), fewer than 4 blocks per CU, and R = blocks % CUs left-over tiles that fit the chip at least twice over
    with at least 4 k-tiles per piece."""
    if blocks < 2 * CUS and max_nkt >= 8:
        return 1                                    # the split-K rule's grid (S > 1 for every case here)
    if not CUS < blocks < 4 * CUS:
        return 1
    left, ways = blocks % CUS, 1
    while left > 0 and ways * 2 <= 8 and ways * 2 * left <= CUS and max_nkt // (ways * 2) >= 4:
        ways *= 2
    return ways


@pytest.mark.parametrize("cid", list(BY_ID))
def test_f16_case_takes_its_route(cid):
    """Host side only.  `tail16`: both launches meet every precondition of the tail split (tail_split_ways)."""
    ops = _ops()
    ops.reload_tuning()
    c = BY_ID[cid]
    assert_route(ops, c)
    if cid in TWINS + ["tail", "tail16"]:
        assert c.C % 64 == 0 and c.cpad == c.C and c.K % 32 == 0
    T = c.R * c.S
    if cid == "tail":       # below 2 blocks per CU: split-K over every tile, no tail split
        assert tail_split_ways(ROUTE[cid]["fwd"][0] * 1, T * c.C // 32) == 1        # (128-wide tile: one N-tile)
        assert tail_split_ways(ROUTE[cid]["bwd"][0] * ((c.C + 63) // 64), T * c.K // 32) == 1
        for stage in (0, 1):        # ... and the library's own plan says the same
            plan = plan16(ops, c, stage)
            assert plan.splitk > 1 and plan.tail_split == 1 and plan.f16 == 1, (stage, plan)
    if cid in TWINS:        # the LDS-DMA kernel: twins, gathered channels % 64 == 0, a forced (or large enough) 256 x 256 tile
        for stage in (0, 1):
            plan = plan16(ops, c, stage, twins=True, ALI_BM=256, ALI_BN=256)
            if gemm_cin(c)[stage] % 64 == 0:
                assert (plan.f16, plan.threads, plan.bm, plan.bn, plan.splitk, plan.tail_split) == (3, 512, 256, 256, 1, 1), (stage, plan)
            else:               # (t-s2's data gradient gathers 160 channels: converted in flight, pick_tile's tile)
                assert plan.f16 == 1 and plan.threads == 256 and plan.bm <= 128, (stage, plan)
            assert plan16(ops, c, stage, twins=True, ALI_NO_DMA16=1, ALI_SPLITK=1).f16 == (2 if gemm_cin(c)[stage] % 64 == 0 else 1)
            assert plan16(ops, c, stage, twins=False, ALI_BM=256, ALI_BN=256).f16 == 1      # no twins: the forced tile is dropped
    if cid == "tail16":
        for stage in (0, 1):
            for twins in (False, True):
                plan = plan16(ops, c, stage, twins=twins)
                assert (plan.bm, plan.bn, plan.splitk, plan.tail_split, plan.tail_u0) == (64, 64, 1, 2, 512), (stage, twins, plan)
                assert plan.f16 == (2 if twins else 1)     # 64 x 64 tiles, one N-tile each way; k-tiles of 32 over all R * S taps of the interior tiles
        assert ROUTE[cid]["fwd"][1] == ROUTE[cid]["bwd"][1] == 64 and c.C == c.K == 64
        assert ROUTE[cid]["fwd"][0] == (c.B * c.P * c.Q + 63) // 64 == 570 and ROUTE[cid]["bwd"][0] == (c.B * c.H * c.W + 63) // 64 == 540
        assert tail_split_ways(570, T * c.C // 32) == 2 and tail_split_ways(540, T * c.K // 32) == 2
    if cid in S2FIRST:      # predicate of conv_s2_first_kernel
        assert c.cpad in (4, 8) and c.K == 64 and c.R == c.S == 5 and c.stride == 2 and c.pad <= 2 and c.Q >= 32
        assert c.P % 4 != 0
        plan = plan16(ops, c, 0)
        assert (plan.route, plan.f16, plan.grid_x, plan.grid_y) == (2, 1, (c.P + 3) // 4, c.B), plan


# ----------------------------------------------------------------------------------------------------------------------
# CPU: properties of the cases themselves

@pytest.mark.parametrize("cid", list(BY_ID))
def test_f16_cases_are_rectangular(cid):
    c = BY_ID[cid]
    assert not (c.H == c.W and c.R == c.S) or cid in SQUARE_OK
    assert c.R != c.S or cid in SQUARE_OK
    assert c.H != c.W and c.P != c.Q


@pytest.mark.parametrize("cid", list(BY_ID))
def test_exact_leg_sums_fit_fp32(cid):
    """Every operand of the exact leg is a multiple of its unit, so every partial sum of an output -- in ANY order -- is a
    multiple of the output's grid unit and no larger than the same sum over the operands' moduli: below 2^24 units it is
    exactly representable in fp32 (and in the fp16 MFMA's fp32 accumulator), and so is the reference."""
    c = BY_ID[cid]
    r = reference(c, "exact")
    t = r["in"]
    for k, unit in (("x", 1.0), ("w", 1 / 8), ("b", 1 / 8), ("gpre", 1 / 4)):
        q = t[k].double() / unit
        assert torch.equal(q, q.round()) and torch.equal(t[k].half().float(), t[k]), (cid, k)
    assert t["x"].abs().max() <= 4 and t["w"].abs().max() <= 0.25 and t["gpre"].abs().max() <= 0.5
    bound, _ = _stages(c, t, torch.float64, "exact", r["gpre_in"], absolute=True)
    for name, unit in GRID.items():
        worst = bound[name].abs().max().item() / unit
        assert worst < 2 ** 24, (cid, name, worst)
        q = r["ref"][name] / unit
        assert torch.equal(q, q.round()), (cid, name)
        assert torch.equal(r["ref"][name].float().double(), r["ref"][name]), (cid, name)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", list(BY_ID))
def test_yprev_keeps_its_sign_class(cid, leg):
    """act' of the layer in front is taken from the fp16 twin of its output: rounding to fp16 may flush an element to
    exactly 0 (then "not > 0" for the device and the reference alike) but never moves one across zero"""
    t = reference(BY_ID[cid], leg)["in"]
    raw, h = t["yprev_raw"], t["yprev_raw"].half().float()
    assert torch.equal(h, t["yprev"])
    moved = (raw > 0) != (h > 0)
    assert bool((h[moved] == 0).all())
    assert bool(((raw < 0) == (h < 0))[h != 0].all())


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", list(BY_ID))
def test_f16_cases_tell_swapped_axes_apart(cid, leg):
    """test_cases_tell_swapped_axes_apart of test_gpu_conv_geometry.py on the ROUNDED operands of both legs: the fp64
    reference of the transposed problem, transposed back, agrees to 1e-12; with the two spatial strides of ONE operand
    exchanged the outputs that depend on it move by more than 100 x 2e-4 x max|ref| (random leg) and by at least one grid
    unit (exact leg, where any difference fails the test)."""
    c = BY_ID[cid]
    r = reference(c, leg)
    t, gy = r["in"], r["gpre_in"]

    def run(x, w, gy, cc):
        x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
        pre = geo._pre(cc, x, w, t["b"].double())
        dx, dw = torch.autograd.grad(pre, (x, w), gy.double())
        return {"pre": pre.detach(), "dx": dx, "dw": dw}

    true = run(t["x"], t["w"], gy, c)
    for k in ("dx", "dw"):
        assert (true[k] - r["ref"][k]).abs().max().item() <= 1e-12 * r["ref"][k].abs().max().item()
    ct = Case(c.id, (c.B, c.C, c.W, c.H, c.K, c.S, c.R, c.stride, c.pad), kind=c.kind, opad=c.opad[::-1])
    tr = run(geo._swap(t["x"]), geo._swap(t["w"]), geo._swap(gy), ct)
    for k in true:
        assert (geo._swap(tr[k]) - true[k]).abs().max().item() <= 1e-12 * true[k].abs().max().item(), (cid, k)
    if leg == "random":
        need = {k: 100 * RTOL * true[k].abs().max().item() for k in true}
    else:
        need = {"pre": 0.99 / 8, "dx": 0.99 / 32, "dw": 0.99 / 4}
    seen = 0
    for name, depends in (("x", ("pre", "dw")), ("w", ("pre", "dx")), ("gy", ("dx", "dw"))):
        ops_ = {"x": t["x"], "w": t["w"], "gy": gy}
        bad = geo._misread(ops_[name])
        if bad is None:
            continue
        ops_[name] = bad
        got = run(ops_["x"], ops_["w"], ops_["gy"], c)
        for k in depends:
            d = (got[k] - true[k]).abs().max().item()
            assert d > need[k], (cid, leg, name, k, d, need[k])
        seen += 1
    assert seen >= 2, cid


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the layers

class Layer:
    """device operands of one case and leg; ``twins``: every operand carries its fp16 twin (what a stepper iteration
    leaves: AliEpilogue.in16 / w16 / dact_y16, x16 / dy16 of ali_conv_bwd_weight)"""

    def __init__(self, ops, c, r, twins):
        t, T = r["in"], c.R * c.S
        self.ops, self.c, self.r, self.twins, self.geom = ops, c, r, twins, c.geom(ops)
        self.slope, self.dslope = SLOPE[r["leg"]]
        self.x = padded_nhwc(t["x"], c.cpad)
        self.gpre = nhwc(r["gpre_in"]).cuda()
        self.yprev = nhwc(t["yprev"]).cuda()
        self.mask, self.bias = t["mask"].cuda(), t["b"].cuda()
        if is_conv(c):
            self.wf = pack(ops, t["w"], c.K, T, c.C, c.cpad, c.C * T, 1, T)             # [K][T][cpad]
            self.wd = pack(ops, t["w"], c.C, T, c.K, c.K, T, 1, c.C * T)                # [C][T][K]
            if c.cpad != c.C:
                wd = torch.zeros(c.cpad, T, c.K, device="cuda")
                wd[:c.C] = self.wd
                self.wd = wd
        else:
            self.wf = pack(ops, t["w"], c.K, T, c.C, c.cpad, T, 1, c.K * T)
            self.wd = pack(ops, t["w"], c.C, T, c.K, c.K, c.K * T, 1, T)
        self.operands = (self.x, self.gpre, self.yprev, self.wf, self.wd)
        if twins:
            for a in self.operands:
                a._ali16 = a.half()
                assert torch.equal(a._ali16.float(), a)          # the operands ARE fp16 values

    def poison(self, *which):
        for a in which:
            a._ali16.zero_()

    def restore(self, *which):
        for a in which:
            a._ali16.copy_(a)

    def fwd(self, plain=False):
        ops, c = self.ops, self.c
        if plain:
            ep = ops.epilogue()
        elif is_conv(c):
            ep = ops.epilogue(bias=self.bias, act=ops.ACT_LEAKY, slope=self.slope)
        else:
            ep = ops.epilogue(bias=self.bias) if self.r["leg"] == "exact" else ops.epilogue(bias=self.bias, act=ops.ACT_TANH)
        y = nan(c.B, c.P, c.Q, c.K)
        dirty_workspace(ops)
        (ops.conv_fwd if is_conv(c) else ops.conv_bwd_data)(self.geom, self.x, self.wf, y, ep)
        return y

    def dgrad(self, epi):
        ops, c = self.ops, self.c
        ep = ops.epilogue()
        if epi:
            ep = ops.epilogue(mask=self.mask, dact_y=self.yprev, dact=ops.ACT_LEAKY, dslope=self.dslope)
            assert bool(ep.dact_y16) == (self.twins and ops._PRECISION["f16"])
        dx = nan(c.B, c.H, c.W, c.cpad)
        dirty_workspace(ops)
        (ops.conv_bwd_data if is_conv(c) else ops.conv_fwd)(self.geom, self.gpre, self.wd, dx, ep)
        return dx

    def wgrad(self):
        """(dw, db); a transposed convolution's weight gradient swaps the operands and has no fused bias gradient"""
        ops, c, T = self.ops, self.c, self.c.R * self.c.S
        dirty_workspace(ops)
        if is_conv(c):
            dw, db = nan(c.K, c.C, c.R, c.S), nan(c.K)
            ops.conv_bwd_weight(self.geom, self.x, self.gpre, dw, c.C, c.K, c.C * T, T, 1, db=db)
            return dw, db
        dw = nan(c.C, c.K, c.R, c.S)
        ops.conv_bwd_weight(self.geom, self.gpre, self.x, dw, c.K, c.C, c.K * T, T, 1)
        return dw, None

    def reads_twins(self, stage):
        """does the GEMM of the forward (0) / data gradient (1) read in16 / w16: only the 64-deep twin loop does"""
        return self.twins and gemm_cin(self.c)[stage] % 64 == 0


def dirty_workspace(ops):
    """NaN bit patterns all over the shared workspace behind its reserved head of arrival counters (include/ali_hip.h:
    ALI_WS_RESERVED): a split-K or pixel-split slab that a fold reads without the launch having written it shows in
    the output instead of depending on what ran before"""
    ops.workspace(torch.device("cuda", torch.cuda.current_device()))[4096:].fill_(0xFF)


def twin_is_rounded_output(ops, out):
    h = ops.shadow16(out)
    assert h is not None and h.dtype == torch.float16 and torch.equal(h, out.half()), "out16 is not the rounded output"


def run_gemms(ops, L, tag=""):
    """forward, data gradient plain and with mask + act' under precision("f16"), each against the reference, each leaving
    the fp16 twin of its output; a launch that ali_conv_uses_f16 reports as fp32 arithmetic equals the precision("f32")
    launch bit for bit"""
    c, r = L.c, L.r
    outs = {}
    with ops.precision("f16"):
        uses = [uses_f16(ops, c, s) for s in (0, 1)]
        for name, stage, go in (("y", 0, L.fwd), ("dx", 1, lambda: L.dgrad(False)), ("dx_epi", 1, lambda: L.dgrad(True))):
            out = outs[name] = go()
            verify(c, r, name, nchw(out[..., :c.C] if stage else out), name + tag)
            twin_is_rounded_output(ops, out)
            if stage and c.cpad != c.C:
                assert out[..., c.C:].abs().max().item() == 0.0
    for name, stage, go in (("y", 0, L.fwd), ("dx", 1, lambda: L.dgrad(False)), ("dx_epi", 1, lambda: L.dgrad(True))):
        if not uses[stage]:
            with ops.precision("f32"):
                o32 = go()
            assert ops.shadow16(o32) is None
            assert torch.equal(outs[name], o32), f"{c.id} {name}: the fp32 fall-back under f16 differs from the f32 launch"
    return outs, uses


def run_wgrad(ops, L, tag=""):
    c, r = L.c, L.r
    with ops.precision("f16"):
        dw, db = L.wgrad()
    verify(c, r, "dw", dw, "dw" + tag)
    if db is not None:
        verify(c, r, "db", db, "db (fused into wgrad)" + tag)
    return dw, db


@gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", CONVERTING)
def test_f16_gemm_converting_in_flight(cid, leg, forced_tile):
    """gconv_kernel<.., 2, 1> and wgrad_fast_kernel<.., F16 = 1>: fp32 operands in memory, no twins"""
    ops = _ops()
    c = BY_ID[cid]
    if forced_tile is None:
        assert_route(ops, c)
    L = Layer(ops, c, reference(c, leg), twins=False)
    _, uses = run_gemms(ops, L)
    assert tuple(uses) == ROUTE[cid]["uses"]
    run_wgrad(ops, L)
    if cid == "uni-pix":
        # whole k-loops: the launch follows the cost-ordered dispatch table ops uploads; ALI_NO_ORDER=1: natural order
        for env, tag in (({"ALI_SPLITK": 1}, " (cost-ordered)"), ({"ALI_SPLITK": 1, "ALI_NO_ORDER": 1}, " (natural order)")):
            with ops.tuning(**env):
                with ops.precision("f16"):
                    dev = torch.device("cuda", torch.cuda.current_device())
                    for which in (0, 1):
                        assert ops.conv_tile_order(L.geom, which, dev) is not None
                run_gemms(ops, L, tag)


@gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", FALLBACK)
def test_f16_fallback_is_the_f32_launch(cid, leg, forced_tile):
    """gathers of 6 / 20 / 8 channels: ali_conv_uses_f16 = 0, the launch under f16 is bit-identical to the f32 one and
    still leaves the fp16 twin of its output.  Weight gradient: `scalar` takes the generic wgrad_kernel (fp32 whatever
    the precision: bit-identical); `vec` / `pow2` take wgrad_fast_kernel<.., F16 = 1> with a pixel split."""
    ops = _ops()
    c = BY_ID[cid]
    if forced_tile is None:
        assert_route(ops, c)
    L = Layer(ops, c, reference(c, leg), twins=False)
    _, uses = run_gemms(ops, L)
    assert uses == [0, 0]
    dw, db = run_wgrad(ops, L)
    if cid == "scalar":
        with ops.precision("f32"):
            dw32, db32 = L.wgrad()
        assert torch.equal(dw, dw32) and torch.equal(db, db32)


@gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", TWINS)
def test_f16_gemm_from_twins(cid, leg, forced_tile):
    """gconv_kernel<.., 2, 2>: in16 / w16 read with 16-byte gathers of 8 halves, act' from dact_y16.  Poisoned twins
    prove what is read: zeroed in16 gives an all-zero output, zeroed dact_y16 gives act' = dslope everywhere."""
    ops = _ops()
    c = BY_ID[cid]
    if forced_tile is None:
        assert_route(ops, c)
    L = Layer(ops, c, reference(c, leg), twins=True)
    outs, uses = run_gemms(ops, L)
    assert uses == [1, 1]
    L.poison(L.yprev)
    with ops.precision("f16"):
        z = L.dgrad(True)
    want = outs["dx"] * L.mask.reshape(c.B, 1, 1, c.cpad) * L.dslope
    assert (z - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    assert not torch.equal(z, outs["dx_epi"])
    for what, twins in (("w16", (L.wf, L.wd)), ("in16", (L.x, L.gpre))):       # one operand's twin at a time
        L.poison(*twins)
        with ops.precision("f16"):
            for stage, go in ((0, lambda: L.fwd(plain=True)), (1, lambda: L.dgrad(False))):
                z = go()
                if L.reads_twins(stage):
                    assert z.abs().max().item() == 0.0, (cid, stage, "the launch did not read " + what)
                else:       # (t-s2's data gradient: 160 gathered channels, converted in flight from the fp32 operands)
                    assert torch.equal(z, outs["dx"])
        L.restore(*twins)


@gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", TWINS + ["uni-pix", "ct-pix"])
def test_f16_weight_gradient_from_twins(cid, leg, forced_tile):
    """wgrad_fast_kernel<.., true, 2> (mem16: x16 / dy16 read from memory; C % 8 == 0, K % 8 == 0, >= 64 dense channels per
    tile), every launch split over pixels: dw and the fused db (column sum of the rounded gpre) against the reference;
    a zeroed x16 gives an all-zero dw and leaves db alone, a zeroed dy16 zeroes both."""
    if forced_tile and forced_tile[3] < 64:
        pytest.skip("the twin-reading weight-gradient loop is instantiated for >= 64 dense channels per tile (wgrad.hip: mem16)")
    ops = _ops()
    c = BY_ID[cid]
    geom = c.geom(ops)
    assert geom.C % 8 == 0 and geom.K % 8 == 0 and geom.K > 32        # (K > 32: wgrad_tile's own tile is >= 64 wide)
    L = Layer(ops, c, reference(c, leg), twins=True)
    run_wgrad(ops, L, " (twins)")
    gathered, dense = (L.x, L.gpre) if is_conv(c) else (L.gpre, L.x)
    L.poison(gathered)
    with ops.precision("f16"):
        dw, db = L.wgrad()
    assert dw.abs().max().item() == 0.0, "the launch did not read x16"
    if db is not None:
        verify(c, L.r, "db", db, "db (x16 zeroed)")
    L.restore(gathered)
    L.poison(dense)
    with ops.precision("f16"):
        dw, db = L.wgrad()
    assert dw.abs().max().item() == 0.0, "the launch did not read dy16"
    if db is not None:
        assert db.abs().max().item() == 0.0, "the bias gradient did not come from dy16"


@gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", TWINS)
def test_f16_lds_dma_kernel(cid, leg):
    """gconv_kernel512<256, 256, .., 3> forced onto the rectangular twin cases (ragged M: t-img, t-ct; ragged N: all, K <
    256 or 160; pixel-major with tile-wide tap skipping: t-pix; sub-pixel phases with nr != ns: t-ct): against the
    reference, and EQUAL to the register-staged twin loop run with whole k-loops (ALI_NO_DMA16=1, ALI_SPLITK=1).
    ali_conv_mtiles plans without the twins and never reports this kernel, and a forced 256 x 256 tile quietly falls back
    to pick_tile's when the launch may not use it: the test asserts plan_conv's preconditions (both twins, gathered
    channels % 64 == 0, no fused BatchNorm or in_ld, ALI_SPLITK / ALI_NO_DMA16 unset) and that ali_conv_plan, asked
    with the epilogue of the launch itself, names the kernel (F16 = 3, 512 threads)."""
    import os
    ops = _ops()
    c = BY_ID[cid]
    L = Layer(ops, c, reference(c, leg), twins=True)
    assert all(ops.shadow16(a) is not None for a in (L.x, L.gpre, L.wf, L.wd))
    assert os.environ.get("ALI_SPLITK", "0") in ("", "0") and os.environ.get("ALI_NO_DMA16", "0") in ("", "0")
    stages = [("y", 0, L.fwd), ("dx", 1, lambda: L.dgrad(False)), ("dx_epi", 1, lambda: L.dgrad(True))]
    stages = [s for s in stages if L.reads_twins(s[1])]       # (the LDS-DMA kernel wants Cin % 64 == 0: not t-s2's dgrad)
    assert len(stages) == (1 if cid == "t-s2" else 3)
    outs = []
    for env, tag in (({"ALI_BM": 256, "ALI_BN": 256}, " (LDS-DMA)"), ({"ALI_NO_DMA16": 1, "ALI_SPLITK": 1}, " (register-staged)")):
        with ops.tuning(**env), ops.precision("f16"):
            outs.append({})
            for name, stage, go in stages:
                out = outs[-1][name] = go()
                ep = ops.epilogue()
                ops._f16_operands(L.geom, _which(c)[stage], *((L.x, L.wf) if stage == 0 else (L.gpre, L.wd)), out, ep)
                assert ops.conv_plan(L.geom, _which(c)[stage], ep).f16 == (3 if "ALI_BM" in env else 2), (cid, name, tag)
                verify(c, L.r, name, nchw(out), name + tag)
                twin_is_rounded_output(ops, out)
    for name, _, _ in stages:
        assert torch.equal(outs[0][name], outs[1][name]), f"{cid} {name}: LDS-DMA loop differs from the register-staged twin loop"
    for what, twins in (("w16", (L.wf, L.wd)), ("in16", (L.x, L.gpre))):
        L.poison(*twins)
        with ops.tuning(ALI_BM=256, ALI_BN=256), ops.precision("f16"):
            for stage, go in ((0, lambda: L.fwd(plain=True)), (1, lambda: L.dgrad(False))):
                if L.reads_twins(stage):
                    assert go().abs().max().item() == 0.0, (cid, stage, "the forced 256 x 256 launch did not read " + what)
        L.restore(*twins)


@gpu
@pytest.mark.parametrize("twins", [False, True], ids=["converting", "twins"])
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", ["tail16", "tail"])
def test_f16_tail_split(cid, leg, twins):
    """`tail16` at the library's own tile (the block count is the route): forward 570 and data gradient 540 blocks of
    64 x 64, of which 512 run whole and the 58 / 28 left over are cut two ways along K and folded in the kernel
    (plan_conv: uniform-tap loops, fp32 and fp16 alike; test_f16_case_takes_its_route asserts the
    preconditions).  `tail`, the fp32 module's geometry, has too few blocks under the fp16 tile rule: plain split-K."""
    ops = _ops()
    c = BY_ID[cid]
    assert_route(ops, c)
    L = Layer(ops, c, reference(c, leg), twins=twins)
    run_gemms(ops, L)
    run_wgrad(ops, L)


@gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("cid", S2FIRST)
def test_f16_s2_first_kernel(cid, leg):
    """conv_s2_first_kernel<4 | 8, true>: y and the out16 twin its row-walking stores leave, NaN-filled beforehand"""
    ops = _ops()
    c = BY_ID[cid]
    assert_route(ops, c)
    L = Layer(ops, c, reference(c, leg), twins=False)
    with ops.precision("f16"):
        assert uses_f16(ops, c, 0) == 1
        y = L.fwd()
    verify(c, L.r, "y", nchw(y))
    twin_is_rounded_output(ops, y)
