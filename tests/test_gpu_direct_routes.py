"""Every route of the direct one-channel kernels (csrc/direct.hip: ali_tconv1_fwd / ali_tconv1_dgrad / ali_tconv1_wgrad).

The three entry points choose among eleven kernels and 38 instantiations (37 of which a shape can reach) by shape,
LDS budget, batch and ALI_NO_T1_MFMA.  Every case below is the smallest shape that takes the instantiation named in its table entry, has a
rectangular map (P != Q) and, where the op accepts one, a rectangular kernel (R != S); ``ops.tconv1_route`` -- the
launches' own plan -- is asserted first, so a later change of the dispatch cannot move a case silently.

Convention of test_gpu_conv_geometry.py (its RTOL, YARD and ``check``).  Reference: F.conv_transpose2d with autograd on
the CPU in fp64, bias, activation, act' and rowscale applied in fp64.  Yardstick: the same computation in CPU fp32.
With e(t) = max|t - ref64| every device output is held to e <= 4 * e(cpu fp32) and e <= 2e-4 * max|ref64|.  Each op
is fed its own fp32 inputs (the activated map for act', the pre-activation gradient as the 1-channel map), so each
kernel is judged alone.  Outputs are prefilled with NaN; a strided plane's neighbours must keep it; operand planes the
op must not read are NaN too.  Weight gradients run twice and must be bit-identical (fixed-order reductions), and leave
the workspace's reserved head at zero.  DESIGN.md 4 has the measured ratios per route.

instantiation                    case ids
  tconv1_fwd_mfma_kernel<1,4,8>  f-m14, f-m14-full, f-m14-edge
  tconv1_fwd_mfma_kernel<1,2,8>  f-m12
  tconv1_fwd_mfma_kernel<2,4,8>  f-m24
  tconv1_fwd_mfma_kernel<2,2,8>  f-m22, f-m22-edge
  tconv1_fwd_kernel<25,5>        f-v25, f-v25-nomfma
  tconv1_fwd_kernel<16,4>        f-v16, f-v16-lds, f-v16-nomfma
  tconv1_fwd_kernel<9,3>         f-v9, f-xcd8, f-xcd16, f-xcd9
  tconv1_fwd_kernel<4,2>         f-v4
  tconv1_fwd_kernel<1,1>         f-v1
  tconv1_dgrad_band_kernel<1>    d-b-1x1
  tconv1_dgrad_band_kernel<4>    d-b-1x4, d-b-4x1, d-b-2x2, d-b-whole
  tconv1_dgrad_band_kernel<9>    d-b-3x3, d-b-ragged
  tconv1_dgrad_band_kernel<16>   d-b-4x4
  tconv1_dgrad_band_kernel<25>   d-b-5x5
  tconv1_dgrad_kernel<1>         d-n-1x1
  tconv1_dgrad_kernel<4>         d-n-1x4, d-n-4x1, d-n-2x2
  tconv1_dgrad_kernel<9>         d-n-3x3
  tconv1_dgrad_kernel<16>        d-n-4x4, d-n-stride, d-n-wide
  tconv1_dgrad_kernel<25>        d-n-5x5
  tconv1_wgrad_mfma_kernel<1,8>  w-m1, w-m1-pack, w-m1-many, w-m1-edge
  tconv1_wgrad_mfma_kernel<2,8>  none: no shape reaches it (see WGRAD); its shapes are w-t25, w-t20-4x5, w-t20-5x4
  tconv1_wgrad_rb_kernel<1,3>    w-rb13, w-m1-past, w-rb13-many
  tconv1_wgrad_rb_kernel<1,4>    w-rb14, w-rb14-nomfma
  tconv1_wgrad_rb_kernel<1,5>    w-rb15, w-t20-4x5
  tconv1_wgrad_rb_kernel<5,3>    w-rb53
  tconv1_wgrad_rb_kernel<5,4>    w-rb54
  tconv1_wgrad_rb_kernel<5,5>    w-rb55
  tconv1_wgrad_rb_kernel<7,3>    w-rb73
  tconv1_wgrad_rb_kernel<7,4>    w-rb74
  tconv1_wgrad_rb_kernel<7,5>    w-rb75
  tconv1_wgrad_kernel<1>         w-g1, w-t25, w-t20-5x4
  tconv1_wgrad_kernel<2>         w-g2, w-g2-many
  tconv1_wgrad_kernel<3..8>      w-g3, w-g4, w-g5, w-g6, w-g7, w-g8
(test_cases_name_every_instantiation holds the table's left column against the cases.)
"""
import contextlib
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_geometry import RTOL, YARD, check, nan   # noqa: F401  (RTOL, YARD: the bounds ``check`` applies)

gpu = pytest.mark.gpu

NO_MFMA = {"ALI_NO_T1_MFMA": 1}
NUM_CU = 256                 # kNumCU of csrc/ali_common.h: the batch thresholds below are multiples of it

# (case id, output) -> why the 4x yardstick does not apply (the 2e-4 cap still does).  At most 3; see DESIGN.md 4.
CAP_ONLY = {}


def _ops():
    from ali_hip import ops
    return ops


class Case:
    """One launch: ``op`` in fwd / dgrad / wgrad on a [B,P,Q,K] many-channel map and an R x S kernel; the 1-channel map
    is H x W = (P + R - 1 - 2 pad) x (Q + S - 1 - 2 pad).  ``route``: what ops.tconv1_route must say under ``env``."""

    def __init__(self, cid, op, route, B, P, Q, K, R, S, pad, env=None, **opt):
        self.id, self.op, self.route, self.env, self.opt = cid, op, route, env or {}, opt
        self.B, self.P, self.Q, self.K, self.R, self.S, self.pad = B, P, Q, K, R, S, pad
        self.H, self.W, self.T = P + R - 1 - 2 * pad, Q + S - 1 - 2 * pad, R * S
        self.nc = opt.get("nc", 1)

    def dims(self):
        return (self.B, self.P, self.Q, self.K, self.R, self.S, self.pad)


def Fw(cid, route, B, P, Q, K, R, pad, act="none", bias=True, ostride=1, rowscale=False, env=None):
    return Case("f-" + cid, "fwd", route, B, P, Q, K, R, R, pad, env, act=act, bias=bias, ostride=ostride, rowscale=rowscale)


def Dg(cid, route, B, P, Q, K, R, S, pad, sstride=1, dact=None, env=None):
    return Case("d-" + cid, "dgrad", route, B, P, Q, K, R, S, pad, env, sstride=sstride, dact=dact)


def Wg(cid, route, B, P, Q, K, R, S, pad, nc=1, sstride=None, layout="own", env=None):
    return Case("w-" + cid, "wgrad", route, B, P, Q, K, R, S, pad, env, nc=nc, sstride=sstride or nc, layout=layout)


FWD = [
    # matrix-core scatter form (K in {32, 64}, <= 32 taps, P * Q * LDC * 4 <= 64 KB); pad in {0, 1, R - 1}
    Fw("m14", "fwd_mfma<1,4>", 3, 7, 9, 64, 4, 0, act="tanh"),
    Fw("m14-full", "fwd_mfma<1,4>", 2, 8, 9, 64, 4, 3, act="leaky", ostride=4),
    Fw("m12", "fwd_mfma<1,2>", 3, 8, 13, 32, 3, 1, act="leaky", rowscale=True),
    Fw("m24", "fwd_mfma<2,4>", 3, 7, 10, 64, 5, 4, bias=False),
    Fw("m22", "fwd_mfma<2,2>", 3, 8, 11, 32, 5, 0, act="tanh", bias=False, rowscale=True),
    # the LDS boundary from both sides: 26 * 37 * 17 * 4 = 65416 and 21 * 31 * 25 * 4 = 65100 bytes fit ...
    Fw("m14-edge", "fwd_mfma<1,4>", 2, 26, 37, 64, 4, 1, act="tanh"),
    Fw("m22-edge", "fwd_mfma<2,2>", 2, 21, 31, 32, 5, 2),
    # ... 31 * 32 * 17 * 4 = 67456 do not: the gather form, 9 row bands x 2 column blocks
    Fw("v16-lds", "fwd<16,4>", 2, 31, 32, 64, 4, 0, act="tanh"),
    # gather form on the VALU: K outside {32, 64} (96 is legal for the forward only) ...
    Fw("v25", "fwd<25,5>", 3, 7, 9, 96, 5, 0, act="leaky"),
    Fw("v16", "fwd<16,4>", 3, 7, 9, 128, 4, 1, ostride=4),
    Fw("v9", "fwd<9,3>", 3, 5, 9, 256, 3, 2, act="tanh", rowscale=True),
    Fw("v4", "fwd<4,2>", 3, 7, 9, 96, 2, 0, bias=False),
    Fw("v1", "fwd<1,1>", 3, 7, 9, 128, 1, 0, act="leaky"),
    # ... or ALI_NO_T1_MFMA=1
    Fw("v16-nomfma", "fwd<16,4>", 3, 7, 9, 64, 4, 0, act="tanh", env=NO_MFMA),
    Fw("v25-nomfma", "fwd<25,5>", 3, 8, 11, 32, 5, 4, env=NO_MFMA),
    # the XCD block remap (gridDim.z % 8 == 0) with 2 row bands x 2 column blocks (H = 8 > 4, W = 35 > 32), one and two
    # images per XCD; the same map at B = 9 keeps the natural order.  Every image has its own values and its own factor
    Fw("xcd8", "fwd<9,3>", 8, 6, 33, 128, 3, 0, act="tanh", rowscale=True),
    Fw("xcd16", "fwd<9,3>", 16, 6, 33, 128, 3, 0, act="tanh", rowscale=True),
    Fw("xcd9", "fwd<9,3>", 9, 6, 33, 128, 3, 0, act="tanh", rowscale=True),
]

# (taps id, B, P, Q, K, R, S, pad, sstride, dact): once on the band kernel, once under ALI_NO_T1_MFMA=1 on the other
DGRAD_TABLE = [
    ("1x1", 3, 5, 7, 32, 1, 1, 0, 1, None),
    ("1x4", 3, 5, 7, 64, 1, 4, 0, 4, "leaky"),
    ("4x1", 3, 5, 7, 128, 4, 1, 0, 1, "tanh"),
    ("2x2", 3, 5, 7, 256, 2, 2, 1, 1, None),
    ("3x3", 3, 5, 7, 32, 3, 3, 1, 4, "tanh"),
    ("4x4", 3, 5, 7, 64, 4, 4, 0, 1, "leaky"),
    ("5x5", 3, 5, 7, 256, 5, 5, 2, 1, "leaky"),
]
DGRAD = (
    [Dg("b-" + t[0], f"dgrad_band<{t[5] * t[6]}>", *t[1:]) for t in DGRAD_TABLE]
    + [Dg("n-" + t[0], f"dgrad<{t[5] * t[6]}>", *t[1:], env=NO_MFMA) for t in DGRAD_TABLE]
    + [
        # 64 images: bands of 2 rows give 64 * 8 = 512 = 2 * kNumCU blocks, the last band of the 15 rows is ragged
        Dg("b-ragged", "dgrad_band<9>", 64, 15, 5, 32, 3, 3, 1, dact="leaky"),
        # 520 >= 2 * kNumCU images: one band is the whole image
        Dg("b-whole", "dgrad_band<4>", 520, 5, 6, 32, 2, 2, 0),
        # 16 * 32 * 33 * 256 / 4 = 1081344 items > 4096 * 256 threads: the grid stride runs
        Dg("n-stride", "dgrad<16>", 16, 32, 33, 256, 4, 4, 0, dact="leaky", env=NO_MFMA),
        # a band of one output row needs 4 * 2103 * 4 = 33648 bytes > 32 KB: the non-band kernel by itself
        Dg("n-wide", "dgrad<16>", 1, 4, 2100, 32, 4, 4, 0),
    ])

WGRAD = [
    # matrix cores: one small channel, K = 64, <= 32 taps, the padded 1-channel image + the fold scratch in 64 KB
    Wg("m1", "wgrad_mfma<1,8>", 3, 6, 9, 64, 3, 3, 1, layout="tail"),
    Wg("m1-pack", "wgrad_mfma<1,8>", 3, 5, 7, 64, 3, 3, 0, layout="pack"),
    # 17 to 32 taps would take tconv1_wgrad_mfma_kernel<2,8> -- whose fold scratch alone is 8 * 4 * 2 * 64 * 4 floats =
    # 64 KB, so `lds_m <= 64 KB` never holds and the launch falls through (test_wgrad_mfma_two_tap_tiles_is_never_launched):
    # 5x5 and 5x4 land on the VALU kernel (R = 5 > 256 / 64), 4x5 on the register-blocked one
    Wg("t25", "wgrad<1>", 3, 6, 9, 64, 5, 5, 2, layout="tail"),
    Wg("t20-4x5", "wgrad_rb<1,5>", 3, 6, 7, 64, 4, 5, 0, sstride=4),
    Wg("t20-5x4", "wgrad<1>", 3, 7, 6, 64, 5, 4, 1),
    # 520 > 2 * kNumCU tiny images: 512 blocks, eight of them walk two images
    Wg("m1-many", "wgrad_mfma<1,8>", 520, 3, 5, 64, 2, 3, 0),
    # (1022 + 2) * (6 + 2) = 8192 floats of image + 8192 of scratch = 64 KB exactly; one row more falls back
    Wg("m1-edge", "wgrad_mfma<1,8>", 2, 1022, 6, 64, 3, 3, 0),
    Wg("m1-past", "wgrad_rb<1,3>", 2, 1023, 6, 64, 3, 3, 0),
    # register-blocked: nc in {1, 5, 7}, S in {3, 4, 5}, R <= 256 / K; Q a multiple of 4 and not; P in {5, 6, 7}
    Wg("rb13", "wgrad_rb<1,3>", 4, 5, 7, 128, 2, 3, 0),
    Wg("rb14", "wgrad_rb<1,4>", 4, 6, 9, 256, 1, 4, 0),
    Wg("rb15", "wgrad_rb<1,5>", 4, 7, 12, 32, 5, 5, 2),
    Wg("rb14-nomfma", "wgrad_rb<1,4>", 4, 6, 7, 64, 4, 4, 1, env=NO_MFMA),
    Wg("rb53", "wgrad_rb<5,3>", 4, 5, 8, 32, 2, 3, 0, nc=5, sstride=8),
    Wg("rb54", "wgrad_rb<5,4>", 4, 6, 7, 64, 4, 4, 1, nc=5),
    Wg("rb55", "wgrad_rb<5,5>", 4, 7, 9, 32, 5, 5, 0, nc=5, sstride=8, layout="pack"),
    Wg("rb73", "wgrad_rb<7,3>", 4, 5, 6, 128, 2, 3, 1, nc=7, layout="wide"),
    Wg("rb74", "wgrad_rb<7,4>", 4, 6, 8, 256, 1, 4, 0, nc=7, sstride=8),
    Wg("rb75", "wgrad_rb<7,5>", 4, 7, 5, 64, 3, 5, 1, nc=7),
    # 300 images x 7 bands = 2100 work items > 8 * kNumCU = 2048 blocks: some blocks walk two
    Wg("rb13-many", "wgrad_rb<1,3>", 300, 28, 4, 32, 3, 3, 1),
    # VALU: every nc; K = 64 with 25 taps owns 7 accumulators (28 slots), K = 128 with 10 / 12 taps 5 / 6, K = 256 with 6
    Wg("g1", "wgrad<1>", 4, 6, 7, 32, 2, 2, 0),
    Wg("g2", "wgrad<2>", 4, 6, 7, 32, 5, 5, 0, nc=2),
    Wg("g3", "wgrad<3>", 4, 5, 7, 128, 2, 5, 0, nc=3, sstride=4, layout="wide"),
    Wg("g4", "wgrad<4>", 4, 5, 7, 128, 3, 4, 1, nc=4),
    Wg("g5", "wgrad<5>", 4, 5, 7, 256, 2, 3, 0, nc=5, sstride=8),
    Wg("g6", "wgrad<6>", 4, 6, 7, 64, 3, 3, 1, nc=6, layout="pack"),
    Wg("g7", "wgrad<7>", 4, 6, 7, 64, 5, 5, 0, nc=7),
    Wg("g8", "wgrad<8>", 4, 6, 7, 32, 4, 4, 0, nc=8),
    Wg("g2-many", "wgrad<2>", 300, 28, 4, 32, 2, 2, 0, nc=2),
]

CASES = FWD + DGRAD + WGRAD
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

ALL_ROUTES = (
    {f"fwd_mfma<{nt},{kc}>" for nt in (1, 2) for kc in (2, 4)} | {f"fwd<{s * s},{s}>" for s in range(1, 6)}
    | {f"{k}<{t}>" for k in ("dgrad_band", "dgrad") for t in (1, 4, 9, 16, 25)}
    | {"wgrad_mfma<1,8>"} | {f"wgrad_rb<{nc},{s}>" for nc in (1, 5, 7) for s in (3, 4, 5)}
    | {f"wgrad<{nc}>" for nc in range(1, 9)})


# ----------------------------------------------------------------------------------------------------------------------
# host side (no GPU)

def route_of(ops, c):
    return ops.tconv1_route(c.op, *c.dims(), nc=c.nc)


def setting(ops, c):
    """the case's tuning variables for the block (nothing is re-read for a case without any)"""
    return ops.tuning(**c.env) if c.env else contextlib.nullcontext()


def test_cases_name_every_instantiation():
    assert len(ALL_ROUTES) == 37 and {c.route for c in CASES} == ALL_ROUTES
    assert len(CAP_ONLY) <= 3
    assert all(c.P != c.Q for c in CASES)
    assert any(c.R != c.S for c in DGRAD) and any(c.R != c.S for c in WGRAD)


def test_wgrad_mfma_two_tap_tiles_is_never_launched():
    """tconv1_wgrad_mfma_kernel<2,8> is instantiated and dispatched to, but its LDS need starts at 64 KB + one image: the
    predicate of its branch is false for every shape, so no parity case can name it.  Should this ever fail, the
    dispatch has changed and the 17..32-tap shapes need cases of their own on the new route."""
    ops = _ops()
    ops.reload_tuning()
    for R in range(1, 6):
        for S in range(1, 6):
            for B, P, Q in ((1, 1, 2), (3, 6, 9), (600, 2, 3)):
                got = ops.tconv1_route("wgrad", B, P, Q, 64, R, S, 0, nc=1)
                assert got is not None and got != "wgrad_mfma<2,8>", (R, S, B, P, Q, got)
                assert (got == "wgrad_mfma<1,8>") == (R * S <= 16), (R, S, B, P, Q, got)


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_case_takes_its_route(cid):
    """the launches' own plan names the case's instantiation -- and the arithmetic of the launch parameters the plan does
    not report (band heights, work items, remap) puts the case where its comment says"""
    ops, c = _ops(), BY_ID[cid]
    ops.reload_tuning()
    with setting(ops, c):
        assert route_of(ops, c) == c.route, (cid, route_of(ops, c))
    if c.env:       # ... and the case needs its setting to get there
        assert route_of(ops, c) != c.route, cid
    if c.op == "dgrad" and c.route.startswith("dgrad_band"):
        rbv = c.P
        while rbv > 1 and c.B * -(-c.P // rbv) < 2 * NUM_CU:
            rbv = (rbv + 1) // 2
        want = {"d-b-ragged": 2, "d-b-whole": c.P}.get(cid, 1)
        assert rbv == want and (cid != "d-b-ragged" or c.P % rbv), (cid, rbv)
    if cid == "d-n-stride":
        assert c.B * c.P * c.Q * c.K // 4 > 4096 * 256
    if c.op == "wgrad":
        items = c.B * -(-c.P // 4)
        assert (items > 8 * NUM_CU) == cid.endswith("-many") or c.route.startswith("wgrad_mfma"), (cid, items)
        if cid == "w-m1-many":
            assert c.B > 2 * NUM_CU
    if c.op == "fwd" and c.route.startswith("fwd<"):
        grid = (-(-c.W // 32), -(-c.H // 4), c.B)
        if "xcd" in cid:
            assert grid[0] >= 2 and grid[1] >= 2 and (c.B % 8 == 0) == (cid != "f-xcd9")
        else:
            assert c.B % 8 != 0


# ----------------------------------------------------------------------------------------------------------------------
# references (computed once per case, never modified)

def _slope(dt):
    return torch.tensor(0.2).to(dt)      # (the device's slope is the fp32 0.2)


def _act(pre, act, dt):
    if act == "tanh":
        return torch.tanh(pre)
    if act == "leaky":
        return torch.where(pre > 0, pre, pre * _slope(dt))
    return pre


def _act_grad(y, act, dt):
    if act == "tanh":
        return 1 - y * y
    return torch.where(y > 0, torch.ones((), dtype=dt), _slope(dt))


def _inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    t = {}
    if c.op == "fwd":
        t["big"] = torch.randn(c.B, c.K, c.P, c.Q, generator=g)
        t["w"] = torch.randn(c.K, 1, c.R, c.S, generator=g) / (c.K * c.T) ** 0.5
        t["bias"] = torch.randn(1, generator=g)
        t["rs"] = (torch.rand(c.B, 5, generator=g) > 0.3).float() * 1.25 + torch.rand(c.B, 5, generator=g)
    elif c.op == "dgrad":
        t["small"] = torch.randn(c.B, 1, c.H, c.W, generator=g)
        t["w"] = torch.randn(c.K, 1, c.R, c.S, generator=g)
        y = torch.randn(c.B, c.K, c.P, c.Q, generator=g)       # the activated map in front: any sign / inside (-1, 1)
        t["y"] = torch.tanh(y) if c.opt["dact"] == "tanh" else y
    else:
        t["big"] = torch.randn(c.B, c.K, c.P, c.Q, generator=g)
        t["small"] = torch.randn(c.B, c.nc, c.H, c.W, generator=g)
    return t


def _host(c, t, dt):
    if c.op == "fwd":
        bias = t["bias"].to(dt) if c.opt["bias"] else None
        y = _act(F.conv_transpose2d(t["big"].to(dt), t["w"].to(dt), bias, padding=c.pad), c.opt["act"], dt)
        if c.opt["rowscale"]:
            y = y * t["rs"][:, 3].to(dt).reshape(c.B, 1, 1, 1)
        return {"y": y[:, 0]}
    if c.op == "dgrad":     # the input gradient of the transposed convolution, cotangent = the 1-channel map
        x = torch.zeros(c.B, c.K, c.P, c.Q, dtype=dt, requires_grad=True)
        (gx,) = torch.autograd.grad(F.conv_transpose2d(x, t["w"].to(dt), None, padding=c.pad), x, t["small"].to(dt))
        if c.opt["dact"]:
            gx = gx * _act_grad(t["y"].to(dt), c.opt["dact"], dt)
        return {"gx": gx}
    w = torch.zeros(c.K, c.nc, c.R, c.S, dtype=dt, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv_transpose2d(t["big"].to(dt), w, None, padding=c.pad), w, t["small"].to(dt))
    return {"dw": dw}


_REF = {}


def reference(c):
    hit = _REF.get(c.id)
    if hit is None:
        t = _inputs(c)
        hit = _REF[c.id] = {"in": t, "ref": _host(c, t, torch.float64), "f32": _host(c, t, torch.float32)}
    return hit


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def w_tk(w):
    """[K,1,R,S] -> the kernels' [R*S][K]"""
    K = w.shape[0]
    return w.reshape(K, -1).t().contiguous().cuda()


ACT = {"none": "ACT_NONE", "leaky": "ACT_LEAKY", "tanh": "ACT_TANH"}


# ----------------------------------------------------------------------------------------------------------------------
# device

@gpu
@pytest.mark.parametrize("cid", [c.id for c in FWD])
def test_forward(cid):
    ops, c = _ops(), BY_ID[cid]
    r = reference(c)
    t, o = r["in"], c.opt
    big, w = nhwc(t["big"]).cuda(), w_tk(t["w"])
    bias = t["bias"].cuda() if o["bias"] else None
    mask = t["rs"].cuda()                                   # [B, 5]: column 3 is a strided view
    full = nan(c.B, c.H, c.W, o["ostride"])
    out = full[..., 2 if o["ostride"] > 1 else 0]
    with setting(ops, c):
        assert route_of(ops, c) == c.route
        ops.tconv1_fwd(big, w, bias, out, c.B, c.P, c.Q, c.K, c.R, c.S, c.pad, o["ostride"], getattr(ops, ACT[o["act"]]),
                       0.2, rowscale=mask[:, 3] if o["rowscale"] else None)
        torch.cuda.synchronize()
    check(c, r, "y", out, prefix="DIRECT", cap_only=CAP_ONLY)
    if o["ostride"] > 1:
        others = full[..., [0, 1, 3]]
        assert torch.isnan(others).all().item(), f"{cid}: wrote outside its plane"


@gpu
@pytest.mark.parametrize("cid", [c.id for c in DGRAD])
def test_data_gradient(cid):
    ops, c = _ops(), BY_ID[cid]
    r = reference(c)
    t, o = r["in"], c.opt
    planes = nan(c.B, c.H, c.W, o["sstride"])               # the other planes of the NHWC tensor must not be read
    small = planes[..., o["sstride"] - 1]
    small.copy_(t["small"][:, 0].cuda())
    y = nhwc(t["y"]).cuda() if o["dact"] else None
    gx = nan(c.B, c.P, c.Q, c.K)
    with setting(ops, c):
        assert route_of(ops, c) == c.route
        ops.tconv1_dgrad(small, o["sstride"], w_tk(t["w"]), y, getattr(ops, ACT[o["dact"] or "none"]), 0.2, gx,
                         c.B, c.P, c.Q, c.K, c.R, c.S, c.pad)
        torch.cuda.synchronize()
    check(c, r, "gx", gx.permute(0, 3, 1, 2), prefix="DIRECT", cap_only=CAP_ONLY)


def _dw_buffer(c, layout):
    """(buffer, [K,nc,R,S] view of it, s_k, s_tap, s_c)"""
    K, nc, R, S, T = c.K, c.nc, c.R, c.S, c.T
    if layout == "pack":        # [nc][taps][K]: the forward pack's order
        buf = nan(nc, T, K)
        return buf, torch.as_strided(buf, (K, nc, R, S), (1, T * K, S * K, K)), 1, K, T * K
    if layout == "wide":        # one more channel than the launch writes: it keeps its NaN
        buf = nan(K, nc + 1, R, S)
        return buf, buf[:, :nc], (nc + 1) * T, 1, T
    buf = nan(K, nc, R, S)      # "own": first_direct's layout; "tail": the one-channel tail's (s_c unused)
    return buf, buf, nc * T, 1, 0 if layout == "tail" else T


@gpu
@pytest.mark.parametrize("cid", [c.id for c in WGRAD])
def test_weight_gradient(cid):
    ops, c = _ops(), BY_ID[cid]
    r = reference(c)
    t, o = r["in"], c.opt
    big = nhwc(t["big"]).cuda()
    small = nan(c.B, c.H, c.W, o["sstride"])                # channels >= nc must not be read
    small[..., :c.nc] = nhwc(t["small"]).cuda()
    runs = []
    with setting(ops, c):
        assert route_of(ops, c) == c.route
        for _ in range(2):
            buf, view, s_k, s_tap, s_c = _dw_buffer(c, o["layout"])
            ops.tconv1_wgrad(big, small, o["sstride"], c.nc, buf, s_k, s_tap, s_c, c.B, c.P, c.Q, c.K, c.R, c.S, c.pad)
            torch.cuda.synchronize()
            runs.append((buf, view))
    check(c, r, "dw", runs[0][1], prefix="DIRECT", cap_only=CAP_ONLY)
    assert torch.equal(runs[0][1], runs[1][1]), f"{cid}: two runs differ (the reductions are fixed-order)"
    if o["layout"] == "wide":
        assert torch.isnan(runs[0][0][:, c.nc]).all().item(), f"{cid}: wrote outside its channels"
    # the slabs live behind the workspace's reserved head (the GEMM kernels' arrival counters, left at zero)
    assert not ops.workspace(torch.device("cuda"))[:4096].any().item()


REFUSED = [
    ("fwd", (3, 7, 9, 64, 3, 4, 0), 1),          # R != S on the forward
    ("fwd", (3, 7, 9, 64, 6, 6, 0), 1),          # S = 6
    ("dgrad", (3, 7, 9, 64, 1, 6, 0), 1),
    ("wgrad", (3, 7, 9, 64, 6, 1, 0), 1),
    ("wgrad", (3, 7, 9, 128, 4, 4, 0), 1),       # 16 taps over 2 tap groups: 8 accumulators, the kernel has 7
    ("wgrad", (3, 7, 9, 256, 3, 3, 0), 1),       # 9 taps, one group
    ("dgrad", (3, 7, 9, 48, 3, 3, 0), 1),        # K / 4 = 12 does not divide the block
    ("dgrad", (3, 7, 9, 64, 3, 4, 0), 1),        # 12 taps: no instantiation
]


@gpu
@pytest.mark.parametrize("op,dims,nc", REFUSED, ids=[f"{op}-{'x'.join(map(str, d))}" for op, d, _ in REFUSED])
def test_refusals_launch_nothing(op, dims, nc):
    """RuntimeError from the C ABI and a None route; the outputs keep their NaN"""
    ops = _ops()
    ops.reload_tuning()
    B, P, Q, K, R, S, pad = dims
    H, W, T = P + R - 1 - 2 * pad, Q + S - 1 - 2 * pad, R * S
    assert ops.tconv1_route(op, *dims, nc=nc) is None
    big, small, w = torch.ones(B, P, Q, K, device="cuda"), torch.ones(B, H, W, 1, device="cuda"), torch.ones(T, K, device="cuda")
    out = nan(B, H, W, 1) if op == "fwd" else nan(B, P, Q, K) if op == "dgrad" else nan(K, 1, R, S)
    with pytest.raises(RuntimeError):
        if op == "fwd":
            ops.tconv1_fwd(big, w, None, out, B, P, Q, K, R, S, pad, 1, ops.ACT_NONE, 0.0)
        elif op == "dgrad":
            ops.tconv1_dgrad(small, 1, w, None, ops.ACT_NONE, 0.0, out, B, P, Q, K, R, S, pad)
        else:
            ops.tconv1_wgrad(big, small, 1, nc, out, T, 1, 0, B, P, Q, K, R, S, pad)
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item()
