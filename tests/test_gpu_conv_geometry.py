"""Rectangular maps and kernels on every route of the convolution kernels (csrc/gconv.hip, csrc/wgrad.hip).

The C ABI takes H, W / P, Q / R, S separately, yet every other conv test hands it squares: a swap of Hin / Win, P / Q,
dh / dw, nr / ns or of the two 16-bit halves of a pixel-table entry would pass them all.  Every case below has
H != W, P != Q and R != S wherever its route allows, and is the smallest shape that still takes the route named in its
comment; the host queries (ali_conv_mtiles, ali_conv_tile_order, ali_wgrad_deferrable) are asserted so that a later
change of pick_tile cannot move a case onto another route unnoticed.

Reference: F.conv2d / F.conv_transpose2d with autograd on the CPU in fp64, epilogue applied in fp64.  Yardstick: the same
computation in CPU fp32.  With e(t) = max|t - ref64| every device output is held to
    e(device) <= 4 * e(cpu fp32)            (the convention of test_gpu_ssim.py / test_gpu_griffinlim.py)
    e(device) <= 2e-4 * max|ref64|          (RTOL of test_gpu_kernels.py)
Every stage is fed the fp32 rounding of the REFERENCE's previous stage (activated output, pre-activation gradient), the
device, the yardstick and the reference alike: a LeakyReLU input within rounding noise of zero (a "sign tie", DESIGN.md
4) then cannot turn one stage's rounding into an O(1) difference of the next, and each kernel is compared on its own.
DESIGN.md 4 has the measured ratios e(device) / e(cpu fp32) per route; CAP_ONLY lists the outputs whose summation
order differs so much from the host's that only the 2e-4 cap holds them.
"""
import ctypes
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

RTOL = 2e-4     # of max|ref64|: never loosened
YARD = 4.0      # times the deviation of the CPU fp32 evaluation

# Same sets as FORCED_TILES of test_gpu_kernels.py: (ALI_BM, ALI_BN, ALI_WBM, ALI_WBN)
FORCED_TILES = {"auto": None, "g64x128_w128x32": (64, 128, 128, 32), "g128x64_w128x64": (128, 64, 128, 64),
                "g128x128_w128x128": (128, 128, 128, 128), "g64x64_w64x64": (64, 64, 64, 64)}

# (case id, output) -> why the 4x yardstick does not apply (the 2e-4 cap still does).  See DESIGN.md 4.
CAP_ONLY = {
    # 128 channels x 6 taps = 768 products per element, which all but the 25 split tiles of the 128x32 launch add up in ONE
    # k-ordered fp32 chain; the host's convolution adds them in blocks.  Measured 1.10e-5 against the host's 2.26e-6
    # (4.9x, 1.5e-6 of max|ref|); the same 768 products added one after the other in fp32 on the CPU give 1.17e-5.
    ("xcd", "dx"): "one 768-term fp32 chain per element against the host's blocked sum",
}


def _ops():
    from ali_hip import ops
    return ops


@pytest.fixture(params=list(FORCED_TILES), ids=list(FORCED_TILES))
def forced_tile(request):
    cfg = FORCED_TILES[request.param]
    if cfg is None:
        yield None
        return
    with _ops().tuning(ALI_BM=cfg[0], ALI_BN=cfg[1], ALI_WBM=cfg[2], ALI_WBN=cfg[3]):
        yield cfg


class Case:
    """One Conv2d layer (kind "conv": B, C, H, W, K, R, S, stride, pad; ``cpad`` = channel stride of x) or one
    ConvTranspose2d layer (kind "convT": C = its input channels, K = its output channels, ``opad`` per axis).
    ``route``: what the host queries must say at the library's own tile choice -- fwd / bwd = (M-tiles, tile rows,
    pixel-major) of ali_conv_fwd / ali_conv_bwd_data, fwd_order / bwd_order = entries of ali_conv_tile_order,
    defer = ali_wgrad_deferrable."""

    def __init__(self, cid, shape, cpad=None, kind="conv", opad=(0, 0), forced=True, **route):
        self.id, self.kind, self.opad, self.forced, self.route = cid, kind, opad, forced, route
        self.B, self.C, self.H, self.W, self.K, self.R, self.S, self.stride, self.pad = shape
        self.cpad = self.C if cpad is None else cpad
        if kind == "conv":
            self.P = (self.H + 2 * self.pad - self.R) // self.stride + 1
            self.Q = (self.W + 2 * self.pad - self.S) // self.stride + 1
        else:       # P, Q: the transposed convolution's OUTPUT map
            self.P = (self.H - 1) * self.stride - 2 * self.pad + self.R + opad[0]
            self.Q = (self.W - 1) * self.stride - 2 * self.pad + self.S + opad[1]

    def geom(self, ops):
        """the AliConvGeom of the layer; a transposed convolution is described by the Conv2d it is the data gradient of"""
        if self.kind == "conv":
            return ops.geom(self.B, self.H, self.W, self.cpad, self.P, self.Q, self.K, self.R, self.S, self.stride, self.pad)
        return ops.geom(self.B, self.P, self.Q, self.K, self.H, self.W, self.cpad, self.R, self.S, self.stride, self.pad)


CASES = [
    # gconv MODE 0 (scalar gathers: channel stride 6, unpadded; the data gradient gathers 10 channels: MODE 0 too);
    # generic wgrad_kernel<.., false, false>, db through ali_colsum
    Case("scalar", (3, 6, 9, 14, 10, 3, 2, 1, 1), fwd=(4, 128, False), bwd=(3, 128, False), fwd_order=0, bwd_order=0, defer=0),
    # MODE 3 (channel stride in {4, 8, 16}: whole taps per k-tile), stride 2 with padding
    Case("pow2", (5, 8, 13, 10, 24, 2, 5, 2, 1), fwd=(2, 128, False), bwd=(8, 128, False), fwd_order=0, bwd_order=0, defer=0),
    # MODE 1 (16-byte gathers, a division per tap: 20 channels).  Weight gradient: wgrad_fast_kernel with a pixel split --
    # the generic wgrad_kernel<.., true, true> is only reachable with operands of 2^30 elements and more
    Case("vec", (4, 20, 7, 12, 40, 4, 3, 1, 0), fwd=(3, 64, False), bwd=(3, 128, False), fwd_order=0, bwd_order=0, defer=1),
    # uniform-tap loop (MODE 2), image-major rows, split-K fold (3 slabs) with the epilogue
    Case("uni-img", (6, 32, 11, 8, 72, 3, 4, 2, 1), fwd=(3, 64, False), bwd=(6, 128, False), fwd_order=0, bwd_order=0, defer=1),
    # pixel-major rows with B = 70 no multiple of the tile height, pad = R - 1 (corner tiles: one live row of taps),
    # taps skipped tile-wide; split-K by default, cost-ordered dispatch with ALI_SPLITK=1
    Case("uni-pix", (70, 64, 5, 9, 96, 3, 5, 1, 2), fwd=(69, 64, True), bwd=(50, 64, True), fwd_order=69, bwd_order=50, defer=1),
    # stride 1, pad 1 ("same" 3x3), pixel-major
    Case("same3", (64, 32, 6, 10, 64, 3, 3, 1, 1), fwd=(60, 64, True), bwd=(30, 128, True), fwd_order=60, bwd_order=30, defer=1),
    # 300 M-tiles x 2 N-tiles = 600 blocks of 64x64: tail split, 88 left-over tiles cut Sr = 2 ways
    Case("tail", (64, 64, 16, 22, 128, 2, 3, 1, 0), forced=False, fwd=(300, 64, True), bwd=(352, 64, True), fwd_order=0,
         bwd_order=352, defer=1),
    # 1050 x 2 = 2100 blocks, image-major: XCD-contiguous order, 8 chunks of 263 with a ragged last one.  Data gradient:
    # 537 tiles of 128x32, tail split
    Case("xcd", (4, 32, 121, 142, 128, 2, 3, 1, 0), forced=False, fwd=(1050, 64, False), bwd=(537, 128, False), fwd_order=0,
         bwd_order=0, defer=1),
    # conv_first_kernel (one image per block; <25, 5> with the live-channel hint, <25> / <9> without),
    # conv_first_wgrad_kernel for the 5x5 ones (Cg_log = 5).  fwd = (images, pixels per image, ..) is ali_conv_mtiles
    # speaking of conv_first_kernel (ali_conv_plan: route 1, asserted below); no host query names
    # conv_first_wgrad_kernel -- only its predicate in ali_conv_bwd_weight (8 -> 32 channels, 5x5, stride 1, pad 0)
    # selects it, which these shapes are chosen to meet
    Case("first-5x5", (64, 5, 12, 20, 32, 5, 5, 1, 0), cpad=8, fwd=(64, 128, False), bwd=(120, 128, True), fwd_order=0,
         bwd_order=120, defer=0),
    Case("first-3x3", (64, 5, 12, 20, 32, 3, 3, 1, 0), cpad=8, fwd=(64, 180, False), bwd=(120, 128, True), fwd_order=0,
         bwd_order=120, defer=0),
    Case("first-tall", (70, 5, 32, 9, 32, 5, 5, 1, 0), cpad=8, fwd=(70, 140, False), bwd=(158, 128, True), fwd_order=0,
         bwd_order=158, defer=0),
    # ... and on a map 3 output pixels wide, where the bias-gradient fold of conv_first_wgrad_kernel needs more LDS than
    # its chunk buffers (db came out wrong there before the launch sized it for both)
    Case("first-narrow", (64, 5, 12, 7, 32, 5, 5, 1, 0), cpad=8, fwd=(64, 24, False), bwd=(42, 128, True), fwd_order=0,
         bwd_order=42, defer=0),
    # conv_s2_first_kernel (a wave walks one output row; Q >= 32, P != Q), 4- and 8-channel strides, pad 1 and 2.
    # ali_conv_plan reports this kernel as route 2 (asserted below).  fwd = (21 / 55, 64, ..) is what ali_conv_mtiles says
    # of the general GEMM, which is NOT launched here (the row-walking kernel has no M-tiles) -- the entries only keep
    # the geometry from drifting
    Case("s2first-c4", (2, 3, 40, 71, 64, 5, 5, 2, 1), cpad=4, fwd=(21, 64, False), bwd=(46, 128, False), fwd_order=0,
         bwd_order=0, defer=1),
    Case("s2first-c8", (3, 7, 69, 66, 64, 5, 5, 2, 2), cpad=8, fwd=(55, 64, False), bwd=(110, 128, False), fwd_order=0,
         bwd_order=0, defer=1),
    # W = 1 / H = 1 maps with a real kernel along the other axis
    Case("1d-col", (5, 32, 50, 1, 48, 5, 1, 2, 0), fwd=(2, 64, False), bwd=(2, 128, False), fwd_order=0, bwd_order=0, defer=1),
    Case("1d-row", (5, 32, 1, 50, 48, 1, 5, 2, 0), fwd=(2, 64, False), bwd=(2, 128, False), fwd_order=0, bwd_order=0, defer=1),
    # forward stride 3 (setup_fwd takes any stride); ali_conv_bwd_data rejects it
    Case("stride3", (3, 16, 14, 20, 32, 4, 2, 3, 1), fwd=(1, 128, False), bwd=(0, 0, False), fwd_order=0, bwd_order=0, defer=0),
    # transposed: four sub-pixel phases with nr != ns and Hq != Wq in every phase
    Case("ct-phase", (3, 32, 4, 7, 24, 5, 3, 2, 1), kind="convT", opad=(1, 0), fwd=(4, 128, False), bwd=(1, 128, False),
         fwd_order=0, bwd_order=0, defer=0),
    # transposed: pixel-major, taps skipped tile-wide (a 1 x 3 map under a 3 x 4 kernel)
    Case("ct-pix", (64, 64, 1, 3, 32, 3, 4, 1, 0), kind="convT", fwd=(9, 128, True), bwd=(3, 64, True), fwd_order=9,
         bwd_order=0, defer=1),
]
BY_ID = {c.id: c for c in CASES}
SQUARE_OK = ("same3", "first-5x5", "first-3x3", "first-tall", "first-narrow", "s2first-c4", "s2first-c8")   # routes that need R == S
CONV_FORCED = [c.id for c in CASES if c.kind == "conv" and c.forced and c.id != "stride3"]
CONV_AUTO = [c.id for c in CASES if c.kind == "conv" and not c.forced]
CONVT = [c.id for c in CASES if c.kind == "convT"]


# ----------------------------------------------------------------------------------------------------------------------
# references (computed once per case, shared by every forced tile and by the CPU test; never modified)

def _inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    t = {"x": torch.randn(c.B, c.C, c.H, c.W, generator=g)}
    if c.kind == "conv":
        t["w"] = torch.randn(c.K, c.C, c.R, c.S, generator=g) / (c.C * c.R * c.S) ** 0.5
    else:
        t["w"] = torch.randn(c.C, c.K, c.R, c.S, generator=g) / (c.C * c.R * c.S / c.stride ** 2) ** 0.5
    t["b"] = torch.randn(c.K, generator=g)
    t["gy"] = torch.randn(c.B, c.K, c.P, c.Q, generator=g)
    t["mask"] = (torch.rand(c.B, c.cpad, generator=g) > 0.3).float() * 1.25          # Dropout2d mask of the layer in front
    t["yprev"] = torch.randn(c.B, c.cpad, c.H, c.W, generator=g)                     # its activated output (leaky, 0.1)
    return t


def _pre(c, x, w, b):
    if c.kind == "conv":
        return F.conv2d(x, w, b, stride=c.stride, padding=c.pad)
    return F.conv_transpose2d(x, w, b, stride=c.stride, padding=c.pad, output_padding=c.opad)


def _stages(c, t, dt, y_in=None, gpre_in=None):
    """all stages of the layer in dtype ``dt``; y_in / gpre_in: the reference's fp32-rounded stage outputs to continue from"""
    x, w, b = (t[k].to(dt).requires_grad_(True) for k in ("x", "w", "b"))
    pre = _pre(c, x, w, b)
    y = F.leaky_relu(pre, 0.2) if c.kind == "conv" else torch.tanh(pre)
    out = {"y": y.detach()}
    y_in = out["y"].float() if y_in is None else y_in
    yi, gy = y_in.to(dt), t["gy"].to(dt)
    one, slope = torch.ones((), dtype=dt), torch.tensor(0.2).to(dt)      # (the device's slope is the fp32 0.2)
    out["gpre"] = gy * (torch.where(yi > 0, one, slope) if c.kind == "conv" else 1 - yi * yi)
    gpre_in = out["gpre"].float() if gpre_in is None else gpre_in
    gp = gpre_in.to(dt)
    out["db"] = gp.sum(dim=(0, 2, 3))
    dx, dw = torch.autograd.grad(pre, (x, w), gp)
    out["dx"], out["dw"] = dx, dw
    m = t["mask"][:, :c.C, None, None].to(dt)
    out["dx_epi"] = dx * m * torch.where(t["yprev"][:, :c.C] > 0, one, torch.tensor(0.1).to(dt))
    return out, y_in, gpre_in


_REF = {}


def reference(c):
    """{"in": inputs, "y_in" / "gpre_in": what the later stages consume, "ref": fp64 outputs, "f32": CPU fp32 outputs}"""
    hit = _REF.get(c.id)
    if hit is None:
        t = _inputs(c)
        ref, y_in, gpre_in = _stages(c, t, torch.float64)
        f32, _, _ = _stages(c, t, torch.float32, y_in, gpre_in)
        hit = _REF[c.id] = {"in": t, "y_in": y_in, "gpre_in": gpre_in, "ref": ref, "f32": f32}
    return hit


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _tile_name():
    import os
    return "x".join(os.environ.get(k, "-") for k in ("ALI_BM", "ALI_BN", "ALI_WBM", "ALI_WBN"))


def check(c, r, name, got, what=None, prefix="GEOM", cap_only=CAP_ONLY):
    """both bounds of the module docstring for output ``name`` of case ``c``; prints the figures before it asserts
    (``prefix`` / ``cap_only``: the line tag and the CAP_ONLY table of the fp16 module, which shares this function)"""
    ref, f32 = r["ref"][name], r["f32"][name]
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (c.id, name, got.shape, ref.shape)
    scale = ref.abs().max().item()
    e_dev = (got - ref).abs().max().item()
    e_cpu = (f32.double() - ref).abs().max().item()
    label = what or name
    print(f"{prefix} case={c.id} tile={_tile_name()} out={label} e_dev={e_dev:.3e} e_cpu={e_cpu:.3e} "
          f"ratio={e_dev / max(e_cpu, 1e-300):.2f} rel={e_dev / max(scale, 1e-300):.2e}")
    assert not math.isnan(e_dev), f"{c.id} {label}: NaN left in the output"
    assert e_dev <= RTOL * scale, f"{c.id} {label}: max err {e_dev:.3e} vs {RTOL} * {scale:.3e}"
    if (c.id, name) not in cap_only:
        assert e_dev <= YARD * e_cpu, f"{c.id} {label}: max err {e_dev:.3e} > {YARD} * {e_cpu:.3e} (CPU fp32)"


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def pack(ops, w, n, t, ch, cpad, s_n, s_tap, s_c):
    dst = nan(n, t, cpad)
    return ops.pack_weights(w.cuda().contiguous(), dst, n, t, ch, cpad, s_n, s_tap, s_c)


def padded_nhwc(t, cpad):
    b, ch, h, w = t.shape
    out = torch.zeros(b, h, w, cpad, device="cuda")
    out[..., :ch] = nhwc(t).cuda()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# routes: what the host side says about every case (runs without a GPU)

def _tile_order_n(ops, geom, which):
    import ali_hip
    buf = (ctypes.c_int32 * 65536)()
    n = ali_hip.load().ali_conv_tile_order(ctypes.byref(geom), which, 0, ctypes.cast(buf, ctypes.c_void_p), 65536)
    assert sorted(buf[:n]) == list(range(n))
    return n


def assert_route(ops, c):
    geom = c.geom(ops)
    # a transposed convolution's forward is ali_conv_bwd_data of its geometry, its data gradient ali_conv_fwd
    fwd, bwd = (0, 1) if c.kind == "conv" else (1, 0)
    assert ops.conv_mtiles(geom, fwd) == c.route["fwd"], (c.id, "fwd", ops.conv_mtiles(geom, fwd))
    assert ops.conv_mtiles(geom, bwd) == c.route["bwd"], (c.id, "bwd", ops.conv_mtiles(geom, bwd))
    assert _tile_order_n(ops, geom, fwd) == c.route["fwd_order"], (c.id, "fwd order")
    assert _tile_order_n(ops, geom, bwd) == c.route["bwd_order"], (c.id, "bwd order")
    assert ops.wgrad_deferrable(geom) == c.route["defer"], (c.id, "deferrable")


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_case_takes_its_route(cid):
    """Host side only: tile count, tile height and row order of both GEMM launches, dispatch-order entries, deferrable
    flag -- and the arithmetic that puts `tail` and `xcd` on their launch shapes (plan_conv's rules), next to what the
    library's own plan says (ops.conv_plan)."""
    ops = _ops()
    ops.reload_tuning()
    c = BY_ID[cid]
    assert_route(ops, c)
    if c.kind == "conv":
        plan = ops.conv_plan(c.geom(ops), 0)
        assert plan.route == (1 if cid.startswith("first-") else 2 if cid.startswith("s2first-") else 0), (cid, plan)
        if plan.route == 0:
            assert (plan.ntile_m, plan.tile_rows, bool(plan.pixel_major)) == c.route["fwd"], (cid, plan)
        if cid == "tail":       # the whole tiles first, the left-over tiles cut two ways (352 blocks of the data gradient: split-K)
            assert (plan.bm, plan.bn, plan.splitk, plan.tail_split, plan.tail_u0, plan.grid_x) == (64, 64, 1, 2, 512, 512 + 2 * 88)
            bwd = ops.conv_plan(c.geom(ops), 1)
            assert bwd.splitk > 1 and bwd.tail_split == 1
        if cid == "xcd":
            assert (plan.xcd_chunk, plan.lin1d, plan.grid_x) == (263, 1, 8 * 263) and plan.tail_split == 1
            assert ops.conv_plan(c.geom(ops), 1).tail_split > 1
    # ali_conv_mtiles reports the tile's height only.  The block counts below take the 64-wide N tile pick_tile pairs
    # with a 64-row tile for the fp32 path (64x64 while blocks(64, 64) <= 16 * 256 CUs; its other tiles are 64x128,
    # reached only beyond that, and 128 rows high): K = 128 makes 2 N-tiles.  Should pick_tile ever pair 64 rows with 128
    # columns at these sizes, the counts halve (300 / 1050 blocks: neither route) and these two shapes must grow.
    if cid == "tail":       # 256 CUs: 512 < blocks < 1024 and blocks % 256 = 88 left-over tiles, cut 2 ways (4 * 88 > 256)
        blocks = c.route["fwd"][0] * ((c.K + 63) // 64)
        assert blocks == 600 and 512 < blocks < 1024 and blocks % 256 == 88
    if cid == "xcd":        # blocks >= 8 * 256, rows image-major, last chunk of (blocks + 7) / 8 ragged
        blocks = c.route["fwd"][0] * ((c.K + 63) // 64)
        assert blocks == 2100 and blocks >= 2048 and blocks % 8 != 0 and not c.route["fwd"][2]


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the inputs can tell a swapped axis from a correct one

def _swap(t):
    return t.transpose(2, 3).contiguous()


def _misread(t):
    """the tensor a kernel would see that exchanged the two spatial extents (strides) of ``t``: same shape, the memory of
    the transposed tensor.  None when that is the identity (an extent of 1)."""
    if min(t.shape[2], t.shape[3]) == 1:
        return None
    return _swap(t).reshape(t.shape)


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_cases_tell_swapped_axes_apart(cid):
    """(1) The fp64 reference of the transposed problem (x, w, gy with their spatial axes exchanged), transposed back,
    equals the reference to 1e-12: the harness treats both axes alike.  (2) With the axes of only ONE operand exchanged
    the outputs that depend on it move by more than 100 x the test's tolerance, so no swap can hide below 2e-4.  Where
    exchanging one operand's axes changes a shape (H != W, R != S: nearly every case) the exchanged operand is the
    transposed tensor's memory read with the original extents -- what a kernel sees that confuses the two strides;
    operands with an extent of 1 are skipped (nothing to exchange).  (3) No case is square in both map and kernel
    unless its route needs it."""
    c = BY_ID[cid]
    assert not (c.H == c.W and c.R == c.S) or cid in SQUARE_OK
    assert c.R != c.S or cid in SQUARE_OK
    r = reference(c)
    t, ref = r["in"], r["ref"]

    def run(x, w, gy, cc):
        x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
        pre = _pre(cc, x, w, t["b"].double())
        dx, dw = torch.autograd.grad(pre, (x, w), gy.double())
        return {"pre": pre.detach(), "dx": dx, "dw": dw}

    gy = r["gpre_in"]
    true = run(t["x"], t["w"], gy, c)
    for k in ("dx", "dw"):       # the same computation as the cached reference
        assert (true[k] - ref[k]).abs().max().item() <= 1e-12 * ref[k].abs().max().item()
    ct = Case(c.id, (c.B, c.C, c.W, c.H, c.K, c.S, c.R, c.stride, c.pad), kind=c.kind, opad=c.opad[::-1])
    tr = run(_swap(t["x"]), _swap(t["w"]), _swap(gy), ct)
    for k in true:
        scale = true[k].abs().max().item()
        assert (_swap(tr[k]) - true[k]).abs().max().item() <= 1e-12 * scale, (cid, k)
    need = {k: 100 * RTOL * true[k].abs().max().item() for k in true}
    seen = 0
    for name, depends in (("x", ("pre", "dw")), ("w", ("pre", "dx")), ("gy", ("dx", "dw"))):
        ops_ = {"x": t["x"], "w": t["w"], "gy": gy}
        bad = _misread(ops_[name])
        if bad is None:
            continue
        ops_[name] = bad
        got = run(ops_["x"], ops_["w"], ops_["gy"], c)
        for k in depends:
            d = (got[k] - true[k]).abs().max().item()
            assert d > need[k], (cid, name, k, d, need[k])
        seen += 1
    assert seen >= 2 or cid.startswith("1d-"), cid      # (the 1-D maps have one extent of 1 in every operand)


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the layers

def _fwd_live_hint(ops, c, r, geom, xh, wf, bias):
    """AliEpilogue.in_ch_live: the padding channels' weights must not matter (conv_first_kernel<25, 5> skips them)"""
    ep = ops.epilogue(bias=bias, act=ops.ACT_LEAKY, slope=0.2)
    ep.in_ch_live = c.C
    wp = wf.clone()
    wp[..., c.C:] = 7.0
    y = nan(c.B, c.P, c.Q, c.K)
    ops.conv_fwd(geom, xh, wp, y, ep)
    check(c, r, "y", nchw(y), "y (live-channel hint)")


def _conv_fwd_stage(ops, c, r, label="y"):
    t = r["in"]
    geom, T = c.geom(ops), c.R * c.S
    xh = padded_nhwc(t["x"], c.cpad)
    wf = pack(ops, t["w"], c.K, T, c.C, c.cpad, c.C * T, 1, T)
    bias = t["b"].cuda()
    y = nan(c.B, c.P, c.Q, c.K)
    ops.conv_fwd(geom, xh, wf, y, ops.epilogue(bias=bias, act=ops.ACT_LEAKY, slope=0.2))
    check(c, r, "y", nchw(y), label)
    return geom, xh, wf, bias


def _conv_dgrad_stage(ops, c, r, geom, gpre, suffix=""):
    t, T = r["in"], c.R * c.S
    wd = torch.zeros(c.cpad, T, c.K, device="cuda")
    ops.pack_weights(t["w"].cuda().contiguous(), wd, c.C, T, c.K, c.K, T, 1, c.C * T)
    dx = nan(c.B, c.H, c.W, c.cpad)
    ops.conv_bwd_data(geom, gpre, wd, dx, ops.epilogue())
    check(c, r, "dx", nchw(dx[..., :c.C]), "dx" + suffix)
    mask, yprev = t["mask"].cuda(), nhwc(t["yprev"]).cuda()
    dxe = nan(c.B, c.H, c.W, c.cpad)
    ops.conv_bwd_data(geom, gpre, wd, dxe, ops.epilogue(mask=mask, dact_y=yprev, dact=ops.ACT_LEAKY, dslope=0.1))
    check(c, r, "dx_epi", nchw(dxe[..., :c.C]), "dx_epi" + suffix)
    if c.cpad != c.C:       # the padding channels of a padded channel stride: exactly zero, with and without the epilogue
        assert dx[..., c.C:].abs().max().item() == 0.0 and dxe[..., c.C:].abs().max().item() == 0.0


def run_conv_case(ops, c, bwd_data=True):
    r = reference(c)
    t, T = r["in"], c.R * c.S
    geom, xh, wf, bias = _conv_fwd_stage(ops, c, r)
    if c.cpad != c.C:
        _fwd_live_hint(ops, c, r, geom, xh, wf, bias)
    # act' and the bias gradient
    y_in, gpre = nhwc(r["y_in"]).cuda(), nhwc(r["gpre_in"]).cuda()
    out = nan(c.B, c.P, c.Q, c.K)
    ops.act_bwd(nhwc(t["gy"]).cuda(), y_in, ops.ACT_LEAKY, 0.2, out=out)
    check(c, r, "gpre", nchw(out))
    db = nan(c.K)
    ops.colsum(c.B * c.P * c.Q, c.K, c.K, gpre, out=db)
    check(c, r, "db", db, "db (colsum)")
    if bwd_data:
        _conv_dgrad_stage(ops, c, r, geom, gpre)
    dw, db2 = nan(c.K, c.C, c.R, c.S), nan(c.K)
    ops.conv_bwd_weight(geom, xh, gpre, dw, c.C, c.K, c.C * T, T, 1, db=db2)
    check(c, r, "dw", dw)
    check(c, r, "db", db2, "db (fused into wgrad)")
    return geom, xh, gpre


@gpu
@pytest.mark.parametrize("cid", CONV_FORCED)
def test_conv_layer_on_its_route(cid, forced_tile):
    """forward (bias + LeakyReLU), act' + column sum, data gradient plain and with mask + act' epilogue, weight gradient
    with the fused bias gradient, every output buffer pre-filled with NaN, under every forced tile"""
    ops = _ops()
    c = BY_ID[cid]
    if forced_tile is None:
        assert_route(ops, c)
    geom, xh, gpre = run_conv_case(ops, c)
    if cid == "uni-pix":
        # by default both GEMMs split K (138 / 50 blocks) and a split launch ignores the dispatch-order table: with
        # ALI_SPLITK=1 every block owns a whole k-loop and the launch follows the table ops uploads; ALI_NO_ORDER=1 is
        # the natural order.  Both against the reference (not against each other).
        r = reference(c)
        for env, tag in (({"ALI_SPLITK": 1}, " (cost-ordered)"), ({"ALI_SPLITK": 1, "ALI_NO_ORDER": 1}, " (natural order)")):
            with ops.tuning(**env):
                for which in (0, 1):
                    assert _tile_order_n(ops, geom, which) == ops.conv_mtiles(geom, which)[0] > 0
                    assert ops.conv_tile_order(geom, which, torch.device("cuda", torch.cuda.current_device())) is not None
                _conv_fwd_stage(ops, c, r, "y" + tag)
                _conv_dgrad_stage(ops, c, r, geom, gpre, tag)


@gpu
@pytest.mark.parametrize("cid", CONV_AUTO)
def test_conv_layer_on_its_launch_shape(cid):
    """the tail split and the XCD-contiguous tile order with an epilogue, against the reference (library's own tile only:
    the block count is the route)"""
    ops = _ops()
    c = BY_ID[cid]
    assert_route(ops, c)
    run_conv_case(ops, c)


@gpu
def test_forward_stride_3_and_its_rejected_data_gradient(forced_tile):
    """setup_fwd takes any stride: forward and weight gradient against the reference.  ali_conv_bwd_data takes strides 1
    and 2: ALI_ERR_BAD_ARG, the text names the stride, dx is not touched."""
    ops = _ops()
    c = BY_ID["stride3"]
    geom, xh, gpre = run_conv_case(ops, c, bwd_data=False)
    T = c.R * c.S
    wd = torch.zeros(c.cpad, T, c.K, device="cuda")
    dx = nan(c.B, c.H, c.W, c.cpad)
    with pytest.raises(RuntimeError, match=r"rc=-1\).*stride 3 unsupported"):
        ops.conv_bwd_data(geom, gpre, wd, dx, ops.epilogue())
    torch.cuda.synchronize()
    assert torch.isnan(dx).all()
    assert ops.conv_mtiles(geom, 1) == (0, 0, False)


@gpu
@pytest.mark.parametrize("cid", CONVT)
def test_transposed_conv_layer_on_its_route(cid, forced_tile):
    """ConvTranspose2d: forward = ali_conv_bwd_data with bias + tanh, data gradient = ali_conv_fwd (plain and with the
    mask + act' epilogue), weight gradient with swapped operands"""
    ops = _ops()
    c = BY_ID[cid]
    if forced_tile is None:
        assert_route(ops, c)
    r = reference(c)
    t, T = r["in"], c.R * c.S
    geom = c.geom(ops)                                   # x := the layer's output (K channels), y := its input
    xh = padded_nhwc(t["x"], c.cpad)
    wf = pack(ops, t["w"], c.K, T, c.C, c.cpad, T, 1, c.K * T)
    bias = t["b"].cuda()
    y = nan(c.B, c.P, c.Q, c.K)
    ops.conv_bwd_data(geom, xh, wf, y, ops.epilogue(bias=bias, act=ops.ACT_TANH))
    check(c, r, "y", nchw(y))
    y_in, gpre = nhwc(r["y_in"]).cuda(), nhwc(r["gpre_in"]).cuda()
    out = nan(c.B, c.P, c.Q, c.K)
    ops.act_bwd(nhwc(t["gy"]).cuda(), y_in, ops.ACT_TANH, 0.0, out=out)
    check(c, r, "gpre", nchw(out))
    db = nan(c.K)
    ops.colsum(c.B * c.P * c.Q, c.K, c.K, gpre, out=db)
    check(c, r, "db", db, "db (colsum)")
    wd = pack(ops, t["w"], c.C, T, c.K, c.K, c.K * T, 1, T)
    dx = nan(c.B, c.H, c.W, c.cpad)
    ops.conv_fwd(geom, gpre, wd, dx, ops.epilogue())
    check(c, r, "dx", nchw(dx))
    mask, yprev = t["mask"].cuda(), nhwc(t["yprev"]).cuda()
    dxe = nan(c.B, c.H, c.W, c.cpad)
    ops.conv_fwd(geom, gpre, wd, dxe, ops.epilogue(mask=mask, dact_y=yprev, dact=ops.ACT_LEAKY, dslope=0.1))
    check(c, r, "dx_epi", nchw(dxe))
    dw = nan(c.C, c.K, c.R, c.S)
    ops.conv_bwd_weight(geom, gpre, xh, dw, c.K, c.C, c.K * T, T, 1)
    check(c, r, "dw", dw)


# ----------------------------------------------------------------------------------------------------------------------
# GPU: branches of ali_conv_bwd_weight the wrappers never take

def _bwd_weight_raw(ops, geom, x, dy, dst, cg, cd, s_dc, s_gc, s_tap, db, pixtab):
    """ali_conv_bwd_weight through the C ABI itself (ops.conv_bwd_weight always passes a pixel table on the fast path)"""
    import ali_hip
    from ali_hip import _lib
    ws = ops.workspace(x.device)
    rc = ali_hip.load().ali_conv_bwd_weight(
        ctypes.byref(geom), x.data_ptr(), dy.data_ptr(), dst.data_ptr(), cg, cd, s_dc, s_gc, s_tap, db.data_ptr(),
        None if pixtab is None else pixtab.data_ptr(), 0, None, None, 0, None, None, 0, ws.data_ptr(), ws.numel(),
        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ali_conv_bwd_weight")


@gpu
@pytest.mark.parametrize("cid", ["uni-img", "uni-pix"])
def test_weight_gradient_without_pixel_table(cid, forced_tile):
    """`pixtab` is optional: wgrad_fast_kernel<.., TAB = false> computes its gather addresses itself.  Against the
    reference under every forced weight-gradient tile, and bit for bit what the table-fed launch gives at the same
    pixel split (ALI_WGRAD_BLOCKS pins the split target for both)."""
    ops = _ops()
    c = BY_ID[cid]
    r = reference(c)
    T = c.R * c.S
    geom = c.geom(ops)
    xh, gpre = padded_nhwc(r["in"]["x"], c.cpad), nhwc(r["gpre_in"]).cuda()
    with ops.tuning(ALI_WGRAD_BLOCKS=1024):
        outs = []
        for tab in (None, ops.wgrad_pixtab(geom, xh.device)):
            dw, db = nan(c.K, c.C, c.R, c.S), nan(c.K)
            _bwd_weight_raw(ops, geom, xh, gpre, dw, c.C, c.K, c.C * T, T, 1, db, tab)
            tag = "no pixel table" if tab is None else "pixel table"
            check(c, r, "dw", dw, f"dw ({tag})")
            check(c, r, "db", db, f"db ({tag})")
            outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _wgrad_maybe_deferred(ops, deferred, geom, x, dy, dst, cg, cd, strides, db):
    if not deferred:
        ops.conv_bwd_weight(geom, x, dy, dst, cg, cd, *strides, db=db)
        return
    q = ops.FoldQueue(torch.device("cuda", torch.cuda.current_device()))
    q.expect([geom])
    ops.conv_bwd_weight(geom, x, dy, dst, cg, cd, *strides, db=db, defer=q)
    assert len(q.launches) == 1 and len(q.jobs) == 1 and torch.isnan(dst).all()      # GEMM and fold both deferred
    q.flush()


@gpu
@pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("cid", ["uni-img", "uni-pix"])
def test_weight_gradient_in_packed_layout(cid, deferred):
    """dst strides other than [K, C, R, S]-contiguous: the forward pack's [K][R*S][C] (s_dc = T*C, s_gc = 1, s_tap = C),
    written by wgrad_reduce_tile_kernel (immediate) and wgrad_fold_multi_kernel (ops.FoldQueue) with R != S -- against the
    reference, and the untouched rest of the buffer stays NaN"""
    ops = _ops()
    c = BY_ID[cid]
    r = reference(c)
    T = c.R * c.S
    geom = c.geom(ops)
    xh, gpre = padded_nhwc(r["in"]["x"], c.cpad), nhwc(r["gpre_in"]).cuda()
    buf, db = nan(c.K * T * c.C + 5), nan(c.K)
    _wgrad_maybe_deferred(ops, deferred, geom, xh, gpre, buf, c.C, c.K, (T * c.C, 1, c.C), db)
    dw = buf[:c.K * T * c.C].reshape(c.K, c.R, c.S, c.C).permute(0, 3, 1, 2)
    check(c, r, "dw", dw, "dw ([K][R*S][C])")
    check(c, r, "db", db, "db ([K][R*S][C])")
    assert torch.isnan(buf[c.K * T * c.C:]).all()


_LINEAR = {}


@gpu
@pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "deferred"])
def test_weight_gradient_with_linear_strides(deferred):
    """nn.Linear as a 1x1 convolution on a 1x1 map: dW [out][in] = (in, 1, 0) strides (what chain.py passes), 200 rows so
    that the launch splits the pixel range and the slab fold writes the strided result"""
    ops = _ops()
    B, I, O = 200, 96, 40
    c = Case("linear", (B, I, 1, 1, O, 1, 1, 1, 0))
    if not _LINEAR:
        g = torch.Generator().manual_seed(17)
        x, gy = torch.randn(B, I, generator=g), torch.randn(B, O, generator=g)
        _LINEAR.update(x=x, gy=gy, ref={"dw": gy.double().t() @ x.double(), "db": gy.double().sum(0)},
                       f32={"dw": gy.t() @ x, "db": gy.sum(0)})
    r = _LINEAR
    geom = c.geom(ops)
    assert ops.wgrad_deferrable(geom) == 1
    dw, db = nan(O, I), nan(O)
    _wgrad_maybe_deferred(ops, deferred, geom, r["x"].cuda().reshape(B, 1, 1, I), r["gy"].cuda().reshape(B, 1, 1, O), dw,
                          I, O, (I, 1, 0), db)
    check(c, r, "dw", dw, "dw (Linear strides)")
    check(c, r, "db", db, "db (Linear strides)")
