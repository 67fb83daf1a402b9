"""Fixed cost of a tile in the fp32 MFMA GEMM kernel (csrc/gconv.hip MODE 2; DESIGN.md 3.1 "Fixed cost of a tile").

A *uniform* tile -- rows ordered (pixel, image), B a multiple of the tile height -- derives its tap mask, live-tap list,
row tables and gather offsets from block-uniform scalars and issues its first gathers before any barrier;
ALI_NO_UNIFORM=1 sends every tile through the general per-row prologue.  The switch changes no stored value, so every
case runs twice -- with and without it -- and requires BIT-EQUAL outputs, BatchNorm partials included; one run of the
pair is compared with torch on the CPU at the tolerance tests/test_gpu_kernels.py uses for the kernel.  (The second
half of that work, the epilogue's operands in one batch of buffer loads, was measured and rejected -- DESIGN.md 3.1 --
so there is no switch for it; the epilogue cases stay, because the epilogue reads the row tables the uniform prologue
fills.)  The shapes are the smallest at which each piece can go wrong: one / two tiles per pixel position against tiles
that straddle positions, ragged M and N, sub-pixel phases, image-major rows, every epilogue flavour on full and ragged
tiles, paired BatchNorm passes, split-K (an empty k-slice included), the tail split, a multi-job launch with two
epilogues and a uniform and a straddling job, every tile shape, and the MODE 3 kernel, which must not notice."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL = 2e-4   # tests/test_gpu_kernels.py: fp32 MFMA = fp32 fma chain, only the summation order differs from the CPU
SLOPE, DSLOPE = 0.2, 0.1


def _ops():
    from ali_hip import ops
    return ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(got, ref, rtol=RTOL, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def pack_fwd(ops, w):                       # [K, C, R, S] -> [K, R*S, C]
    K, C, R, S = w.shape
    dst = torch.empty(K, R * S, C, device="cuda")
    return ops.pack_weights(w.cuda().contiguous(), dst, K, R * S, C, C, C * R * S, 1, R * S)


def both_paths(run, **knobs):
    """run() -> tuple of tensors, once with the uniform prologue and once with ALI_NO_UNIFORM=1 (ops.tuning reloads the
    library's knobs on entry and exit); the two must agree bit for bit.  Returns the first run's outputs."""
    ops = _ops()
    with ops.tuning(**knobs):
        new = run()
    with ops.tuning(ALI_NO_UNIFORM=1, **knobs):
        old = run()
    torch.cuda.synchronize()
    assert len(new) == len(old)
    for i, (a, b) in enumerate(zip(new, old)):
        assert not torch.isnan(a).any(), f"output {i}: NaN left"
        assert torch.equal(a, b), (f"output {i}: uniform prologue != general prologue, "
                                   f"max diff {(a - b).abs().max().item():.3e}")
    return new


def check_uniform(geom, which, B, expected, **knobs):
    """The launch's tiles are uniform exactly when its rows are ordered (pixel, image) and B is a multiple of the tile
    height (what the host tests); a case meant for one prologue must not quietly run the other against itself."""
    ops = _ops()
    with ops.tuning(**knobs):
        _, rows, pixel_major = ops.conv_mtiles(geom, which)
    assert (pixel_major and B % rows == 0) == expected, (pixel_major, rows, B)


T64 = dict(ALI_BM=64, ALI_BN=64)            # the 64 x 64 tile the shapes below are sized for

FLAVOURS = ["plain", "mask", "mask+dact", "dact", "mask_ld+out_ld", "bn1", "bn1+stat_mask", "bn2", "bn2+in",
            "bn2+in+pre"]


def part_sums(part, K):
    """bn_part[(s*K + n) * slots + slot] -> [2, K] column sums over the slots (in double: the slots are few)"""
    return part.double().reshape(2, K, -1).sum(dim=2).float()


def conv_ep_case(B, C, H, K, R, stride, pad, flavour, seed, uniform, **knobs):
    """Conv2d forward B x C x H x H -> K channels with one epilogue flavour; new == old bit for bit, new ~ CPU.
    uniform: whether the launch's tiles must be uniform ones."""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g)
    pre = F.conv2d(x, w, b, stride=stride, padding=pad)
    P = pre.shape[2]
    mask = (torch.rand(B, K, generator=g) > 0.3).float() * 1.25
    mask2 = (torch.rand(B, K, generator=g) > 0.5).float() * 2.0
    yprev = torch.randn(B, K, P, P, generator=g)             # the saved activation act' is evaluated on
    mean, invstd = torch.randn(K, generator=g), torch.rand(K, generator=g) + 0.5
    dgrad = torch.where(yprev > 0, torch.ones(()), torch.full((), DSLOPE))
    bn = flavour.startswith("bn")
    has_mask = flavour in ("mask", "mask+dact", "mask_ld+out_ld", "bn1+stat_mask")
    v = pre if flavour.startswith("bn2") else F.leaky_relu(pre, SLOPE)
    if has_mask:
        v = v * mask[:, :, None, None]
    if "dact" in flavour:
        v = v * dgrad
    sums = None
    if flavour.startswith("bn1"):
        vt = v * mask2[:, :, None, None] if flavour == "bn1+stat_mask" else v
        sums = torch.stack([vt.sum(dim=(0, 2, 3)), (vt * vt).sum(dim=(0, 2, 3))])
    if flavour.startswith("bn2"):
        m_in = mask if "in" in flavour else None
        m_pre = mask2 if "pre" in flavour else None
        gt = v * m_pre[:, :, None, None] if m_pre is not None else v
        xin = yprev * m_in[:, :, None, None] if m_in is not None else yprev
        xhat = (xin - mean[None, :, None, None]) * invstd[None, :, None, None]
        sums = torch.stack([(gt * xhat).sum(dim=(0, 2, 3)), gt.sum(dim=(0, 2, 3))])

    geom = ops.geom(B, H, H, C, P, P, K, R, R, stride, pad)
    check_uniform(geom, 0, B, uniform, **knobs)
    xh, wp, bc = nhwc(x).cuda(), pack_fwd(ops, w), b.cuda()
    mk, mk2, yp = mask.cuda(), mask2.cuda(), nhwc(yprev).cuda()
    mean_c, invstd_c = mean.cuda(), invstd.cuda()
    ld, off = K + 96, 32
    mask_w = torch.zeros(B, ld, device="cuda")
    mask_w[:, off:off + K] = mk

    def run():
        y = torch.full((B, P, P, K), float("nan"), device="cuda")
        act = dict(bias=bc, act=ops.ACT_LEAKY, slope=SLOPE)
        if flavour == "plain":
            ops.conv_fwd(geom, xh, wp, y, ops.epilogue(**act))
        elif flavour == "mask":
            ops.conv_fwd(geom, xh, wp, y, ops.epilogue(mask=mk, **act))
        elif flavour == "mask+dact":
            ops.conv_fwd(geom, xh, wp, y, ops.epilogue(mask=mk, dact_y=yp, dact=ops.ACT_LEAKY, dslope=DSLOPE, **act))
        elif flavour == "dact":
            ops.conv_fwd(geom, xh, wp, y, ops.epilogue(dact_y=yp, dact=ops.ACT_LEAKY, dslope=DSLOPE, **act))
        elif flavour == "mask_ld+out_ld":
            wide = torch.full((B, P, P, ld), 3.0, device="cuda")
            ep = ops.epilogue(**act)
            ep.mask, ep.mask_ld = mask_w[:, off:off + K].data_ptr(), ld
            ops.conv_fwd(geom, xh, wp, wide[..., off:off + K], ep, out_ld=ld)
            assert (wide[..., :off] == 3.0).all() and (wide[..., off + K:] == 3.0).all(), "stored outside its columns"
            y = wide[..., off:off + K].contiguous()
        else:
            slots = ops.conv_mtiles(geom, 0)[0]                # (under the knobs in force)
            part = torch.full((2 * K * slots,), float("nan"), device="cuda")
            if flavour == "bn1":
                ops.conv_fwd(geom, xh, wp, y, ops.epilogue(bn_fwd=(part, 1, None, slots), **act))
            elif flavour == "bn1+stat_mask":
                ops.conv_fwd(geom, xh, wp, y, ops.epilogue(mask=mk, bn_fwd=(part, 1, mk2, slots), **act))
            else:
                m_in = mk if "in" in flavour else None
                m_pre = mk2 if "pre" in flavour else None
                ops.conv_fwd(geom, xh, wp, y, ops.epilogue(bias=bc, bn_bwd=(part, yp, mean_c, invstd_c, m_in, m_pre, slots)))
            return y, part
        return (y,)

    out = both_paths(run, **knobs)
    close(nchw(out[0]), v, what=f"conv fwd, {flavour}")
    if bn:
        close(part_sums(out[1], K), sums, what=f"BatchNorm partials, {flavour}")


@pytest.mark.parametrize("B,pad", [(64, 1), (128, 1), (96, 1), (64, 0)])
def test_uniform_and_straddling_tiles(B, pad):
    """6 x 6 map, 3 x 3 stride 1, 32 -> 64 channels, rows ordered (pixel, image).  Padded: B = 64 is one pixel position
    per 64-row tile (border tiles have dead taps), B = 128 two tiles per position, B = 96 tiles that straddle two
    positions and must take the general prologue.  Unpadded at B = 64: no dead tap anywhere."""
    conv_ep_case(B, 32, 6, 64, 3, 1, pad, "mask+dact", seed=B + pad, uniform=B != 96, **T64)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("B,K", [(64, 64), (70, 72)])
def test_every_epilogue_flavour_on_full_and_ragged_tiles(B, K, flavour):
    """The padded 3 x 3 conv with each epilogue flavour.  B = 64, K = 64: uniform, full tiles.  B = 70, K = 72: the last
    M-tile holds absent rows, the last n-tile absent columns -- nothing may be stored or summed for them."""
    conv_ep_case(B, 32, 6, K, 3, 1, 1, flavour, seed=B + len(flavour), uniform=B == 64, **T64)


def test_paired_batchnorm_passes_slot_mapping():
    """bn_groups = 2 at B = 128 (two passes of 64 images back to back): the slot of a tile depends on its pixel
    position and its pass; 64-row tiles, two per position."""
    ops = _ops()
    B, C, H, K, R = 128, 32, 6, 64, 3
    g = torch.Generator().manual_seed(29)
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    smask = (torch.rand(B, K, generator=g) > 0.4).float() * 1.5
    ref = F.conv2d(x, w, padding=1)
    vt = ref * smask[:, :, None, None]
    sums = torch.stack([torch.stack([vt[p * 64:(p + 1) * 64].sum(dim=(0, 2, 3)),
                                     (vt[p * 64:(p + 1) * 64] ** 2).sum(dim=(0, 2, 3))]) for p in range(2)])  # [pass, 2, K]
    geom = ops.geom(B, H, H, C, H, H, K, R, R, 1, 1)
    check_uniform(geom, 0, B, True, **T64)
    xh, wp, sm = nhwc(x).cuda(), pack_fwd(ops, w), smask.cuda()

    def run():
        slots = ops.conv_mtiles(geom, 0)[0]
        part = torch.full((2 * K * slots,), float("nan"), device="cuda")
        y = torch.full((B, H, H, K), float("nan"), device="cuda")
        ops.conv_fwd(geom, xh, wp, y, ops.epilogue(bn_fwd=(part, 2, sm, slots)))
        return y, part

    y, part = both_paths(run, **T64)
    close(nchw(y), ref, what="conv fwd, paired passes")
    per_pass = part.double().reshape(2, K, 2, -1).sum(dim=3).permute(2, 0, 1).float()     # slots of pass g: contiguous
    close(per_pass, sums, what="BatchNorm partials per pass")


def test_stride2_transposed_conv_phases_and_its_data_gradient():
    """ConvTranspose2d 3 x 3 stride 2, 3 x 3 -> 7 x 7, 32 -> 32 channels, B = 64: four sub-pixel phases with 4 / 2 / 2 / 1
    taps, each with its own border and its own tile range (with a Dropout2d mask); then the gradient w.r.t. its input
    (a stride-2 unpadded conv) with the act' operand."""
    ops = _ops()
    B, Ci, Co, H, R = 64, 32, 32, 3, 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Ci, H, H, generator=g)
    w = torch.randn(Ci, Co, R, R, generator=g) / (Ci * R * R / 4) ** 0.5
    mask = (torch.rand(B, Co, generator=g) > 0.3).float() * 1.25
    xr = x.clone().requires_grad_(True)
    yr = F.conv_transpose2d(xr, w, stride=2)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    yprev = torch.randn(B, Ci, H, H, generator=g)
    dgrad = torch.where(yprev > 0, torch.ones(()), torch.full((), DSLOPE))
    Ho, T = yr.shape[2], R * R
    geom = ops.geom(B, Ho, Ho, Co, H, H, Ci, R, R, 2, 0)          # the conv this transposed conv is the dgrad of
    wf = torch.empty(Co, T, Ci, device="cuda")
    ops.pack_weights(w.cuda().contiguous(), wf, Co, T, Ci, Ci, T, 1, Co * T)
    wd = torch.empty(Ci, T, Co, device="cuda")
    ops.pack_weights(w.cuda().contiguous(), wd, Ci, T, Co, Co, Co * T, 1, T)
    check_uniform(geom, 1, B, True, **T64)
    check_uniform(geom, 0, B, True, **T64)
    xh, gh, mk, yp = nhwc(x).cuda(), nhwc(gy).cuda(), mask.cuda(), nhwc(yprev).cuda()

    def run():
        y = torch.full((B, Ho, Ho, Co), float("nan"), device="cuda")
        ops.conv_bwd_data(geom, xh, wf, y, ops.epilogue(mask=mk))
        dx = torch.full((B, H, H, Ci), float("nan"), device="cuda")
        ops.conv_fwd(geom, gh, wd, dx, ops.epilogue(dact_y=yp, dact=ops.ACT_LEAKY, dslope=DSLOPE))
        return y, dx

    y, dx = both_paths(run, **T64)
    close(nchw(y), yr * mask[:, :, None, None], what="convT fwd")
    close(nchw(dx), xr.grad * dgrad, what="convT dgrad")


def test_image_major_rows_are_never_uniform():
    """40 x 40 map, 5 x 5 stride 2 pad 2, 32 -> 64 channels, B = 2: rows ordered (image, pixel), ragged last tile."""
    conv_ep_case(2, 32, 40, 64, 5, 2, 2, "mask+dact", seed=3, uniform=False, **T64)


def gemm_case(M, C, K, seed, **knobs):
    """1 x 1 GEMM M x C x K with mask + act' operand (every row is its own image: uniform tiles)"""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g)
    w = torch.randn(K, C, generator=g) / C ** 0.5
    mask = (torch.rand(M, K, generator=g) > 0.3).float() * 1.25
    yprev = torch.randn(M, K, generator=g)
    ref = (x @ w.t()) * mask * torch.where(yprev > 0, torch.ones(()), torch.full((), DSLOPE))
    geom = ops.geom(M, 1, 1, C, 1, 1, K, 1, 1, 1, 0)
    check_uniform(geom, 0, M, True, **knobs)
    xh, wp = x.reshape(M, 1, 1, C).cuda(), w.reshape(K, 1, C).cuda().contiguous()
    mk, yp = mask.cuda(), yprev.reshape(M, 1, 1, K).cuda()

    def run():
        y = torch.full((M, 1, 1, K), float("nan"), device="cuda")
        ops.conv_fwd(geom, xh, wp, y, ops.epilogue(mask=mk, dact_y=yp, dact=ops.ACT_LEAKY, dslope=DSLOPE))
        return (y,)

    (y,) = both_paths(run, **knobs)
    close(y.reshape(M, K), ref, what="1x1 GEMM")


@pytest.mark.parametrize("C", [1024, 128])
def test_forced_split_k_applies_the_operands_once(C):
    """M = 128, K = 64, ALI_SPLITK=3.  C = 1024: 32 k-tiles in slices of 11 + 11 + 10.  C = 128: 4 k-tiles in slices of
    2 + 2 + 0 -- the third block has nothing to multiply and still has to fill its row tables, deliver its (zero)
    slab and, if it arrives last, run the epilogue."""
    gemm_case(128, C, 64, seed=C, ALI_SPLITK=3, **T64)


def test_tail_split_launch_with_a_mask():
    """The 19200 x 288 x 128 launch of tests/test_gpu_clean_tiles.py (512 whole tiles, then 88 tiles cut two ways
    along K), here with epilogue operands."""
    gemm_case(300 * 64, 288, 128, seed=5, **T64)


def test_multi_job_launch_with_two_epilogues():
    """One launch, two jobs: a uniform one (B = 64, unpadded) with a Dropout2d mask and a straddling one (B = 96,
    padded) with the BatchNorm backward sums."""
    ops = _ops()
    g = torch.Generator().manual_seed(17)
    C, H, K, R = 32, 6, 64, 3
    jobs = []
    for (B, pad) in [(64, 0), (96, 1)]:
        x = torch.randn(B, C, H, H, generator=g)
        w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
        ref = F.conv2d(x, w, padding=pad)
        P = ref.shape[2]
        jobs.append(dict(B=B, P=P, geom=ops.geom(B, H, H, C, P, P, K, R, R, 1, pad), x=nhwc(x).cuda(), w=pack_fwd(ops, w),
                         ref=ref))
    check_uniform(jobs[0]["geom"], 0, 64, True, **T64)
    check_uniform(jobs[1]["geom"], 0, 96, False, **T64)
    mask = (torch.rand(64, K, generator=g) > 0.3).float() * 1.25
    bnx = torch.randn(96, K, jobs[1]["P"], jobs[1]["P"], generator=g)
    mean, invstd = torch.randn(K, generator=g), torch.rand(K, generator=g) + 0.5
    m_in = (torch.rand(96, K, generator=g) > 0.5).float() * 2.0
    xhat = (bnx * m_in[:, :, None, None] - mean[None, :, None, None]) * invstd[None, :, None, None]
    sums = torch.stack([(jobs[1]["ref"] * xhat).sum(dim=(0, 2, 3)), jobs[1]["ref"].sum(dim=(0, 2, 3))])
    mk, bx, mc, ic, mi = mask.cuda(), nhwc(bnx).cuda(), mean.cuda(), invstd.cuda(), m_in.cuda()

    def run():
        outs = [torch.full((j["B"], j["P"], j["P"], K), float("nan"), device="cuda") for j in jobs]
        slots = ops.conv_mtiles(jobs[1]["geom"], 0)[0]
        part = torch.full((2 * K * slots,), float("nan"), device="cuda")
        with ops.gemm_batch() as batch:
            ops.conv_fwd(jobs[0]["geom"], jobs[0]["x"], jobs[0]["w"], outs[0], ops.epilogue(mask=mk))
            ops.conv_fwd(jobs[1]["geom"], jobs[1]["x"], jobs[1]["w"], outs[1],
                         ops.epilogue(bn_bwd=(part, bx, mc, ic, mi, None, slots)))
            assert len(batch.jobs) == 2
        return outs[0], outs[1], part

    y0, y1, part = both_paths(run, **T64)
    close(nchw(y0), jobs[0]["ref"] * mask[:, :, None, None], what="multi-job conv, mask")
    close(nchw(y1), jobs[1]["ref"], what="multi-job conv, bn_mode 2")
    close(part_sums(part, K), sums, what="multi-job BatchNorm partials")


@pytest.mark.parametrize("bm,bn", [(64, 64), (128, 32), (64, 128), (128, 64), (128, 128)])
def test_every_fp32_tile_shape(bm, bn):
    """The padded 3 x 3 conv at B = 128 (uniform for 64- and 128-row tiles) with mask + act' operand on every fp32 tile."""
    conv_ep_case(128, 32, 6, 64, 3, 1, 1, "mask+dact", seed=bm + bn, uniform=True, ALI_BM=bm, ALI_BN=bn)


def test_small_channel_stride_kernel_is_untouched():
    """Channel stride 8 (MODE 3; the geometry would be uniform, the kernel has no such prologue): the switch may not
    change anything."""
    conv_ep_case(64, 8, 6, 64, 3, 1, 1, "mask", seed=8, uniform=True, **T64)
