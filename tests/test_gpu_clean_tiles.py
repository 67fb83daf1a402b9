"""Clean-tile fast path of the fp32 MFMA loops (csrc/gconv.hip MODE 2, csrc/wgrad.hip TAB path).

A tile whose gathers cannot be dead runs a k-loop without per-gather predicates; ALI_NO_CLEAN=1 forces the general loop
everywhere.  Both loops stage the same LDS image in the same k order, so every case here runs twice -- with and without
the switch -- and requires BIT-EQUAL outputs; one run of the pair is also compared with torch on the CPU at the
tolerance tests/test_gpu_kernels.py uses for the kernel.  The shapes are the smallest that exercise each way the clean
flag can go wrong: dead taps that are tile-uniform, tiles that straddle pixel positions, ragged M / N, the sub-pixel
phases of a transposed conv, k-ranges that end early (split-K, tail split), image-major rows, multi-job launches, and
weight-gradient blocks whose taps are / are not in range for every pixel."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL = 2e-4   # tests/test_gpu_kernels.py: fp32 MFMA = fp32 fma chain, only the summation order differs from the CPU


def _ops():
    from ali_hip import ops
    return ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(got, ref, rtol=RTOL, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def pack_fwd(ops, w):                       # [K, C, R, S] -> [K, R*S, C]
    K, C, R, S = w.shape
    dst = torch.empty(K, R * S, C, device="cuda")
    return ops.pack_weights(w.cuda().contiguous(), dst, K, R * S, C, C, C * R * S, 1, R * S)


def pack_dgrad(ops, w):                     # [K, C, R, S] -> [C, R*S, K]
    K, C, R, S = w.shape
    dst = torch.zeros(C, R * S, K, device="cuda")
    ops.pack_weights(w.cuda().contiguous(), dst, C, R * S, K, K, R * S, 1, C * R * S)
    return dst


def both_loops(run, **knobs):
    """run() -> tuple of tensors, once on the clean-tile path and once with ALI_NO_CLEAN=1 (ops.tuning reloads the
    library's knobs on entry and exit); the two must agree bit for bit.  Returns the clean-path outputs."""
    ops = _ops()
    with ops.tuning(**knobs):
        clean = run()
    with ops.tuning(ALI_NO_CLEAN=1, **knobs):
        general = run()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(clean, general)):
        assert not torch.isnan(a).any(), f"output {i}: NaN left"
        assert torch.equal(a, b), f"output {i}: clean loop != general loop, max diff {(a - b).abs().max().item():.3e}"
    return clean


T64 = dict(ALI_BM=64, ALI_BN=64)            # the 64 x 64 tile the shapes below are sized for


def conv_case(B, C, H, K, R, stride, pad, seed, **knobs):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g)
    ref = F.leaky_relu(F.conv2d(x, w, b, stride=stride, padding=pad), 0.2)
    P = ref.shape[2]
    geom = ops.geom(B, H, H, C, P, P, K, R, R, stride, pad)
    xh, wp, bc = nhwc(x).cuda(), pack_fwd(ops, w), b.cuda()

    def run():
        y = torch.full((B, P, P, K), float("nan"), device="cuda")
        ops.conv_fwd(geom, xh, wp, y, ops.epilogue(bias=bc, act=ops.ACT_LEAKY, slope=0.2))
        return (y,)

    (y,) = both_loops(run, **knobs)
    close(nchw(y), ref, what="conv fwd")


@pytest.mark.parametrize("B", [64, 96])
def test_padded_3x3_conv_uniform_and_straddling_tiles(B):
    """6 x 6 map, 3 x 3 stride 1 pad 1, 32 -> 64 channels, rows ordered (pixel, image).  B = 64: one pixel position
    per 64-row tile -- edge tiles have dead taps, all tile-uniform (clean).  B = 96: tiles straddle two positions, so
    one launch holds clean and non-clean tiles side by side."""
    conv_case(B, 32, 6, 64, 3, 1, 1, seed=B, **T64)


def test_ragged_m_and_n_take_the_general_loop():
    """B = 70 (the last M-tile holds absent rows) and K = 72 (the last n-tile holds absent weight rows)."""
    conv_case(70, 32, 6, 72, 3, 1, 1, seed=7, **T64)


def test_stride2_transposed_conv_phases_and_its_data_gradient():
    """ConvTranspose2d 3 x 3 stride 2, 3 x 3 -> 7 x 7, 32 -> 32 channels, B = 64: four sub-pixel phases with 4 / 2 / 2 / 1
    taps, each with its own border; then the gradient w.r.t. its input (a stride-2 unpadded conv: every tile clean)."""
    ops = _ops()
    B, Ci, Co, H, R = 64, 32, 32, 3, 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Ci, H, H, generator=g)
    w = torch.randn(Ci, Co, R, R, generator=g) / (Ci * R * R / 4) ** 0.5
    xr = x.clone().requires_grad_(True)
    yr = F.conv_transpose2d(xr, w, stride=2)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    Ho, T = yr.shape[2], R * R
    geom = ops.geom(B, Ho, Ho, Co, H, H, Ci, R, R, 2, 0)          # the conv this transposed conv is the dgrad of
    wf = torch.empty(Co, T, Ci, device="cuda")
    ops.pack_weights(w.cuda().contiguous(), wf, Co, T, Ci, Ci, T, 1, Co * T)
    wd = torch.empty(Ci, T, Co, device="cuda")
    ops.pack_weights(w.cuda().contiguous(), wd, Ci, T, Co, Co, Co * T, 1, T)
    xh, gh = nhwc(x).cuda(), nhwc(gy).cuda()

    def run():
        y = torch.full((B, Ho, Ho, Co), float("nan"), device="cuda")
        ops.conv_bwd_data(geom, xh, wf, y, ops.epilogue())
        dx = torch.full((B, H, H, Ci), float("nan"), device="cuda")
        ops.conv_fwd(geom, gh, wd, dx, ops.epilogue())
        return y, dx

    y, dx = both_loops(run, **T64)
    close(nchw(y), yr, what="convT fwd")
    close(nchw(dx), xr.grad, what="convT dgrad")


def gemm_case(M, C, K, seed, **knobs):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g)
    w = torch.randn(K, C, generator=g) / C ** 0.5
    ref = x @ w.t()
    geom = ops.geom(M, 1, 1, C, 1, 1, K, 1, 1, 1, 0)
    xh, wp = x.reshape(M, 1, 1, C).cuda(), w.reshape(K, 1, C).cuda().contiguous()

    def run():
        y = torch.full((M, 1, 1, K), float("nan"), device="cuda")
        ops.conv_fwd(geom, xh, wp, y, ops.epilogue())
        return (y,)

    (y,) = both_loops(run, **knobs)
    close(y.reshape(M, K), ref, what="1x1 GEMM")


@pytest.mark.parametrize("S", [3, 5])
def test_1x1_gemm_split_k_uneven_k_ranges(S):
    """M = 128, C = 1024 (32 k-tiles), K = 64, split-K forced: 32 tiles over 3 (11 + 11 + 10) or 5 (7 x 4 + 4) slices --
    the last block's k-range ends early, odd and even lengths: the fetches past the end of a range must stage zeros."""
    gemm_case(128, 1024, 64, seed=S, ALI_SPLITK=S, **T64)


def test_1x1_gemm_tail_split_launch():
    """M = 19200 (300 M-tiles of 64), K = 128 (2 n-tiles): 600 blocks of 64 x 64.  By plan_conv's rules: 600
    blocks is not below 2 x 256 CUs, so no split-K search runs and S = 1; 256 < 600 < 1024 with 600 % 256 = 88 left-over
    tiles, and Sr = 2 is the largest power of two with Sr * 88 <= 256 (one piece per CU), so it is a tail split: 512 whole
    tiles, then 88 tiles cut two ways along K.  C = 288 = 9 k-tiles: the two pieces are 5 and 4 k-tiles long (odd and
    even; the second ends early), and each fetches two tiles past its end.  (The same grid as the "tail" case of
    tests/test_gpu_conv_geometry.py.  No knob forces a tail split and a 2-tile GEMM such as M = 128 never takes one:
    that shape runs in the split-K test above.)"""
    gemm_case(300 * 64, 288, 128, seed=5, **T64)


def test_image_major_rows_mix_validity_inside_a_tile():
    """40 x 40 map, 5 x 5 stride 2 pad 2, 32 -> 64 channels, B = 2: 400 output pixels per image, rows ordered
    (image, pixel).  Border tiles mix rows that hit the padding with rows that do not; interior tiles are clean; the
    last tile (800 rows = 12.5 tiles) is ragged."""
    conv_case(2, 32, 40, 64, 5, 2, 2, seed=3, **T64)


def test_multi_job_launch_with_a_clean_and_a_mixed_job():
    ops = _ops()
    g = torch.Generator().manual_seed(17)
    jobs = []
    for (B, C, H, K, R, pad) in [(64, 32, 6, 64, 3, 0), (96, 32, 6, 64, 3, 1)]:     # unpadded: all clean; B = 96 padded: mixed
        x = torch.randn(B, C, H, H, generator=g)
        w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
        ref = F.conv2d(x, w, padding=pad)
        P = ref.shape[2]
        jobs.append((ops.geom(B, H, H, C, P, P, K, R, R, 1, pad), nhwc(x).cuda(), pack_fwd(ops, w), (B, P, P, K), ref))

    def run():
        outs = [torch.full(shape, float("nan"), device="cuda") for (_, _, _, shape, _) in jobs]
        with ops.gemm_batch() as batch:
            for (geom, xh, wp, _, _), y in zip(jobs, outs):
                ops.conv_fwd(geom, xh, wp, y, ops.epilogue())
            assert len(batch.jobs) == 2
        return tuple(outs)

    outs = both_loops(run, **T64)
    for y, (_, _, _, _, ref) in zip(outs, jobs):
        close(nchw(y), ref, what="multi-job conv")


# The clean loop of wgrad_fast_body runs pairs of k-tiles (32 pixels each) while pix0 + 96 <= pix_end: a slab needs more
# than three k-tiles to enter it.  The host (ali_conv_bwd_weight) splits the pixels S = ceil(target / blocks) ways,
# S <= k-tiles / 2, when blocks < target; target = 1024, or ALI_WGRAD_BLOCKS.  Per case: blocks, S, slab, what runs.
W64 = dict(ALI_WBM=64, ALI_WBN=64)
WGRAD_CASES = [
    # B, C, H, K, R, stride, pad, knobs       (4 x 4 stride 2 on 8 x 8: P = 3 unpadded, 4 with pad 1; Mtot = 16 * C rows)
    # the issue's small pair, 36 / 64 pixels = 2 k-tiles: too short for the clean loop, general iterations only
    (4, 32, 8, 64, 4, 2, 0, {}),
    (4, 32, 8, 64, 4, 2, 1, {}),
    # 360 pixels, 8 blocks, target 8 -> S = 1: one slab [0, 360): clean pairs at 0 .. 256 (10 k-tiles), then the general
    # iteration for the k-tile at 320 and the ragged one at 352; every block is clean
    (40, 32, 8, 64, 4, 2, 0, dict(ALI_WGRAD_BLOCKS=8, **W64)),
    # the same, target 16 -> S = 2, 6 k-tiles per slab: [0, 192) runs clean pairs at 0 and 64, [192, 360) at 192 and 256
    # and ends ragged: the pixel count is no multiple of 32 * S
    (40, 32, 8, 64, 4, 2, 0, dict(ALI_WGRAD_BLOCKS=16, **W64)),
    # pad 1, C = 64: one tap per 64-row tile, 16 blocks, target 16 -> S = 1, slab [0, 640) = 20 k-tiles.  The blocks of the
    # interior taps (dh, dw in {0, 1}: taps 5, 6, 9, 10) are clean and run 9 pairs; the 12 border taps miss the map at
    # some output pixel and stay general -- clean and general blocks in one launch
    (40, 64, 8, 64, 4, 2, 1, dict(ALI_WGRAD_BLOCKS=16, **W64)),
    # 333 pixels, 8 blocks, target 24 -> S = 3 (11 k-tiles: 4 per slab = 128 pixels): one clean pair per slab, the last
    # slab [256, 333) has 3 k-tiles and none
    (37, 32, 8, 64, 4, 2, 0, dict(ALI_WGRAD_BLOCKS=24, **W64)),
    # K = 72: two n-tiles, 16 blocks, target 16 -> S = 1, slab [0, 360).  n-tile 0 is clean; n-tile 1 (columns 64 .. 127 of
    # 72) must take the general loop: without its column test its lanes would gather past the pixel's row
    (40, 32, 8, 72, 4, 2, 0, dict(ALI_WGRAD_BLOCKS=16, **W64)),
]


@pytest.mark.parametrize("B,C,H,K,R,stride,pad,knobs", WGRAD_CASES)
def test_weight_gradient_clean_and_mixed_blocks(B, C, H, K, R, stride, pad, knobs):
    ops = _ops()
    g = torch.Generator().manual_seed(B + C + K + pad)
    x = torch.randn(B, C, H, H, generator=g)
    wr = (torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5).requires_grad_(True)
    br = torch.zeros(K, requires_grad=True)
    yr = F.conv2d(x, wr, br, stride=stride, padding=pad)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    P = yr.shape[2]
    geom = ops.geom(B, H, H, C, P, P, K, R, R, stride, pad)
    xh, gh = nhwc(x).cuda(), nhwc(gy).cuda()

    def run():
        dw = torch.full((K, C, R, R), float("nan"), device="cuda")
        db = torch.full((K,), float("nan"), device="cuda")
        ops.conv_bwd_weight(geom, xh, gh, dw, C, K, C * R * R, R * R, 1, db=db)
        return dw, db

    dw, db = both_loops(run, **knobs)
    close(dw, wr.grad, what="wgrad")
    close(db, br.grad, what="db fused into wgrad")


def test_batchnorm_partials_are_untouched():
    """The padded 3 x 3 conv at B = 64 with the BatchNorm statistics in its epilogue (bn_mode 1), and the data gradient
    of an unpadded 3 x 3 conv with the BatchNorm backward reductions in its epilogue (bn_mode 2): partials bit-equal."""
    ops = _ops()
    g = torch.Generator().manual_seed(23)
    B, C, H, K, R = 64, 32, 6, 64, 3
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    ref = F.conv2d(x, w, padding=1)
    geom = ops.geom(B, H, H, C, H, H, K, R, R, 1, 1)
    xh, wp = nhwc(x).cuda(), pack_fwd(ops, w)
    # mode 2: dgrad of a conv K -> K2 (unpadded 3 x 3) that consumes the [B, H, H, K] map
    K2, P2 = 32, H - 2
    w2 = torch.randn(K2, K, R, R, generator=g) / (K * R * R) ** 0.5
    gy2 = torch.randn(B, K2, P2, P2, generator=g)
    geom2 = ops.geom(B, H, H, K, P2, P2, K2, R, R, 1, 0)
    gh2, wd2 = nhwc(gy2).cuda(), pack_dgrad(ops, w2)
    x_in = torch.randn(B, H, H, K, generator=g).cuda()
    mean, invstd = torch.randn(K, generator=g).cuda(), (torch.rand(K, generator=g) + 0.5).cuda()

    def run():
        slots, slots2 = ops.conv_mtiles(geom, 0)[0], ops.conv_mtiles(geom2, 1)[0]   # (under the knobs in force)
        part = torch.zeros(2 * K * slots, device="cuda")
        y = torch.full((B, H, H, K), float("nan"), device="cuda")
        ops.conv_fwd(geom, xh, wp, y, ops.epilogue(bn_fwd=(part, 1, None, slots)))
        part2 = torch.zeros(2 * K * slots2, device="cuda")
        gt = torch.full((B, H, H, K), float("nan"), device="cuda")
        ops.conv_bwd_data(geom2, gh2, wd2, gt, ops.epilogue(bn_bwd=(part2, x_in, mean, invstd, None, None, slots2)))
        return y, part, gt, part2

    y, part, gt, part2 = both_loops(run, **T64)
    close(nchw(y), ref, what="conv fwd with BatchNorm statistics")
    close(nchw(gt), F.conv_transpose2d(gy2, w2), what="dgrad with BatchNorm reductions")
