"""GPU parity of csrc/gan.hip through the C ABI (``ali_hip.ops`` bindings): ``ali_gp_mix``, ``ali_gp_penalty``,
``ali_wgan_critic``.

Reference: the same computation on the CPU in fp64; yardstick: the same computation in CPU fp32.  With e(t) = max|t -
ref64| every device output is held to e(device) <= 4 * e(cpu fp32) and e(device) <= 2e-4 * max|ref64| (the bounds of
test_gpu_conv_geometry.py).  Where the CPU fp32 evaluation happens to be exact (e = 0: single elements, all-zero images)
the yardstick has a floor of one fp32 rounding of the largest reference value, 2^-24 * max|ref64| -- the device result
is an fp32 number and cannot be nearer than that.  ``ali_gp_mix`` with given eps is exact: bit for bit torch's fp32
statement.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 2e-4     # of max|ref64|
YARD = 4.0      # times the deviation of the CPU fp32 evaluation
SHAPES = [(1, 1), (3, 7), (2, 1000), (4, 16384)]


def within(name, got, ref64, f32):
    got, ref64, f32 = got.detach().double().cpu(), ref64.double(), f32.double()
    scale = ref64.abs().max().item()
    e_dev, e_cpu = (got - ref64).abs().max().item(), (f32 - ref64).abs().max().item()
    if scale == 0.0:
        assert e_dev == 0.0, f"{name}: the reference is exactly zero, the device is not ({e_dev:.3e})"
        return
    yard = max(e_cpu, 2.0 ** -24 * scale)
    print(f"{name}: device {e_dev:.3e}, cpu fp32 {e_cpu:.3e} (ratio {e_dev / yard:.2f}), max|ref| {scale:.3e}")
    assert e_dev <= RTOL * scale, f"{name}: max err {e_dev:.3e} vs {RTOL} * {scale:.3e}"
    assert e_dev <= YARD * yard, f"{name}: max err {e_dev:.3e} > {YARD} * {yard:.3e} (CPU fp32)"


# ---------------------------------------------------------------------- ali_gp_mix
@pytest.mark.parametrize("shape", SHAPES)
def test_mix_given_eps_is_torchs_fp32_statement(shape):
    from ali_hip import ops
    B, P = shape
    g = torch.Generator().manual_seed(B * 1000 + P)
    xr, xf = torch.randn(B, P, generator=g), torch.randn(B, P, generator=g)
    eps = torch.rand(B, generator=g)
    want = eps[:, None] * xr + (1 - eps[:, None]) * xf
    got, eps_out = ops.gp_mix(xr.cuda(), xf.cuda(), eps=eps.cuda())
    assert torch.equal(got.cpu(), want) and torch.equal(eps_out.cpu(), eps)
    # 4-d image batches, and rows that start off a 16-byte boundary (a slice one float into a larger buffer)
    if P % 4 == 0 and P >= 16:
        img = ops.gp_mix(xr.cuda().reshape(B, 1, 4, P // 4), xf.cuda().reshape(B, 1, 4, P // 4), eps=eps.cuda())[0]
        assert img.shape == (B, 1, 4, P // 4) and torch.equal(img.cpu().reshape(B, P), want)
        buf = torch.zeros(B * P + 1, device="cuda")
        buf[1:].copy_(xr.reshape(-1))
        off = ops.gp_mix(buf[1:].reshape(B, P), xf.cuda(), eps=eps.cuda())[0]
        assert torch.equal(off.cpu(), want)


def test_mix_drawn_eps():
    from ali_hip import ops, source
    B, P = 4096, 8
    g = torch.Generator().manual_seed(1)
    xr, xf = torch.ones(B, P).cuda(), torch.zeros(B, P).cuda()          # xhat = eps exactly
    ctr = torch.tensor([5], dtype=torch.int64, device="cuda")
    xhat, eps = ops.gp_mix(xr, xf, seed=11, dev_counter=ctr, offset=3)
    e = eps.cpu()
    assert e.shape == (B,) and float(e.min()) >= 0.0 and float(e.max()) < 1.0
    assert torch.equal(xhat.cpu(), e[:, None].expand(B, P))             # constant across an image, the eps written out
    assert torch.equal(e, source.uniform_reference(11, 5, B, offset=3))
    again = ops.gp_mix(xr, xf, seed=11, dev_counter=ctr, offset=3)[1]
    assert torch.equal(again, eps)                                      # same (seed, counter, offset): same bits
    shifted = ops.gp_mix(xr, xf, seed=11, dev_counter=ctr, offset=4)[1]
    assert torch.equal(shifted[:-1], eps[1:]) and not torch.equal(shifted, eps)
    ctr += 1                                                            # a captured graph advances with the counter
    assert not torch.equal(ops.gp_mix(xr, xf, seed=11, dev_counter=ctr, offset=3)[1], eps)
    assert not torch.equal(ops.gp_mix(xr, xf, seed=12, dev_counter=ctr - 1, offset=3)[1], eps)
    assert torch.equal(ops.gp_mix(xr, xf, seed=11, offset=3)[1].cpu(), source.uniform_reference(11, 0, B, offset=3))
    assert abs(float(e.double().mean()) - 0.5) <= 5 / (12 * 4096) ** 0.5
    # random images: the draw only decides eps
    a, b = torch.randn(7, 33, generator=g), torch.randn(7, 33, generator=g)
    xh, e7 = ops.gp_mix(a.cuda(), b.cuda(), seed=2)
    e7 = e7.cpu()
    assert torch.equal(xh.cpu(), e7[:, None] * a + (1 - e7[:, None]) * b)


def test_mix_rejects_bad_arguments():
    from ali_hip import ops
    x = torch.zeros(2, 8, device="cuda")
    with pytest.raises(ValueError):
        ops.gp_mix(x, torch.zeros(2, 4, device="cuda"))
    with pytest.raises(ValueError):
        ops.gp_mix(x, x, eps=torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError):
        ops.gp_mix(x.cpu(), x.cpu())


# ---------------------------------------------------------------------- ali_gp_penalty
def penalty_ref(g0, lam):
    n = g0.flatten(1).norm(dim=1)
    scale = torch.where(n > 0, lam * (2.0 / g0.shape[0]) * (1 - 1 / n), torch.zeros_like(n))
    return torch.stack([((n - 1) ** 2).mean(), n.mean()]), scale[:, None] * g0


@functools.lru_cache(maxsize=None)
def penalty_case(shape, norm, zero_image):
    B, P = shape
    g = torch.Generator().manual_seed(B * 7 + P)
    g0 = torch.randn(B, P, generator=g)
    g0 = g0 / g0.norm(dim=1, keepdim=True) * norm * (1 + 0.1 * torch.arange(B).float()[:, None])
    if zero_image:
        g0[B // 2] = 0
    return g0, penalty_ref(g0.double(), 10.0), penalty_ref(g0, 10.0)


@pytest.mark.parametrize("zero_image", [False, True], ids=["", "zero_image"])
@pytest.mark.parametrize("norm", [0.1, 1.0, 30.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_penalty_against_fp64(shape, norm, zero_image):
    from ali_hip import ops
    g0, (out64, v64), (out32, v32) = penalty_case(shape, norm, zero_image)
    gd = g0.cuda()
    out2, v = ops.gp_penalty(gd, 10.0)
    within(f"{shape} n={norm} penalty", out2[0:1], out64[0:1], out32[0:1])
    within(f"{shape} n={norm} mean norm", out2[1:2], out64[1:2], out32[1:2])
    if v64.abs().max() > 0:
        within(f"{shape} n={norm} v", v, v64, v32)
    if zero_image:
        assert float(v[shape[0] // 2].abs().max()) == 0.0 and torch.isfinite(v).all()
    out2b, vb = ops.gp_penalty(gd, 10.0)                        # fixed reduction order: the same bits
    assert torch.equal(out2b, out2) and torch.equal(vb, v)
    alias = gd.clone()
    out2c, vc = ops.gp_penalty(alias, 10.0, out=alias)         # v aliased to g0
    assert vc.data_ptr() == alias.data_ptr() and torch.equal(out2c, out2) and torch.equal(vc, v)
    out2d, none = ops.gp_penalty(gd, 10.0, want_v=False)
    assert none is None and torch.equal(out2d, out2) and torch.equal(gd.cpu(), g0)


def test_penalty_unaligned_rows():
    """rows one float off a 16-byte boundary with P % 4 == 0: the element-wise path"""
    from ali_hip import ops
    g0, (out64, v64), (out32, v32) = penalty_case((2, 1000), 1.0, False)
    buf = torch.zeros(2001, device="cuda")
    buf[1:].copy_(g0.reshape(-1))
    out2, v = ops.gp_penalty(buf[1:].reshape(2, 1000), 10.0)
    within("unaligned penalty", out2[0:1], out64[0:1], out32[0:1])
    within("unaligned v", v, v64, v32)


# ---------------------------------------------------------------------- ali_wgan_critic
@pytest.mark.parametrize("B", [1, 3, 64])
def test_critic_against_fp64(B):
    from ali_hip import ops
    g = torch.Generator().manual_seed(B)
    df, dr = torch.randn(B, generator=g) * 3 + 1, torch.randn(B, generator=g) * 3 - 2

    def ref(f, r):
        mf = f.mean() if f is not None else torch.zeros((), dtype=(r if f is None else f).dtype)
        mr = r.mean() if r is not None else torch.zeros((), dtype=(f if r is None else r).dtype)
        return torch.stack([mf - mr, mf, mr])

    for name, f, r, gs in (("both", df, dr, 1.0), ("no real", df, None, -1.0), ("no fake", None, dr, 2.5)):
        out3, gf, gr = ops.wgan_critic(None if f is None else f.cuda(), None if r is None else r.cuda(), gs)
        r64 = ref(None if f is None else f.double(), None if r is None else r.double())
        r32 = ref(f, r)
        for i, what in enumerate(("loss", "mean fake", "mean real")):
            if r64[i] != 0:
                within(f"B={B} {name} {what}", out3[i:i + 1], r64[i:i + 1], r32[i:i + 1])
            else:
                assert float(out3[i]) == 0.0
        assert (gf is None) == (f is None) and (gr is None) == (r is None)
        want = torch.full((B,), gs / B, dtype=torch.float64)
        if gf is not None:
            within(f"B={B} {name} g_fake", gf, want, want.float())
        if gr is not None:
            within(f"B={B} {name} g_real", gr, -want, -want.float())
    out3, gf, gr = ops.wgan_critic(df.cuda(), dr.cuda(), want_grad=False)
    assert gf is None and gr is None
    # gradients written into slices of a caller's buffer
    buf = torch.ones(3 * B, device="cuda")
    ops.wgan_critic(df.cuda(), dr.cuda(), 1.0, g_fake=buf[:B], g_real=buf[B:2 * B])
    assert torch.equal(buf[2 * B:].cpu(), torch.ones(B)) and float(buf[0]) == pytest.approx(1.0 / B, rel=1e-6)
    assert float(buf[B]) == pytest.approx(-1.0 / B, rel=1e-6)
    with pytest.raises(ValueError):
        ops.wgan_critic(None, None)
