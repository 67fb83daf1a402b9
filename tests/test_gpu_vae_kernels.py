"""csrc/vae.hip: ali_vae_latent_fwd, ali_vae_loglik, ali_vae_latent_bwd.

Reference: the closed form under torch autograd on the CPU in fp64; yardstick: the same in CPU fp32.  With
e(t) = max|t - ref64| every result is held to the two bounds of test_gpu_conv_geometry.py,
    e(device) <= YARD * e(cpu fp32)     and     e(device) <= RTOL * max|ref64|,
both imported from there.  Shapes: a pruned cross of B in {1, 5, 64, 257}, S in {1, 2, 5}, L in {1, 3, 64, 65, 512},
P in {1, 3, 63, 64, 65, 784, 16384} (P = 16384 with B <= 5 only); S*B = 1285 rows exceed the log-likelihood's 1024
blocks.  Variants: log_var rows at +-10, mean scaled by 1e3, x == xhat, k = 0.5 / 1.0, kl_weight 0 / 1 / 10, a decoder
row stride ld > L whose other columns hold sentinels.  Also: identical bits on a second run, the workspace's reserved
head back at zero, in-kernel draws against ``ali_normal_fill`` and ``ali_hip.source.normal_reference``."""
import math

import numpy as np
import pytest
import torch

from test_gpu_conv_geometry import RTOL, YARD

gpu = pytest.mark.gpu

LATENT = [(1, 1, 1), (5, 2, 3), (64, 1, 64), (5, 5, 65), (257, 2, 65), (64, 2, 512), (1, 5, 512), (257, 1, 3)]
LOGLIK = [(1, 1, 1), (5, 2, 3), (64, 1, 63), (5, 5, 64), (257, 2, 65), (64, 2, 784), (5, 1, 16384), (1, 5, 16384),
          (257, 5, 3), (64, 5, 65)]
VARIANTS = ("normal", "lv10", "mean1e3")
KLW = {"normal": 10.0, "lv10": 1.0, "mean1e3": 0.0}


def _check(label, got, ref, f32):
    got = got.detach().double().cpu()
    scale = ref.abs().max().item()
    e_dev = (got - ref).abs().max().item()
    e_cpu = (f32.double() - ref).abs().max().item()
    print(f"VAE {label} e_dev={e_dev:.3e} e_cpu={e_cpu:.3e} scale={scale:.3e}")
    assert e_dev == e_dev, f"{label}: NaN"
    assert e_dev <= RTOL * scale, f"{label}: max err {e_dev:.3e} vs {RTOL} * {scale:.3e}"
    assert e_dev <= YARD * e_cpu, f"{label}: max err {e_dev:.3e} > {YARD} * {e_cpu:.3e} (CPU fp32)"


def _latent_inputs(B, S, L, variant):
    g = torch.Generator().manual_seed(100000 * B + 1000 * S + L)
    mean, lv = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    eps, gin = torch.randn(S, B, L, generator=g), torch.randn(S * B, L + 5, generator=g)
    if variant == "lv10":
        lv[0::2], lv[1::2] = 10.0, -10.0
    elif variant == "mean1e3":
        mean = mean * 1e3
    return mean, lv, eps, gin


_LAT = {}


def latent_reference(B, S, L, variant, k):
    """per dtype: z, kl_sum, and the gradients of sum(gin[:, :L] * z) + kl_weight * kl_sum / B w.r.t. mean, log_var"""
    key = (B, S, L, variant, k)
    if key not in _LAT:
        mean, lv, eps, gin = _latent_inputs(B, S, L, variant)
        out = {}
        for name, dt in (("ref", torch.float64), ("f32", torch.float32)):
            m, v = mean.to(dt).requires_grad_(True), lv.to(dt).requires_grad_(True)
            z = (m + eps.to(dt) * torch.exp(k * v)).reshape(S * B, L)
            kl = (0.5 * (torch.exp(v) + m * m - 1 - v)).sum()
            f = (gin[:, :L].to(dt) * z).sum() + KLW[variant] * kl / B
            gm, gv = torch.autograd.grad(f, (m, v))
            gc = gin[:, L:].to(dt).reshape(S, B, 5).sum(0)
            out[name] = (z.detach(), kl.detach(), gm, gv, gc)
        _LAT[key] = (mean, lv, eps, gin, out)
    return _LAT[key]


@gpu
@pytest.mark.parametrize("B,S,L", LATENT, ids=[f"B{b}-S{s}-L{l}" for b, s, l in LATENT])
def test_latent_forward_and_backward(B, S, L):
    from ali_hip import ops
    for variant in VARIANTS:
        for k in (0.5, 1.0):
            mean, lv, eps, gin, out = latent_reference(B, S, L, variant, k)
            label = f"B={B} S={S} L={L} {variant} k={k}"
            head = torch.cat([mean, lv], dim=1).cuda()                    # one [B, 2L] head output serves both
            md, vd = head[:, :L], head[:, L:]
            ld = L + 5
            rows = torch.full((S * B, ld), 7.0, device="cuda")           # sentinels behind the latent columns
            kl, _ = ops.vae_latent_fwd(md, vd, S, rows, k=k, eps=eps.cuda())
            _check(label + " z", rows[:, :L], out["ref"][0], out["f32"][0])
            _check(label + " kl", kl[0], out["ref"][1], out["f32"][1])
            assert bool((rows[:, L:] == 7.0).all()), label + ": the conditioning columns were touched"
            rows2 = torch.full((S * B, ld), 7.0, device="cuda")
            kl2, _ = ops.vae_latent_fwd(md, vd, S, rows2, k=k, eps=eps.cuda())
            assert torch.equal(rows, rows2) and torch.equal(kl, kl2), label
            ghead = torch.full((B, 2 * L + 1), 7.0, device="cuda")
            gcond = ops.vae_latent_bwd(gin.cuda(), eps.cuda(), md, vd, S, ghead[:, :L], ghead[:, L:2 * L], k,
                                       KLW[variant], None, ncond=5)
            _check(label + " gmean", ghead[:, :L], out["ref"][2], out["f32"][2])
            _check(label + " glog_var", ghead[:, L:2 * L], out["ref"][3], out["f32"][3])
            _check(label + " gcond", gcond, out["ref"][4], out["f32"][4])
            assert bool((ghead[:, 2 * L] == 7.0).all()), label
            # the KL terms times a device scalar: linear in it
            ghalf = torch.empty(B, 2 * L, device="cuda")
            ops.vae_latent_bwd(gin.cuda() * 0, eps.cuda(), md, vd, S, ghalf[:, :L], ghalf[:, L:], k, KLW[variant],
                               torch.full((1,), 0.5, device="cuda"))
            gfull = torch.empty(B, 2 * L, device="cuda")
            ops.vae_latent_bwd(gin.cuda() * 0, eps.cuda(), md, vd, S, gfull[:, :L], gfull[:, L:], k, KLW[variant])
            assert torch.equal(ghalf * 2, gfull), label
    assert int(ops.workspace(torch.device("cuda"))[:4096].count_nonzero()) == 0       # the arrival counter is at zero


_LL = {}


def loglik_reference(B, S, P, klw):
    key = (B, S, P, klw)
    if key not in _LL:
        g = torch.Generator().manual_seed(7 + 100000 * B + 1000 * S + P)
        x, xhat = torch.rand(B, P, generator=g) * 2 - 1, torch.tanh(torch.randn(S * B, P, generator=g))
        kl_sum = torch.rand(1, generator=g) * 50 * B
        out = {}
        for name, dt in (("ref", torch.float64), ("f32", torch.float32)):
            h = xhat.to(dt).requires_grad_(True)
            d = (x.to(dt).repeat(S, 1) - h).square().sum(1)
            lp = (-0.5 * d * math.exp(5.0) + 0.5 * P * 5.0 - 0.5 * P * math.log(2 * math.pi)).reshape(S, B).mean(0).mean()
            klm = kl_sum.to(dt)[0] / B
            loss = -(lp - klw * klm)
            (gh,) = torch.autograd.grad(loss * 0.5, h)                   # gscale = 0.5
            out[name] = (torch.stack([lp.detach(), loss.detach(), klm]), gh)
        _LL[key] = (x, xhat, kl_sum, out)
    return _LL[key]


@gpu
@pytest.mark.parametrize("B,S,P", LOGLIK, ids=[f"B{b}-S{s}-P{p}" for b, s, p in LOGLIK])
def test_log_likelihood_loss_and_gradient(B, S, P):
    from ali_hip import ops
    for klw in (0.0, 1.0, 10.0):
        x, xhat, kl_sum, out = loglik_reference(B, S, P, klw)
        label = f"B={B} S={S} P={P} klw={klw}"
        xd, hd, kd = x.cuda(), xhat.cuda(), kl_sum.cuda()
        out3, g = ops.vae_loglik(xd, hd, S, -5.0, kd, klw, gscale=0.5)
        _check(label + " out3", out3, out["ref"][0], out["f32"][0])
        _check(label + " gxhat", g, out["ref"][1], out["f32"][1])
        again = ops.vae_loglik(xd, hd, S, -5.0, kd, klw, gscale=0.5)
        assert torch.equal(out3, again[0]) and torch.equal(g, again[1]), label
        bare, none = ops.vae_loglik(xd, hd, S, -5.0, kd, klw, want_grad=False)
        assert none is None and torch.equal(bare, out3), label
    # unaligned rows (a view one float into a buffer): the scalar path gives the same values
    buf = torch.zeros(S * B * P + 1, device="cuda")
    buf[1:] = hd.reshape(-1)
    o2, g2 = ops.vae_loglik(xd, buf[1:].view(S * B, P), S, -5.0, kd, klw, gscale=0.5)
    _check(label + " unaligned out3", o2, out["ref"][0], out["f32"][0])
    assert torch.equal(g2, g)
    # x == xhat: exactly zero gradient, the loss is the constants
    o0, g0 = ops.vae_loglik(xd, xd.repeat(S, 1), S, -5.0, None, 10.0)
    const = np.float32(0.5 * P * 5.0 - 0.5 * P * math.log(2 * math.pi))
    assert int(g0.count_nonzero()) == 0
    assert o0[0].item() == const and o0[1].item() == -const and o0[2].item() == 0.0
    assert int(ops.workspace(torch.device("cuda"))[:4096].count_nonzero()) == 0


@gpu
@pytest.mark.parametrize("int_onehot", [False, True])
def test_conditioning_columns_in_the_same_launch(int_onehot):
    """[z | onehot_j @ table_j | cont | 0] for all S*B rows, the row of ``ali_g_input`` repeated per draw"""
    from ali_hip import ops
    B, S, L = 5, 2, 64
    g = torch.Generator().manual_seed(3)
    mean, lv, eps = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g), torch.randn(S, B, L, generator=g)
    tabs = [torch.randn(n, 256, generator=g) for n in (10, 3)]
    hots = [torch.eye(n)[torch.randint(0, n, (B,), generator=g)] for n in (10, 3)]
    cont = torch.randn(B, 3, generator=g)
    n_log = L + 512 + 3
    ld = n_log + (-n_log) % 32
    rows = torch.full((S * B, ld), 7.0, device="cuda")
    dh = [(h.int() if int_onehot else h).cuda() for h in hots]
    ops.vae_latent_fwd(mean.cuda(), lv.cuda(), S, rows, eps=eps.cuda(), onehots=dh, tables=[t.cuda() for t in tabs],
                       cont=cont.cuda(), want_kl=False)
    want = torch.cat([h @ t for h, t in zip(hots, tabs)] + [cont, torch.zeros(B, ld - n_log)], dim=1).repeat(S, 1)
    assert torch.equal(rows[:, L:].cpu(), want)
    zs = torch.empty(B, ld, device="cuda")
    ref_rows = ops.g_input(zs[:, :L].contiguous(), [h.cuda() for h in hots], [t.cuda() for t in tabs], cont.cuda(), ld)
    assert torch.equal(rows[:B, L:], ref_rows[:, L:])
    soft = [torch.rand(B, n, generator=g) for n in (10, 3)]                       # soft attributes: a true sum
    ops.vae_latent_fwd(mean.cuda(), lv.cuda(), S, rows, eps=eps.cuda(), onehots=[h.cuda() for h in soft],
                       tables=[t.cuda() for t in tabs], cont=cont.cuda(), want_kl=False)
    ref_rows = ops.g_input(zs[:, :L].contiguous(), [h.cuda() for h in soft], [t.cuda() for t in tabs], cont.cuda(), ld)
    assert torch.equal(rows[B:, L:], ref_rows[:, L:])


@gpu
@pytest.mark.parametrize("B,S,L,offset", [(5, 2, 65, 0), (64, 1, 512, 3), (1, 5, 3, 1001)])
def test_draws_made_in_the_kernel_are_the_latent_stream(B, S, L, offset):
    from ali_hip import ops
    from ali_hip.source import latent_bits, normal_reference
    seed, counter = 0x5EED, 7
    ctr = torch.full((1,), counter, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(B + S + L)
    mean, lv = torch.randn(B, L, generator=g).cuda(), torch.randn(B, L, generator=g).cuda()
    rows = torch.empty(S * B, L, device="cuda")
    kl, eps = ops.vae_latent_fwd(mean, lv, S, rows, seed=seed, dev_counter=ctr, offset=offset, want_eps=True)
    n = S * B * L
    fill = ops.normal_fill(seed, torch.empty(n, device="cuda"), dev_counter=ctr, offset=offset)
    assert torch.equal(eps.reshape(-1), fill)                       # the same stream, bit for bit
    ref = normal_reference(seed, counter, n, offset).numpy()
    k1, k2, odd = latent_bits(seed, counter, n, offset)
    u1, u2 = k1.astype(np.float32) * np.float32(2.0 ** -24), k2.astype(np.float32) * np.float32(2.0 ** -24)
    f32 = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.where(odd, np.sin(np.float32(2.0 * np.pi) * u2),
                                                            np.cos(np.float32(2.0 * np.pi) * u2))
    dev, bound = np.abs(eps.reshape(-1).cpu().numpy() - ref).max(), 4 * np.abs(f32.astype(np.float64) - ref).max()
    print(f"VAE draws B={B} S={S} L={L}: device max |dev| {dev:.3e}, numpy-f32 max |dev| {bound / 4:.3e}")
    assert dev <= bound, (dev, bound)
    given = torch.empty(S * B, L, device="cuda")                    # given the same draws: the same rows and KL
    kl2, _ = ops.vae_latent_fwd(mean, lv, S, given, eps=eps)
    assert torch.equal(given, rows) and torch.equal(kl, kl2)
