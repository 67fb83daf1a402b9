"""Shared by tests/test_gpu_flow_kernels.py and tests/test_gpu_attribute_scms.py: the synthetic attribute table, a graph
with parameters that reach every branch of csrc/flow.hip, and the yardstick comparison.

The yardstick: a kernel's error against the fp64 statement is bounded, entry by entry, by MULT times the error of the
same statement run in fp32 on the CPU, plus FLOOR_ULPS fp32 ulps of the reference's magnitude for the entries whose
yardstick error happens to be (almost) zero.  The kernels evaluate rows in fp64 and round once, so their error is about
half an ulp wherever the fp32 statement is worse than that; MULT leaves room for another summation order, not for a
wrong formula, which is off by orders of magnitude."""
import torch

MULT = 4.0
FLOOR_ULPS = 4.0
EPS32 = 2.0 ** -23
NAMES = ("thickness", "intensity", "slant")


def synth_attrs(n, seed=0):
    """a MorphoMNIST-like attribute table [n, 13]: one-hot digit | thickness | intensity (depends on it) | slant"""
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(n, 13)
    a[torch.arange(n), torch.randint(0, 10, (n,), generator=g)] = 1
    t = torch.exp(torch.randn(n, generator=g) * 0.3 + 0.8)
    a[:, 10] = t
    a[:, 11] = 60 + 190 * torch.sigmoid(0.5 * t + torch.randn(n, generator=g))
    a[:, 12] = torch.randn(n, generator=g) * 0.3
    return a


def within_yardstick(name, got, ref64, f32, mult=MULT):
    """assert |got - ref64| <= mult * |f32 - ref64| + FLOOR_ULPS ulp32(|ref64|) entry by entry; prints the worst ratio
    (error beyond the floor) / (yardstick error) first.  Returns that ratio."""
    got, ref64, f32 = (x.detach().double().cpu().reshape(-1) for x in (got, ref64, f32))
    assert got.shape == ref64.shape == f32.shape, (name, got.shape, ref64.shape, f32.shape)
    assert torch.isfinite(got).all() and torch.isfinite(ref64).all(), name
    err, yard = (got - ref64).abs(), (f32 - ref64).abs()
    floor = FLOOR_ULPS * EPS32 * ref64.abs() + 1e-37
    beyond = (err - floor).clamp(min=0)
    ratio = torch.where(beyond > 0, beyond / yard.clamp(min=1e-300), torch.zeros_like(beyond))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"yardstick {name}: worst ratio {worst:.3g}; max error {float(err.max()):.3g} against the fp32 statement's "
          f"{float(yard.max()):.3g}; largest error in ulp32 of the reference "
          f"{float((err / (EPS32 * ref64.abs()).clamp(min=1e-37)).max()):.3g}")
    bad = err > mult * yard + floor
    assert not bad.any(), (name, int(bad.sum()), worst, got[bad][:4], ref64[bad][:4], f32[bad][:4])
    return worst


def flat_theta(graph):
    """theta [75] of a graph (any dtype, any device) in the layout of include/ali_hip.h"""
    bn, caa, sp = graph.trainable()
    parts = [bn.gamma, bn.beta, caa.nn[0].weight, caa.nn[0].bias, caa.nn[2].weight, caa.nn[2].bias,
             sp.unnormalized_widths, sp.unnormalized_heights, sp.unnormalized_derivatives, sp.unnormalized_lambdas]
    return parts, torch.cat([p.detach().reshape(-1) for p in parts])


def branchy_graph(device="cpu", gamma=1.3, seed=11):
    """An MNISTCausalGraph (slant constants s_min = 0, s_max - s_min = 1, so that slant = q) whose parameters reach the
    branches: hidden unit 9 dead, log_scale below -5 at small thickness and above 3 at large thickness; eval mode with
    moving statistics (0.7, 0.2)."""
    import attribute_scms.mnist as am
    torch.manual_seed(seed)
    a = synth_attrs(64, seed)
    a[:, 12] = torch.linspace(0, 1, 64)
    g = am.MNISTCausalGraph(a, device=device)
    bn, caa, sp = g.trainable()
    with torch.no_grad():
        bn.gamma.fill_(gamma)
        bn.beta.fill_(-0.2)
        bn.moving_mean.fill_(0.7)
        bn.moving_variance.fill_(0.2)
        caa.nn[0].weight.fill_(1.0)
        caa.nn[0].bias.copy_(-torch.tensor([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 100.0]))
        caa.nn[2].weight[0].copy_(torch.linspace(-0.3, 0.4, 10))
        caa.nn[2].weight[1].fill_(1.0)
        caa.nn[2].bias.copy_(torch.tensor([0.2, -8.0]))
    for tr in (bn, caa, sp):
        tr.training = False
    return g


def branchy_rows(graph, n, seed=12, extreme=False):
    """An attribute table [n, 13] (float32, CPU) for ``branchy_graph``.  The special rows come first (as many as fit):
    slant on every knot, 16 points inside every bin (both pieces), q = 0 and 1, q outside [-3, 3]; thickness over
    (0.5, 6) so that log_scale is clamped at both ends.  ``extreme``: intensity at i_min and i_max on alternating rows
    (the clamped logit); otherwise strictly inside."""
    g64 = graph.statement(torch.float64)
    _, yk, _, _ = (v.detach() for v in g64.trainable()[2].processed())
    gen = torch.Generator().manual_seed(seed)
    inner = torch.cat([yk[k] + (yk[k + 1] - yk[k]) * (torch.arange(16, dtype=torch.float64) + 0.5) / 16 for k in range(8)])
    special = torch.cat([yk, inner, torch.tensor([0.0, 1.0, -3.5, 3.25, -3.0, 3.0], dtype=torch.float64)]).float()
    q = torch.cat([special, torch.rand(max(n - len(special), 0), generator=gen) * 6 - 3])[:n]
    i_min, i_rng = float(graph.consts[0]), float(graph.consts[1])
    a = torch.zeros(n, 13)
    a[:, 10] = 0.5 + 5.5 * torch.rand(n, generator=gen)
    a[:, 11] = i_min + i_rng * (0.02 + 0.96 * torch.rand(n, generator=gen))
    if extreme:
        a[0::2, 11] = i_min
        a[1::2, 11] = i_min + i_rng
    a[:, 12] = q
    return a


def columns(a):
    """the three continuous columns of an attribute table as strided [N, 1] views, by name"""
    return {"thickness": a[:, 10:11], "intensity": a[:, 11:12], "slant": a[:, 12:13]}


def statement_nll(graph, a, wgt, dtype):
    """the statement in ``dtype`` on the CPU: (lp [N, 3], gtheta [75] = d sum(wgt * lp) / d theta)"""
    g = graph.statement(dtype)
    parts, _ = flat_theta(g)
    lp = g.log_prob({k: v.to(dtype) for k, v in columns(a.cpu()).items()})
    lp = torch.cat([lp[k] for k in NAMES], dim=1)
    grads = torch.autograd.grad((lp * wgt.cpu().to(dtype)).sum(), parts)
    return lp.detach(), torch.cat([x.reshape(-1) for x in grads])
