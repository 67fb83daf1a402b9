"""The kernels of csrc/flow.hip through ``ali_hip.ops`` against the fp64 statement of ``attribute_scms`` on the CPU.

Tolerances are the yardstick of tests/flow_cases.py: entry by entry, MULT times the error of the fp32
statement on the CPU plus a floor of FLOOR_ULPS fp32 ulps.  Each test prints its measured worst ratio before it asserts.
The rows reach every branch (``flow_cases.branchy_graph`` / ``branchy_rows``); N = 16385 fills the launcher's largest
grid (64 blocks of 256 threads) so that the fold of the last block adds 64 partials per accumulator."""
import functools

import pytest
import torch

import flow_cases as fc
from flow_cases import NAMES, within_yardstick

pytestmark = pytest.mark.gpu
SIZES = [2, 65, 257, 64 * 256 + 1]


def _ops():
    from ali_hip import ops
    return ops


@functools.lru_cache(maxsize=None)
def case(n, gamma=1.3, extreme=False):
    """(graph on the CPU, attribute table, wgt, fp64 and fp32 statement results), computed once per case"""
    g = fc.branchy_graph("cpu", gamma=gamma)
    a = fc.branchy_rows(g, n, extreme=extreme)
    wgt = torch.randn(n, 3, generator=torch.Generator().manual_seed(n))
    ref = fc.statement_nll(g, a, wgt, torch.float64)
    f32 = fc.statement_nll(g, a, wgt, torch.float32)
    mean = fc.statement_nll(g, a, torch.full((n, 3), -1.0 / n), torch.float64)[1], \
        fc.statement_nll(g, a, torch.full((n, 3), -1.0 / n), torch.float32)[1]
    return g, a, wgt, ref, f32, mean


def _device_args(g, a):
    theta = fc.flat_theta(g)[1].float().cuda()
    stats = torch.tensor([0.7, 0.2], device="cuda")
    return fc.columns(a.cuda()), theta, g.consts.float().cuda(), stats


def test_rows_reach_every_branch():
    g, a, *_ = case(257)
    g64 = g.statement(torch.float64)
    bn, caa, sp = g64.trainable()
    xk, yk, _, lam = (v.detach() for v in sp.processed())
    q = a[:, 12].double()
    inside = (q >= -3) & (q <= 3)
    assert (~inside).any() and (q == 0).any() and (q == 1).any() and (q == 3).any() and (q == -3).any()
    u = sp.inv(q.reshape(-1, 1)).flatten().detach()
    k = (q.unsqueeze(-1) >= yk[1:-1]).sum(-1)
    left = (u - xk[k]) / (xk[k + 1] - xk[k]) <= lam[k]
    assert {(int(b), bool(s)) for b, s, i in zip(k, left, inside) if i} == {(b, s) for b in range(8) for s in (0, 1)}
    assert all((q == yk[j].float().double()).any() for j in range(9))                      # on every knot (fp32)
    raw = caa.nn(a[:, 10:11].double())[:, 1]
    assert (raw > 3).any() and (raw < -5).any() and ((raw > -5) & (raw < 3)).any()
    h = torch.relu(caa.nn[0](a[:, 10:11].double()))
    assert (h[:, 9] == 0).all() and (h[:, 0] > 0).all() and (h[:, 8] == 0).any() and (h[:, 8] > 0).any()


@pytest.mark.parametrize("n", SIZES)
def test_flow_nll_against_the_statement(n):
    ops = _ops()
    g, a, wgt, (lp64, g64), (lp32, g32), (gm64, gm32) = case(n)
    cols, theta, cst, stats = _device_args(g, a)
    assert cols["thickness"].stride(0) == 13                                   # strided views of the [N][13] table
    t, i, s = (cols[k] for k in NAMES)
    lp, out4, gth = ops.flow_nll(t, i, s, theta, cst, stats, wgt=wgt.cuda(), want_grad=True)
    within_yardstick(f"lp N={n}", lp, lp64, lp32)
    within_yardstick(f"gtheta (wgt array) N={n}", gth, g64, g32)
    means64, means32 = lp64.mean(0), lp32.mean(0)
    within_yardstick(f"out4 N={n}", out4, torch.cat([-lp64.sum(1).mean().reshape(1), means64]),
                     torch.cat([-lp32.sum(1).mean().reshape(1), means32]))
    # wgt = NULL: the constant gscale / N; lp not asked for
    lp_none, out4b, gthb = ops.flow_nll(t, i, s, theta, cst, stats, gscale=-1.0, want_lp=False, want_grad=True)
    assert lp_none is None and torch.equal(out4b, out4)
    within_yardstick(f"gtheta (wgt NULL) N={n}", gthb, gm64, gm32)
    # the same bits on every run, and the arrival counter is back at zero (the next launch depends on it)
    lp2, out42, gth2 = ops.flow_nll(t, i, s, theta, cst, stats, wgt=wgt.cuda(), want_grad=True)
    assert torch.equal(lp2, lp) and torch.equal(out42, out4) and torch.equal(gth2, gth)
    # contiguous columns give what the strided views give
    lp3, _, gth3 = ops.flow_nll(t.contiguous(), i.contiguous().flatten(), s.contiguous(), theta, cst, stats,
                                wgt=wgt.cuda(), want_grad=True)
    assert torch.equal(lp3, lp) and torch.equal(gth3, gth)


def test_flow_nll_gated_gamma():
    ops = _ops()
    for gamma in (-0.5, 0.0):
        g, a, wgt, (lp64, g64), (lp32, g32), _ = case(257, gamma=gamma)
        cols, theta, cst, stats = _device_args(g, a)
        lp, _, gth = ops.flow_nll(*(cols[k] for k in NAMES), theta, cst, stats, wgt=wgt.cuda(), want_grad=True)
        assert g64[0] == 0 and gth[0] == 0                                      # relu'(gamma <= 0) = 0
        assert gth[21] == 0 and gth[11] == 0 and gth[31] == 0 and gth[41] == 0  # the dead unit: b1, W1, both W2 rows
        within_yardstick(f"lp gamma={gamma}", lp, lp64, lp32)
        within_yardstick(f"gtheta gamma={gamma}", gth, g64, g32)


def test_flow_nll_extreme_logits_relative():
    """i = i_min and i = i_max on every row: the clamped logit, log FLT_MIN = -87.3 and log(1 / FLT_EPSILON) = 15.9.
    A case of its own, compared relatively (these log-densities reach 1e8 in magnitude where log_scale = -5): a row
    is an fp64 evaluation rounded once, so the bound is the floor alone."""
    ops = _ops()
    g, a, wgt, (lp64, g64), (lp32, g32), _ = case(256, extreme=True)
    cols, theta, cst, stats = _device_args(g, a)
    lp, _, gth = ops.flow_nll(*(cols[k] for k in NAMES), theta, cst, stats, wgt=wgt.cuda(), want_grad=True)
    assert lp64[:, 1].abs().max() > 1e6
    rel = ((lp.double().cpu() - lp64).abs() / lp64.abs()).max().item()
    rel32 = ((lp32.double() - lp64).abs() / lp64.abs()).max().item()
    relg = ((gth.double().cpu() - g64).abs() / g64.abs().clamp(min=1e-30)).max().item()
    print(f"extreme rows: lp relative error {rel:.3g} (fp32 statement {rel32:.3g}), gtheta relative error {relg:.3g}")
    assert rel <= fc.FLOOR_ULPS * fc.EPS32
    within_yardstick("gtheta extreme", gth, g64, g32)


@pytest.mark.parametrize("n", SIZES)
def test_flow_stats(n):
    ops = _ops()
    a = case(n)[1]
    t = a.cuda()[:, 10:11]
    x64 = a[:, 10].double().log()
    ref = torch.stack([x64.mean(), x64.var(unbiased=True)])
    x32 = a[:, 10].log()
    f32 = torch.stack([x32.mean(), x32.var(unbiased=True)])
    out = ops.flow_stats(t)
    within_yardstick(f"stats N={n}", out, ref, f32)
    moving = torch.tensor([0.7, 0.2], device="cuda")
    out2 = ops.flow_stats(t, moving=moving, momentum=0.1)
    assert torch.equal(out2, out)                                               # the same bits on every run
    within_yardstick(f"moving N={n}", moving, 0.9 * torch.tensor([0.7, 0.2]).double() + 0.1 * ref,
                     0.9 * torch.tensor([0.7, 0.2]) + 0.1 * f32)
    assert torch.equal(ops.flow_stats(t.contiguous()), out)


def test_flow_stats_refuses_one_row_with_moving():
    ops = _ops()
    t = torch.tensor([1.5], device="cuda")
    with pytest.raises(RuntimeError, match="N >= 2"):
        ops.flow_stats(t, moving=torch.tensor([0.0, 1.0], device="cuda"))
    assert torch.isnan(ops.flow_stats(t)[1])                                    # torch's unbiased variance of one row


def _noise_rows(n):
    z = torch.randn(n, 3, generator=torch.Generator().manual_seed(n + 1)) * 1.5
    z[: min(n, 8), 2] = torch.tensor([-3.0, 3.0, -3.5, 4.0, 0.0, 2.999, -2.999, 3.0001])[: min(n, 8)]   # the identity branch
    return z


def _statement_map(g, rows, forward, dtype):
    """each column through its flow on the CPU; the intensity under the thickness VALUE of the row"""
    gs = g.statement(dtype)
    r = rows.to(dtype)
    if forward:
        t = gs.get_module("thickness").generate(r[:, 0:1])
        i = gs.get_module("intensity").condition(t).generate(r[:, 1:2], t)
        s = gs.get_module("slant").generate(r[:, 2:3])
        return torch.cat([t, i, s], 1).detach()
    noise = gs.recover_noise(dict(zip(NAMES, (r[:, j:j + 1] for j in range(3)))))
    return torch.cat([noise[k] for k in NAMES], 1).detach()


@pytest.mark.parametrize("n", [2, 65, 257])
def test_flow_map_forward_and_inverse(n):
    ops = _ops()
    g, a, *_ = case(n)
    _, theta, cst, stats = _device_args(g, a)
    z = _noise_rows(n)
    fwd, _ = ops.flow_map(z.cuda(), theta, cst, stats, stats, modes=(ops.FLOW_FORWARD,) * 3)
    within_yardstick(f"forward N={n}", fwd, _statement_map(g, z, True, torch.float64), _statement_map(g, z, True, torch.float32))
    vals = torch.stack([a[:, 10], a[:, 11], a[:, 12]], 1).contiguous()
    inv, _ = ops.flow_map(vals.cuda(), theta, cst, stats, stats, modes=(ops.FLOW_INVERSE,) * 3)
    within_yardstick(f"inverse N={n}", inv, _statement_map(g, vals, False, torch.float64),
                     _statement_map(g, vals, False, torch.float32))
    # per column: one column forward, the others passed through; intensity under the INPUT thickness then
    mixed = torch.stack([a[:, 10], z[:, 1], a[:, 12]], 1).contiguous()
    one, _ = ops.flow_map(mixed.cuda(), theta, cst, stats, stats, modes=(ops.FLOW_SKIP, ops.FLOW_FORWARD, ops.FLOW_SKIP))
    assert torch.equal(one[:, 0].cpu(), mixed[:, 0]) and torch.equal(one[:, 2].cpu(), mixed[:, 2])
    g64, g32 = g.statement(torch.float64), g.statement(torch.float32)

    def held(gs, dt):
        t = mixed[:, 0:1].to(dt)
        return gs.get_module("intensity").condition(t).generate(mixed[:, 1:2].to(dt), t).detach()
    within_yardstick(f"intensity under held thickness N={n}", one[:, 1], held(g64, torch.float64), held(g32, torch.float32))
    # forward then inverse, in place
    back, _ = ops.flow_map(fwd, theta, cst, stats, stats, modes=(ops.FLOW_INVERSE,) * 3, out=fwd)
    assert back is fwd


@pytest.mark.parametrize("mask", range(8))
def test_flow_map_counterfactual(mask):
    ops = _ops()
    n = 100
    g, a, *_ = case(n)
    _, theta, cst, stats = _device_args(g, a)
    obs = torch.stack([a[:, 10], a[:, 11], a[:, 12]], 1).contiguous()
    gen = torch.Generator().manual_seed(mask)
    val = torch.stack([0.5 + 5 * torch.rand(n, generator=gen), a[:, 11].flip(0), torch.rand(n, generator=gen)], 1)
    out, noise = ops.flow_map(obs.cuda(), theta, cst, stats, stats, cf_mask=mask, val=val.cuda() if mask else None,
                              want_noise=True)

    def statement(dt):
        gs = g.statement(dt)
        o = dict(zip(NAMES, (obs[:, j:j + 1].to(dt) for j in range(3))))
        cf = gs.sample_cf(o, {k: val[:, j:j + 1].to(dt) for j, k in enumerate(NAMES) if mask >> j & 1})
        return torch.cat([cf[k] for k in NAMES], 1).detach(), torch.cat([gs.recover_noise(o)[k] for k in NAMES], 1).detach()
    (cf64, n64), (cf32, n32) = statement(torch.float64), statement(torch.float32)
    within_yardstick(f"counterfactual mask={mask}", out, cf64, cf32)
    within_yardstick(f"abducted noise mask={mask}", noise, n64, n32)
    for j in range(3):
        if mask >> j & 1:
            assert torch.equal(out[:, j].cpu(), val[:, j])
    if mask == 0:
        # the observation comes back within the round trip's error: rows are evaluated in fp64, where the round trip
        # is exact to ~4e-14 (1e-12 allowed: an observation of exactly 0 need not come back as 0), and rounded once
        err = (out.cpu().double() - obs.double()).abs()
        print(f"empty intervention: the observation returns within {(err / (fc.EPS32 * obs.abs().double() + 1e-12)).max().item():.3g} "
              f"of one ulp + 1e-12")
        assert (err <= fc.EPS32 * obs.abs().double() + 1e-12).all()


@pytest.mark.parametrize("C", [1, 2, 6, 65])
def test_gumbel_posterior(C):
    ops = _ops()
    from attribute_scms.causal_module import gumbel_posterior
    from ali_hip import source
    n = 300
    gen = torch.Generator().manual_seed(C)
    logits = torch.randn(n, C, generator=gen) * 3
    y = torch.randint(0, C, (n,), generator=gen)
    g = -torch.log(-torch.log(torch.rand(n, C, generator=gen).clamp(1e-6, 1 - 1e-6)))
    noise, _ = ops.gumbel_posterior(logits.cuda(), y.cuda(), g=g.cuda())
    within_yardstick(f"gumbel C={C}", noise, gumbel_posterior(logits.double(), y, g.double()), gumbel_posterior(logits, y, g))
    assert torch.equal((logits.cuda() + noise).argmax(1).cpu(), y)
    # drawn on the device: the recipe of ali_hip.source, and again the observation
    noise_d, g_d = ops.gumbel_posterior(logits.cuda(), y.cuda(), seed=5, offset=7, want_g=True)
    ref = source.gumbel_reference(5, 0, n * C, offset=7).reshape(n, C)
    assert (g_d.double().cpu() - ref).abs().max() <= 2 * fc.EPS32 * ref.abs().max()
    assert torch.equal((logits.cuda() + noise_d).argmax(1).cpu(), y)
    within_yardstick(f"gumbel drawn C={C}", noise_d, gumbel_posterior(logits.double(), y, g_d.double().cpu()),
                     gumbel_posterior(logits, y, g_d.cpu()))
    # disjoint offset ranges tile a longer draw; a device counter keys another stream
    half = n // 2
    _, ga = ops.gumbel_posterior(logits[:half].cuda(), y[:half].cuda(), seed=5, offset=7, want_g=True)
    _, gb = ops.gumbel_posterior(logits[half:].cuda(), y[half:].cuda(), seed=5, offset=7 + half * C, want_g=True)
    assert torch.equal(torch.cat([ga, gb]), g_d)
    ctr = torch.tensor([3], dtype=torch.int64, device="cuda")
    _, gc = ops.gumbel_posterior(logits.cuda(), y.cuda(), seed=5, dev_counter=ctr, offset=7, want_g=True)
    assert not torch.equal(gc, g_d)
    assert (gc.double().cpu() - source.gumbel_reference(5, 3, n * C, offset=7).reshape(n, C)).abs().max() <= 1e-5
    again, _ = ops.gumbel_posterior(logits.cuda(), y.cuda(), seed=5, offset=7)
    assert torch.equal(again, noise_d)


def test_bad_arguments_are_refused_before_any_launch():
    ops = _ops()
    g, a, *_ = case(2)
    cols, theta, cst, stats = _device_args(g, a)
    rows = torch.ones(2, 3, device="cuda")
    with pytest.raises(RuntimeError, match="cf_mask"):
        ops.flow_map(rows, theta, cst, stats, stats, cf_mask=3)                 # intervened columns without val
    with pytest.raises(RuntimeError, match="mode"):
        ops.flow_map(rows, theta, cst, stats, stats, modes=(0, 5, 0))
    with pytest.raises(RuntimeError, match="C = 4097"):
        ops.gumbel_posterior(torch.zeros(1, 4097, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.flow_nll(cols["thickness"], cols["intensity"][:1], cols["slant"], theta, cst, stats)
    with pytest.raises(ValueError):
        ops.flow_nll(cols["thickness"].double(), cols["intensity"], cols["slant"], theta, cst, stats)
