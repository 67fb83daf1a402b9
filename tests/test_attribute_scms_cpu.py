"""CPU-side checks of the ``attribute_scms/`` family (no GPU): the torch statement of the flows that csrc/flow.hip is
tested against (tests/test_gpu_flow_kernels.py) -- inverses, log-determinants against autograd, densities that
integrate to one -- and the graph logic, the Gumbel-max posterior and the training loop on top of it."""
import math
import os
import re

import numpy as np
import pytest
import torch

from attribute_scms import _flows, audio_mnist, causal_module, graph, mnist, training_utils
from attribute_scms.causal_module import CategoricalCM, ConditionalCategoricalCM, TransformedCM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
# round trips and log-determinants: a few hundred ulp of the dtype (the spline divides twice and takes a log)
TOL = {torch.float64: 1e-12, torch.float32: 5e-5}


def synth_attrs(n, seed=0, dtype=torch.float32):
    """a MorphoMNIST-like attribute table [n, 13]: one-hot digit | thickness | intensity (depends on it) | slant"""
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(n, 13, dtype=dtype)
    a[torch.arange(n), torch.randint(0, 10, (n,), generator=g)] = 1
    t = torch.exp(torch.randn(n, generator=g) * 0.3 + 0.8)
    a[:, 10] = t
    a[:, 11] = 60 + 190 * torch.sigmoid(0.5 * t + torch.randn(n, generator=g))
    a[:, 12] = torch.randn(n, generator=g) * 0.3
    return a


def _autograd_log_derivative(f, x):
    x = x.detach().clone().requires_grad_()
    g, = torch.autograd.grad(f(x).sum(), x)
    return g.log()


def _spline_grid(sp, dtype):
    """points crossing +-3 that hit every bin and both pieces of each: either side of every x_k + lambda_k w_k"""
    xk, _, _, lam = (v.detach() for v in sp.processed())
    mid = xk[:-1] + lam * (xk[1:] - xk[:-1])
    pts = torch.cat([torch.linspace(-4, 4, 161, dtype=dtype), 0.5 * (xk[:-1] + mid).to(dtype), 0.5 * (mid + xk[1:]).to(dtype)])
    return pts.reshape(-1, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spline_inverse_logdet_and_knot_derivatives(dtype):
    torch.manual_seed(3)
    sp = _flows.Spline(1).to(dtype)
    x = _spline_grid(sp, dtype)
    y = sp(x)
    assert torch.equal(y[x.abs() > 3], x[x.abs() > 3])                           # identity outside
    assert (sp.inv(y) - x).abs().max() <= TOL[dtype] * 10
    inside = (x.abs() <= 3).flatten()
    ld = sp.log_abs_det_jacobian(x, y)
    assert (ld[~inside] == 0).all()
    assert (ld - _autograd_log_derivative(sp, x)).abs().max() <= TOL[dtype] * 10
    assert (sp._map(y, True)[1] + ld).abs().max() <= TOL[dtype] * 10             # log dx/dy = -log dy/dx
    # every bin, both pieces
    xk, _, d, lam = (v.detach() for v in sp.processed())
    k = (x >= xk[1:-1]).sum(-1)[inside]
    left = ((x[inside, 0] - xk[k]) / (xk[k + 1] - xk[k])) <= lam[k]
    assert {(int(a), bool(b)) for a, b in zip(k, left)} == {(a, b) for a in range(8) for b in (False, True)}
    # monotone, and the derivative at the interior knots is d_k (from the bin on the right)
    assert (ld.exp() > 0).all() and (y[1:161] > y[0:160]).all()
    at_knots = _autograd_log_derivative(sp, xk[1:-1].reshape(-1, 1)).exp().flatten()
    assert (at_knots - d[1:-1]).abs().max() <= TOL[dtype] * 10


@pytest.mark.parametrize("dtype", DTYPES)
def test_affine_and_batchnorm_inverse_and_logdet(dtype):
    torch.manual_seed(4)
    caa = _flows.ConditionalAffineAutoregressive(1, 1).to(dtype)
    with torch.no_grad():
        # log_scale = 5 relu(ctx) - 10 relu(-ctx): beyond both clamp bounds
        caa.nn[0].weight.copy_(torch.tensor([[1.0]] * 5 + [[-1.0]] * 5))
        caa.nn[0].bias.zero_()
        caa.nn[2].weight[1].copy_(torch.tensor([1.0] * 5 + [-2.0] * 5))
        caa.nn[2].bias.zero_()
    ctx = torch.linspace(-3, 3, 41, dtype=dtype).reshape(-1, 1)
    tf = caa.condition(ctx)
    mean, ls = tf._params()
    raw = caa.nn(ctx)[:, 1:]
    assert (raw > 3).any() and (raw < -5).any() and ls.max() <= 3 and ls.min() >= -5
    x = torch.randn(41, 1, dtype=dtype)
    y = tf(x)
    assert (tf.inv(y) - x).abs().max() <= TOL[dtype] * 100                       # (exp(3) amplifies)
    assert (tf.log_abs_det_jacobian(x, y) - _autograd_log_derivative(tf, x)).abs().max() <= TOL[dtype]
    # straight-through: the clamped rows still pass the gradient of log_scale to the network
    g, = torch.autograd.grad(ls.sum(), caa.nn[2].bias)
    assert g[1] == 41

    bn = _flows.BatchNorm(1).to(dtype)
    with torch.no_grad():
        bn.gamma.fill_(1.7)
        bn.beta.fill_(0.3)
        bn.moving_mean.fill_(-0.4)
        bn.moving_variance.fill_(2.5)
    bn.eval()
    y = bn(x)
    assert (bn.inv(y) - x).abs().max() <= TOL[dtype]
    assert (bn.log_abs_det_jacobian(x, y) - _autograd_log_derivative(bn, x)).abs().max() <= TOL[dtype]
    with torch.no_grad():
        bn.gamma.fill_(-1.0)                                                    # gated: g = 1e-6, no gradient to gamma
    lad = bn.log_abs_det_jacobian(x, y)
    assert torch.allclose(lad, torch.full_like(lad, -math.log(1e-6) + 0.5 * math.log(2.5 + 1e-5)))
    assert torch.autograd.grad(bn.inv(y.detach()).sum(), bn.gamma)[0] == 0


def test_batchnorm_statistics():
    bn = _flows.BatchNorm(1)
    y = torch.randn(50, 1) * 2 + 1
    m, v = y.mean(0), y.var(0, unbiased=True)
    assert bn.training
    x = bn.inv(y)
    assert torch.allclose(x, (y - m) * torch.rsqrt(v + 1e-5) * (1 + 1e-6))
    assert torch.allclose(bn.moving_mean, 0.1 * m) and torch.allclose(bn.moving_variance, 0.9 + 0.1 * v)
    assert torch.allclose(bn.log_abs_det_jacobian(x, y), (0.5 * torch.log(v + 1e-5) - math.log(1 + 1e-6)).expand(50, 1))
    before = (bn.moving_mean.clone(), bn.moving_variance.clone())
    fwd = bn(x)                                             # the sampling direction ignores ``training``
    assert torch.allclose(fwd, x / (1 + 1e-6) * torch.sqrt(before[1] + 1e-5) + before[0])
    bn.training = False
    assert torch.equal(bn(x), fwd)
    x2 = bn.inv(y)                                          # eval: the buffers, which stay
    assert torch.allclose(x2, (y - before[0]) * torch.rsqrt(before[1] + 1e-5) * (1 + 1e-6))
    assert torch.equal(bn.moving_mean, before[0]) and torch.equal(bn.moving_variance, before[1])
    assert [n for n, _ in bn.named_parameters()] == ["gamma", "beta"]


def _trapezoid(f, lo, hi, n):
    x = torch.linspace(lo, hi, n, dtype=torch.float64)
    y = f(x.reshape(-1, 1)).flatten()
    return torch.trapezoid(y, x).item()


def test_densities_integrate_to_one():
    torch.manual_seed(5)
    g = mnist.MNISTCausalGraph(synth_attrs(64)).statement(torch.float64)
    bn, caa, sp = g.trainable()
    for tr in (bn, caa, sp):
        tr.training = False
    with torch.no_grad():
        bn.moving_mean.fill_(0.8)
        bn.moving_variance.fill_(0.1)
        bn.gamma.fill_(1.4)
    i_min, i_rng, s_min, s_rng = (float(v) for v in g.consts)
    # thickness on (0, inf): substitute t = exp(z), the density of z over a range that holds all its mass
    total = _trapezoid(lambda z: g.log_prob({"thickness": z.exp()})["thickness"].exp() * z.exp(), -4.0, 5.0, 20001)
    assert abs(total - 1) < 1e-8
    # intensity on its affine range for two thicknesses: substitute the logit, where the density is smooth
    for t in (1.5, 4.0):
        def dens(w):
            p = torch.sigmoid(w)
            lp = g.log_prob({"thickness": torch.full_like(w, t), "intensity": i_min + i_rng * p})["intensity"]
            return lp.exp() * i_rng * p * (1 - p)
        assert abs(_trapezoid(dens, -30.0, 30.0, 40001) - 1) < 1e-8
    # slant on [s_min, s_max] is the part of the spline's density that falls on [0, 1] of its [-3, 3]: its mass is the
    # base measure of the preimage; the density over all of the spline's range integrates to one
    def slant(s):
        return g.log_prob({"slant": s})["slant"].exp()
    whole = _trapezoid(slant, s_min - 9 * s_rng, s_min + 9 * s_rng, 400001)
    assert abs(whole - 1) < 1e-6                                                # (kinks at the knots: trapezoid rule)
    u = sp.inv(torch.tensor([[0.0], [1.0]], dtype=torch.float64)).flatten().detach()
    normal = torch.distributions.Normal(0.0, 1.0)
    part = _trapezoid(slant, s_min, s_min + s_rng, 200001)
    assert abs(part - float(normal.cdf(u[1]) - normal.cdf(u[0]))) < 1e-6


def _toy_graph():
    torch.manual_seed(6)
    g = graph.CausalModuleGraph()
    normal = lambda: torch.distributions.Normal(torch.zeros(1), torch.ones(1))   # noqa: E731
    a = torch.distributions.TransformedDistribution(normal(), [torch.distributions.AffineTransform(2.0, 0.5)])
    b = _flows.ConditionalTransformedDistribution(normal(), [_flows.ConditionalAffineAutoregressive(1, 1)])
    c = torch.distributions.TransformedDistribution(normal(), [_flows.Spline(1)])
    g.add_module("a", TransformedCM(a))
    g.add_module("b", causal_module.ConditionalTransformedCM(b))
    g.add_module("c", TransformedCM(c))
    g.add_module("k", CategoricalCM(torch.distributions.Categorical(probs=torch.tensor([0.2, 0.5, 0.3]))))
    g.add_edge("a", "b")
    return g


def test_graph_logic_on_toy_modules():
    g = _toy_graph()
    order = g.top_sort()
    assert sorted(order) == ["a", "b", "c", "k"] and order.index("a") < order.index("b")
    assert g.parents("b") == ["a"] and g.children("a") == ["b"] and g.parents("a") == []
    s = g.sample(n=7)
    assert {k: tuple(v.shape) for k, v in s.items()} == {"a": (7, 1), "b": (7, 1), "c": (7, 1), "k": (7,)}
    held = {"a": torch.full((5, 1), 3.0)}
    s = g.sample(held)
    assert s["a"] is held["a"] and s["b"].shape == (5, 1)
    obs = {k: v for k, v in g.sample(n=9).items()}
    lp = g.log_prob(obs)
    assert list(lp) == ["a", "b", "c", "k"] and lp["a"].shape == (9, 1) and lp["k"].shape == (9,)
    assert "b" not in g.log_prob({"b": obs["b"], "c": obs["c"]})                 # a parent is missing
    # abduction then prediction under the same parents
    noise = g.recover_noise(obs)
    again = g.get_module("b").condition(obs["a"]).generate(noise["b"], obs["a"])
    assert torch.allclose(again, obs["b"], atol=1e-5)
    cf = g.sample_cf(obs, {})
    for k in obs:
        assert torch.allclose(cf[k].float(), obs[k].float(), atol=1e-5), k
    cf = g.sample_cf(obs, {"a": obs["a"] + 1})
    assert torch.equal(cf["a"], obs["a"] + 1) and not torch.allclose(cf["b"], obs["b"])
    assert torch.allclose(cf["c"], obs["c"], atol=1e-5) and torch.equal(cf["k"], obs["k"])
    g.remove_edge("a", "b")
    assert g.parents("b") == []


def test_categorical_mle_matches_counts():
    labels = torch.tensor([0, 2, 2, 5, 5, 5, 2, 0])
    cm = audio_mnist.categorical_mle(labels)
    assert cm.n_categories == 6
    assert torch.allclose(cm.d.probs, torch.tensor([2, 0, 3, 0, 0, 3]) / 8.0)
    assert cm.recover_noise(labels) is labels and cm.generate(labels) is labels and list(cm.parameters()) == []
    a = synth_attrs(500)
    g = mnist.MNISTCausalGraph(a)
    assert torch.allclose(g.get_module("digit").d.probs, a[:, :10].sum(0) / 500)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [2, 6])
def test_gumbel_posterior_regenerates_the_observation(dtype, C):
    torch.manual_seed(7)
    net = torch.nn.Linear(3, C).to(dtype)
    cm = ConditionalCategoricalCM(net, C)
    ctx = torch.randn(2000, 3, dtype=dtype) * 3
    y = torch.randint(0, C, (2000,))
    noise = cm.recover_noise(y, ctx)
    assert noise.shape == (2000, C) and noise.dtype == dtype
    assert torch.equal(cm.generate(noise, ctx), y)
    # the shifted lse: logits the unshifted one overflows on
    big = torch.tensor([[1000.0, 0.0]], dtype=dtype)
    n = causal_module.gumbel_posterior(big, torch.tensor([0]), torch.zeros(1, 2, dtype=dtype))
    assert torch.isfinite(n[0, 0]) and n[0, 0] == 0


def test_gumbel_distribution_and_reference_recipe():
    torch.manual_seed(8)
    g = causal_module.gumbel_distribution().sample((20000,))
    assert abs(g.mean().item() - 0.5772) < 0.03 and abs(g.var().item() - math.pi ** 2 / 6) < 0.08
    from ali_hip import source
    a = source.gumbel_reference(7, 3, 4096)
    assert a.dtype == torch.float64 and torch.isfinite(a).all()
    assert a.min() >= -math.log(-math.log(0.5 / 2 ** 24)) and a.max() <= -math.log(-math.log(1 - 0.5 / 2 ** 24))
    assert torch.equal(a[100:164], source.gumbel_reference(7, 3, 64, offset=100))
    assert not torch.equal(a, source.gumbel_reference(7, 4, 4096)) and not torch.equal(a, source.gumbel_reference(8, 3, 4096))
    assert abs(a.mean().item() - 0.5772) < 0.06


def test_mnist_train_lowers_the_loss_and_samples():
    torch.manual_seed(9)
    np.random.seed(9)
    a = synth_attrs(300)
    g = mnist.train(a, steps=3, device="cpu")
    assert len(g.train_losses) == 3 and g.train_losses[-1] < g.train_losses[0]
    s = g.sample(n=16)
    assert {k: tuple(v.shape) for k, v in s.items()} == {"thickness": (16, 1), "intensity": (16, 1), "slant": (16, 1),
                                                         "digit": (16,)}
    assert (s["thickness"] > 0).all()
    assert (s["intensity"] >= a[:, 11].min()).all() and (s["intensity"] <= a[:, 11].max()).all()
    # the script's switch (causal_graph_cf.py) and the counterfactual of one observed row
    g.get_module("thickness").td.transforms[0].training = False
    obs = {"thickness": a[:1, 10:11], "intensity": a[:1, 11:12], "slant": a[:1, 12:13], "digit": a[:1, :10].argmax(1)}
    cf = g.sample_cf(obs, {"thickness": obs["thickness"] + 1})
    assert cf["intensity"] != obs["intensity"] and torch.allclose(cf["slant"], obs["slant"], atol=1e-5)
    assert len(g.get_module("thickness").parameters()) == 2 and len(g.get_module("intensity").parameters()) == 4
    assert len(g.get_module("slant").parameters()) == 4
    g.get_module("slant").clear_cache()
    twin = g.statement(torch.float64)
    lp, lp64 = g.log_prob(obs), twin.log_prob({k: v.double() if v.is_floating_point() else v for k, v in obs.items()})
    for k in ("thickness", "intensity", "slant"):
        assert lp64[k].dtype == torch.float64 and torch.allclose(lp[k].double(), lp64[k], atol=1e-4), k


def test_audio_graph_on_the_cpu():
    torch.manual_seed(10)
    np.random.seed(10)
    sizes = {"country_of_origin": 5, "native_speaker": 2, "accent": 6, "digit": 10, "age": 5, "gender": 2}
    ds = {k: torch.eye(n)[torch.randint(0, n, (200,))] for k, n in sizes.items()}
    g = audio_mnist.train(ds, steps=3, device="cpu", lr=1e-2)
    assert g.train_losses[-1] < g.train_losses[0]
    labels = {k: v.argmax(1) for k, v in ds.items()}
    lp = g.log_prob(labels)
    assert all(lp[k].shape == (200,) for k in sizes)
    s = g.sample(n=11)
    assert all(s[k].shape == (11,) and s[k].max() < sizes[k] for k in sizes)
    cf = g.sample_cf(labels, {})
    assert all(torch.equal(cf[k], labels[k]) for k in sizes)
    cf = g.sample_cf(labels, {"native_speaker": 1 - labels["native_speaker"]})
    assert torch.equal(cf["country_of_origin"], labels["country_of_origin"]) and cf["accent"].shape == (200,)
    assert len(audio_mnist.VALIDATION_RUNS) == 10
    with pytest.raises(ImportError):
        audio_mnist.AudioMNISTData("nowhere.zip")
    net = audio_mnist.dense_net(4, 8, 3, n_hidden_layers=2)
    assert [type(m).__name__ for m in net] == ["Linear", "ReLU", "Linear", "ReLU", "Linear", "ReLU", "Linear"]


def test_batchify_and_flow_walks():
    x, y = torch.arange(10), torch.arange(12)
    parts = list(training_utils.batchify(x, y, batch_size=4))
    assert [len(p[0]) for p in parts] == [4, 4, 2] and torch.equal(parts[2][0], torch.tensor([8, 9]))
    d = torch.distributions.TransformedDistribution(torch.distributions.Normal(torch.zeros(1), torch.ones(1)),
                                                    [_flows.BatchNorm(1), torch.distributions.ExpTransform()])
    d.transforms[0].training = False
    z = torch.randn(5, 1)
    assert torch.allclose(training_utils.nf_inverse(d, training_utils.nf_forward(d, z)), z, atol=1e-6)
    assert len(training_utils.dist_parameters(d)) == 2


def test_new_symbols_declared_bound_and_exported():
    import ali_hip
    from ali_hip import _lib, flow, ops
    header = open(os.path.join(ROOT, "include", "ali_hip.h")).read()
    lib = ali_hip.load()
    for name in ("ali_flow_stats", "ali_flow_nll", "ali_flow_map", "ali_gumbel_posterior"):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("flow_stats", "flow_nll", "flow_map", "gumbel_posterior"):
        assert callable(getattr(ops, name))
    assert ops.FLOW_THETA == 75 and "#define ALI_FLOW_THETA 75" in header
    for name in ("FlowLogProb", "FlowStepper"):
        assert hasattr(flow, name)
