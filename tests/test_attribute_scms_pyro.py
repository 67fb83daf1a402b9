"""The pyro-specific definitions that ``attribute_scms/_flows.py`` restates from pyro's documentation (DESIGN.md 3.13,
"unverified against pyro"), against pyro itself: parameters are copied into pyro's transforms and ``log_prob`` and
``sample_cf`` compared.  Skips wherever pyro is not installed -- which includes every machine this project's suite
runs on -- and shows nothing until someone runs it where pyro exists."""
import pytest
import torch

pyro = pytest.importorskip("pyro")


def _pyro_twin(g):
    """the MorphoMNIST graph's three flows built from pyro's transforms with this graph's parameters"""
    import pyro.distributions as dist
    import pyro.distributions.transforms as T
    bn, caa, sp = g.trainable()
    i_min, i_rng, s_min, s_rng = g.consts
    pbn = T.BatchNorm(1)
    pbn.load_state_dict(bn.state_dict())
    pbn.training = bn.training
    pcaa = T.conditional_affine_autoregressive(1, 1)
    # pyro's ConditionalAutoRegressiveNN: with one variable every path from it is masked away; the context reaches the
    # hidden layer through the leading context_dim input columns and the outputs are (mean, log_scale)
    made = pcaa.nn
    with torch.no_grad():
        for layer in made.layers:
            layer.weight.zero_()
        made.layers[0].weight[:, :1].copy_(caa.nn[0].weight)
        made.layers[0].bias.copy_(caa.nn[0].bias)
        made.layers[-1].weight.copy_(caa.nn[2].weight)
        made.layers[-1].bias.copy_(caa.nn[2].bias)
    psp = T.Spline(1)
    psp.load_state_dict(sp.state_dict())
    normal = lambda: dist.Normal(torch.zeros(1), torch.ones(1))   # noqa: E731
    t = dist.TransformedDistribution(normal(), [pbn, T.ExpTransform()])
    i = dist.ConditionalTransformedDistribution(normal(), [pcaa, T.SigmoidTransform(), T.AffineTransform(i_min, i_rng)])
    s = dist.TransformedDistribution(normal(), [psp, T.AffineTransform(s_min, s_rng)])
    return t, i, s


@pytest.mark.parametrize("training", [True, False])
def test_log_prob_and_counterfactual_against_pyro(training):
    import attribute_scms.mnist as am
    from attribute_scms.training_utils import nf_forward, nf_inverse
    from flow_cases import synth_attrs
    torch.manual_seed(31)
    a = synth_attrs(256, seed=31)
    g = am.MNISTCausalGraph(a)
    for tr in g.trainable():
        tr.training = training
    pt, pi, ps = _pyro_twin(g)
    th, it, sl = a[:, 10:11], a[:, 11:12], a[:, 12:13]
    lp = g.log_prob({"thickness": th, "intensity": it, "slant": sl})
    assert torch.allclose(lp["thickness"].flatten(), pt.log_prob(th).flatten(), atol=1e-4)
    assert torch.allclose(lp["intensity"].flatten(), pi.condition(th).log_prob(it).flatten(), atol=1e-4)
    assert torch.allclose(lp["slant"].flatten(), ps.log_prob(sl).flatten(), atol=1e-4)
    if training:
        return
    cf = g.sample_cf({"thickness": th, "intensity": it, "slant": sl, "digit": a[:, :10].argmax(1)},
                     {"thickness": th + 1})
    cond_obs, cond_cf = pi.condition(th), pi.condition(th + 1)
    expect = nf_forward(cond_cf, nf_inverse(cond_obs, it))
    assert torch.allclose(cf["intensity"], expect, rtol=1e-4, atol=1e-3)
    assert torch.allclose(cf["slant"], nf_forward(ps, nf_inverse(ps, sl)), atol=1e-4)
