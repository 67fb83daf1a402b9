"""``attribute_scms`` on the device: ``MNISTCausalGraph`` through ``ali_hip.flow`` (autograd, the three-launch stepper
eager and from HIP graphs, sampling, counterfactuals) against the torch statement on the CPU, and
``AudioMNISTCausalGraph`` across the Gumbel kernel.  Tolerances: the yardstick of tests/flow_cases.py."""
import functools

import numpy as np
import pytest
import torch

import flow_cases as fc
from flow_cases import NAMES, within_yardstick

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def table():
    return fc.synth_attrs(512, seed=21)


def device_graph(seed=22):
    import attribute_scms.mnist as am
    torch.manual_seed(seed)
    return am.MNISTCausalGraph(table(), device="cuda")


def _obs(a, dtype=None, device=None):
    return {k: v.to(device=device, dtype=dtype) for k, v in fc.columns(a).items()}


def _state(g):
    """parameters in theta's order, then the moving buffers"""
    bn = g.trainable()[0]
    return torch.cat([fc.flat_theta(g)[1].reshape(-1), bn.moving_mean.detach().reshape(-1),
                      bn.moving_variance.detach().reshape(-1)])


def test_log_prob_under_autograd_equals_the_statement():
    g = device_graph()
    assert g._flow is not None and g._flow.matches(g)
    refs = [g.statement(dt) for dt in (torch.float64, torch.float32)]           # before the buffers move
    a = table()
    lp = g.log_prob(_obs(a.cuda()))
    assert list(lp) == list(NAMES) and all(lp[k].shape == (512, 1) for k in NAMES)
    w = torch.randn(512, 3, generator=torch.Generator().manual_seed(1))
    loss = sum((lp[k] * w[:, j:j + 1].cuda()).sum() for j, k in enumerate(NAMES))
    parts, _ = fc.flat_theta(g)
    grads = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, parts)])
    out = []
    for gs, dt in zip(refs, (torch.float64, torch.float32)):
        lps = gs.log_prob(_obs(a, dt))
        ps, _ = fc.flat_theta(gs)
        ls = sum((lps[k] * w[:, j:j + 1].to(dt)).sum() for j, k in enumerate(NAMES))
        out.append((torch.cat([lps[k] for k in NAMES], 1).detach(),
                    torch.cat([x.reshape(-1) for x in torch.autograd.grad(ls, ps)]), _state(gs)[75:]))
    (lp64, g64, mv64), (lp32, g32, mv32) = out
    within_yardstick("log_prob", torch.cat([lp[k] for k in NAMES], 1), lp64, lp32)
    within_yardstick("parameter gradients", grads, g64, g32)
    within_yardstick("moving buffers", _state(g)[75:], mv64, mv32)
    # the script's loop: backward into .grad, a torch optimiser steps the views of the flat buffer
    opt = torch.optim.Adam([p for k in NAMES for p in g.get_module(k).parameters()], lr=1e-2)
    before = g._flow.theta.clone()
    lp = g.log_prob(_obs(a.cuda()))
    (-(lp["thickness"] + lp["intensity"] + lp["slant"]).mean()).backward()
    opt.step()
    assert not torch.equal(g._flow.theta, before) and g._flow.matches(g)
    both = g.log_prob({**_obs(a.cuda()), "digit": a[:, :10].cuda()})
    assert list(both) == ["thickness", "intensity", "slant", "digit"] and both["digit"].shape == (512,)


def _statement_steps(g, batches, dtype):
    gs = g.statement(dtype)
    opt = torch.optim.Adam(fc.flat_theta(gs)[0], lr=1e-2)
    losses = []
    for a in batches:
        opt.zero_grad()
        lp = gs.log_prob(_obs(a, dtype))
        loss = -(lp["thickness"] + lp["intensity"] + lp["slant"]).mean()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return _state(gs), torch.stack(losses)


@pytest.mark.parametrize("capture", [False, True])
def test_stepper_equals_statement_steps_with_torch_adam(capture):
    from ali_hip.flow import FlowStepper
    g = device_graph()
    a = table()
    sizes = [512, 200, 512] if capture else [512, 512, 512]                     # captured: a ragged batch in between
    batches = [a[:n] for n in sizes]
    (s64, l64), (s32, l32) = _statement_steps(g, batches, torch.float64), _statement_steps(g, batches, torch.float32)
    stepper = FlowStepper(g, lr=1e-2, capture=capture)
    losses = []
    for b in batches:
        out = stepper.step(*(b.cuda()[:, j:j + 1] for j in (10, 11, 12)))
        assert set(out) == {"loss", "lp_thickness", "lp_intensity", "lp_slant"} and out["loss"].is_cuda
        losses.append(out["loss"].clone())
    assert len(stepper.graphs) == (2 if capture else 0)
    assert int(stepper.dev_step) == 3 and int(stepper.arrive) == 0
    within_yardstick(f"losses capture={capture}", torch.stack(losses), l64, l32)
    within_yardstick(f"parameters and buffers after 3 steps capture={capture}", _state(g), s64, s32)
    assert g._flow.matches(g)


def test_train_on_the_device_lowers_the_loss():
    import attribute_scms.mnist as am
    torch.manual_seed(23)
    np.random.seed(23)
    g = am.train(table(), steps=2, device="cuda")
    assert len(g.train_losses) == 2 and g.train_losses[1] < g.train_losses[0]
    assert g._flow is not None and g._flow.theta.is_cuda


def test_sample_and_held_values():
    g = device_graph()
    a = table()
    s = g.sample(n=64)
    assert {k: tuple(v.shape) for k, v in s.items()} == {"thickness": (64, 1), "intensity": (64, 1), "slant": (64, 1),
                                                         "digit": (64,)}
    assert all(v.is_cuda for v in s.values()) and (s["thickness"] > 0).all() and torch.isfinite(s["slant"]).all()
    i_min, i_rng = (float(v) for v in g.consts[:2])
    assert (s["intensity"] >= i_min).all() and (s["intensity"] <= i_min + i_rng).all()
    assert s["digit"].min() >= 0 and s["digit"].max() <= 9
    held = {"thickness": a[:64, 10:11].cuda(), "digit": a[:64, :10].argmax(1).cuda()}
    s = g.sample(held)
    assert s["thickness"] is held["thickness"] and s["digit"] is held["digit"] and s["intensity"].shape == (64, 1)
    # the intensity is drawn under the held thickness: its noise, abducted under that thickness, is standard normal
    noise = g.recover_noise({k: s[k] for k in NAMES})
    assert set(noise) == set(NAMES) and all(noise[k].shape == (64, 1) for k in NAMES)
    assert noise["intensity"].abs().max() < 6
    hi = a[:64, 11:12].cuda()
    s = g.sample({"intensity": hi})
    assert s["intensity"] is hi and s["thickness"].shape == (64, 1) and s["digit"].shape == (64,)


def test_sample_cf_over_100_rows_and_the_training_switch():
    g = device_graph()
    a = table()[:100]
    bn = g.get_module("thickness").td.transforms[0]
    with torch.no_grad():
        bn.moving_mean.fill_(0.8)
        bn.moving_variance.fill_(0.1)
    lp_train = g.log_prob(_obs(a.cuda()))["thickness"].detach().clone()          # batch statistics (moves the buffers)
    g.get_module("thickness").td.transforms[0].training = False                  # causal_graph_cf.py's switch
    g64, g32 = g.statement(torch.float64), g.statement(torch.float32)
    lp_eval = g.log_prob(_obs(a.cuda()))
    assert not torch.allclose(lp_eval["thickness"], lp_train)
    l64, l32 = g64.log_prob(_obs(a, torch.float64)), g32.log_prob(_obs(a))
    within_yardstick("log_prob in eval mode", torch.cat([lp_eval[k] for k in NAMES], 1).detach(),
                     torch.cat([l64[k] for k in NAMES], 1).detach(), torch.cat([l32[k] for k in NAMES], 1).detach())
    digit = a[:, :10].argmax(1)
    obs = {**_obs(a.cuda()), "digit": digit.cuda()}
    obs_int = {"thickness": (a[:, 10:11] + 1).cuda()}
    cf = g.sample_cf(obs, obs_int)
    assert set(cf) == set(NAMES) | {"digit"}
    assert cf["thickness"] is obs_int["thickness"] and torch.equal(cf["digit"], obs["digit"])
    refs = []
    for gs, dt in ((g64, torch.float64), (g32, torch.float32)):
        c = gs.sample_cf({**_obs(a, dt), "digit": digit}, {"thickness": (a[:, 10:11] + 1).to(dt)})
        refs.append(torch.cat([c[k] for k in NAMES], 1).detach())
    within_yardstick("sample_cf", torch.cat([cf[k] for k in NAMES], 1), *refs)
    assert not torch.allclose(cf["intensity"].cpu(), a[:, 11:12])
    # a graph whose structure was changed runs the statement
    g.add_edge("thickness", "slant")
    assert g._flow is not None and not g._flow.matches(g)
    g.remove_edge("thickness", "slant")
    assert g._flow.matches(g)


def test_audio_graph_on_the_device():
    import attribute_scms.audio_mnist as aa
    torch.manual_seed(24)
    sizes = {"country_of_origin": 5, "native_speaker": 2, "accent": 6, "digit": 10, "age": 5, "gender": 2}
    ds = {k: torch.eye(n)[torch.randint(0, n, (256,))].cuda() for k, n in sizes.items()}
    g = aa.AudioMNISTCausalGraph(ds, device="cuda")
    lp = g.log_prob(ds)
    assert all(lp[k].shape == (256,) and lp[k].is_cuda for k in sizes)
    s = g.sample(n=32)
    assert all(s[k].shape == (32,) and s[k].is_cuda and int(s[k].max()) < sizes[k] for k in sizes)
    labels = {k: v.argmax(1) for k, v in ds.items()}
    cf = g.sample_cf(labels, {})
    assert all(torch.equal(cf[k], labels[k]) for k in sizes)                     # the posterior noise regenerates y
    cf = g.sample_cf(labels, {"native_speaker": 1 - labels["native_speaker"]})   # across the Gumbel kernel
    assert torch.equal(cf["native_speaker"], 1 - labels["native_speaker"])
    assert torch.equal(cf["country_of_origin"], labels["country_of_origin"])
    assert cf["accent"].shape == (256,) and int(cf["accent"].max()) < 6
    noise = g.get_module("native_speaker").recover_noise(labels["native_speaker"], ds["country_of_origin"])
    assert noise.shape == (256, 2) and noise.is_cuda and torch.isfinite(noise).all()
    # one autograd training step moves the MLP weights
    params = [p for k in ("native_speaker", "accent") for p in g.get_module(k).parameters()]
    before = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=1e-2)
    lp = g.log_prob({k: ds[k] for k in ("country_of_origin", "native_speaker", "accent", "age")})
    (-(lp["native_speaker"] + lp["accent"]).mean()).backward()
    opt.step()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
