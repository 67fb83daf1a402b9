"""The deepscm_vae family without a GPU: the drop-in classes against fixtures recorded from the reference's own
``VAEEncoder`` / ``VAEDecoder`` (tests/golden/vae_*.npz: seeds and results, no weights), the closed form of the pyro
likelihood against ``torch.distributions`` in fp64, gradients, data classes, and the executors of ``ali_hip.vae`` on
CPU tensors against the plain loop.

A fixture was recorded under ``torch.manual_seed(seed)``: encoder, decoder, ``init_weights``, then the batch
(x, attributes, z, eps) from the same stream -- the same constructor order consumes the same draws."""
import os

import numpy as np
import pytest
import torch

FAMILIES = ("mnist_b4", "audio_d8_b2", "whale_d8_b2")


def _family(name):
    import deepscm_vae.audio_mnist as am
    import deepscm_vae.mnist as mm
    import deepscm_vae.training_utils as tu
    import deepscm_vae.whalecalls as wm

    def mnist_attrs(B):
        c = {"digit": torch.eye(10)[torch.randint(0, 10, (B,))]}
        for k in ("intensity", "slant", "thickness"):
            c[k] = torch.rand(B) * 2 - 1
        return c

    return {"mnist_b4": (mm, mm.MorphoMNISTVAE, tu.init_weights, (28, 28), mnist_attrs),
            "audio_d8_b2": (am, am.VAE, am.init_weights, (128, 128),
                            lambda B: {k: torch.eye(n)[torch.randint(0, n, (B,))] for k, n in am.ATTRIBUTE_DIMS.items()}),
            "whale_d8_b2": (wm, wm.WhaleCallVAE, wm.init_weights, (256, 256),
                            lambda B: {"call_type": torch.eye(3)[torch.randint(0, 3, (B,))]})}[name]


def build(name, golden_dir):
    """(fixture, vae, x, c, z, eps) rebuilt from the fixture's seed"""
    fx = np.load(os.path.join(golden_dir, f"vae_{name}.npz"))
    mod, _, init, hw, attr_fn = _family(name)
    B, d, S = int(fx["B"]), int(fx["d"]), int(fx["S"])
    torch.manual_seed(int(fx["seed"]))
    enc = mod.VAEEncoder() if d < 0 else mod.VAEEncoder(d)
    dec = mod.VAEDecoder() if d < 0 else mod.VAEDecoder(d)
    enc.apply(init), dec.apply(init)
    x = torch.rand(B, 1, *hw) * 2 - 1
    c = attr_fn(B)
    z = torch.randn(B, 512, 1, 1)
    eps = torch.randn(S, B, 512, 1, 1)
    vae = _family(name)[1]() if d < 0 else _family(name)[1](d=d)
    vae.encoder, vae.decoder = enc, dec
    return fx, vae, x, c, z, eps


def _close(got, want, rtol=1e-5):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(np.abs(want).max(), 1e-300)
    assert np.abs(got - want).max() <= rtol * scale, (np.abs(got - want).max(), scale)


@pytest.mark.parametrize("name", FAMILIES)
def test_drop_in_reproduces_the_reference_classes(name, golden_dir):
    fx, vae, x, c, z, eps = build(name, golden_dir)
    for tag, m in (("encoder", vae.encoder), ("decoder", vae.decoder)):
        sd = m.state_dict()
        assert list(sd.keys()) == list(fx[f"{tag}_keys"])
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(fx[f"{tag}_shapes"])
        _close([v.double().sum().item() for v in sd.values()], fx[f"{tag}_sums"], 1e-9)
        _close([v.double().abs().sum().item() for v in sd.values()], fx[f"{tag}_abs"], 1e-9)
    assert set(vae.state_dict()) == {f"encoder.{k}" for k in fx["encoder_keys"]} | {f"decoder.{k}"
                                                                                   for k in fx["decoder_keys"]}
    B, S, klw = int(fx["B"]), int(fx["S"]), float(fx["kl_weight"])
    with torch.no_grad():
        mean, lv = vae.encoder(x, c)
        img = vae.decoder(z, c).reshape(B, -1)
        elbo = vae.elbo(x, c, num_samples=S, kl_weight=klw, eps=eps)
    assert mean.shape == lv.shape == (B, 512, 1, 1)
    _close(mean.reshape(B, -1)[:, ::16], fx["mean"])
    _close(lv.reshape(B, -1)[:, ::16], fx["log_var"])
    _close(img[:, ::int(fx["image_step"])], fx["image"])
    _close(img.double().abs().sum().item(), fx["image_abs"])
    _close(elbo.item(), fx["elbo"])
    _close(elbo.item(), fx["lp"].mean() - klw * fx["dkl"].mean())


def test_closed_form_is_the_transformed_distribution_log_prob():
    """TransformedDistribution(MultivariateNormal(0, I), AffineTransform(bias, scale)).log_prob(x) and the whale
    family's Normal(...).log_prob(x).sum(1) in fp64"""
    from torch.distributions import AffineTransform, MultivariateNormal, Normal, TransformedDistribution
    from deepscm_vae._vae import gaussian_log_prob
    g = torch.Generator().manual_seed(5)
    for P, log_var in ((7, -5.0), (50, -5.0), (12, 0.7)):
        x = torch.randn(3, P, generator=g, dtype=torch.float64)
        bias = torch.randn(3, P, generator=g, dtype=torch.float64)
        scale = torch.exp(torch.ones(P, dtype=torch.float64) * log_var / 2)
        base = MultivariateNormal(torch.zeros(P, dtype=torch.float64), torch.eye(P, dtype=torch.float64))
        want = TransformedDistribution(base, [AffineTransform(bias, scale)]).log_prob(x)
        got = gaussian_log_prob(x, bias, log_var)
        assert torch.allclose(got, want, rtol=1e-13, atol=0), (got, want)
        base1 = Normal(torch.zeros(P, dtype=torch.float64), torch.ones(P, dtype=torch.float64))
        want1 = TransformedDistribution(base1, [AffineTransform(bias, scale)]).log_prob(x).sum(1)
        assert torch.allclose(got, want1, rtol=1e-13, atol=0)


def test_broadcast_mean_of_the_reference_is_the_difference_of_means():
    g = torch.Generator().manual_seed(6)
    lp, dkl = torch.randn(5, generator=g, dtype=torch.float64), torch.rand(5, 1, 1, generator=g, dtype=torch.float64)
    assert torch.allclose((lp - 10.0 * dkl).mean(), lp.mean() - 10.0 * dkl.mean(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", FAMILIES)
def test_elbo_backward_fills_every_gradient(name, golden_dir):
    _, vae, x, c, _, eps = build(name, golden_dir)
    (-vae.elbo(x, c, num_samples=2, kl_weight=10, eps=eps)).backward()
    unused = {"decoder.digit_embedding.weight"} if name.startswith("whale") else set()      # (reference :287)
    for k, p in vae.named_parameters():
        if k in unused:
            assert p.grad is None
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, k
    assert vae(x, c, num_samples=1).dim() == 0          # forward is the elbo


def test_sample_multiplies_by_the_variance(golden_dir):
    _, vae, x, c, _, eps = build("mnist_b4", golden_dir)
    with torch.no_grad():
        mean, lv = vae.encoder(x, c)
        z = vae.encoder.sample(x, c, 'cpu', eps=eps[0])
    assert torch.equal(z, mean + eps[0] * torch.exp(lv))
    torch.manual_seed(1)
    a = vae.encoder.sample(x, c)
    torch.manual_seed(1)
    assert torch.equal(a, mean + torch.randn(mean.shape) * torch.exp(lv))


def test_data_classes_raise_and_pickles_load():
    import io
    import deepscm_vae.audio_mnist as am
    import deepscm_vae.whalecalls as wm
    with pytest.raises(ImportError, match="AudioMNISTData"):
        am.AudioMNISTData("x.zip")
    with pytest.raises(ImportError, match="WhaleCallData"):
        wm.WhaleCallData("a", "b", "c")
    vae = am.VAE(d=8)
    buf = io.BytesIO()
    torch.save({"vae": vae}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)["vae"]
    assert list(back.state_dict()) == list(vae.state_dict())
    assert not any("base" in k or "dist" in k for k in vae.state_dict())


def test_executors_on_cpu_equal_the_plain_loop(golden_dir):
    import copy
    from ali_hip.vae import VaeReconstructor, VaeStepper
    _, vae, x, c, _, eps = build("mnist_b4", golden_dir)
    ref = copy.deepcopy(vae)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    stepper = VaeStepper(vae, lr=1e-3, kl_weight=10, num_samples=2)
    for _ in range(2):
        opt.zero_grad()
        loss = -ref.elbo(x, c, num_samples=2, kl_weight=10, eps=eps)
        loss.backward()
        opt.step()
        r = stepper.step(x, c, eps)
        assert set(r) == {"loss", "logp", "kl"} and all(v.dim() == 0 for v in r.values())
        assert torch.allclose(r["loss"], loss.detach(), rtol=1e-6)
        assert torch.allclose(r["loss"], -(r["logp"] - 10 * r["kl"]), rtol=1e-6)
    for p, q in zip(vae.parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-9)
    # draws named by (seed, step number) when none are given: the counter stream, not torch's generator
    state = torch.get_rng_state()
    stepper.step(x, c)
    assert torch.equal(torch.get_rng_state(), state) and stepper.draws == 1
    c_cf = dict(c, digit=c["digit"].roll(1, 0))
    for rounds in (1, 3):
        e = torch.randn(rounds, 4, 512, 1, 1)
        for cf in (None, c_cf):
            with torch.no_grad():
                want = 0
                for r_ in range(rounds):
                    want = want + vae.decoder(vae.encoder.sample(x, c, 'cpu', eps=e[r_]), cf or c)
                want = want / rounds
            got = VaeReconstructor(vae, rounds=rounds).add(x, c, cf, e)
            assert torch.allclose(got, want, rtol=1e-6, atol=1e-12)


def test_host_side_argument_checks():
    """bad shapes are refused before any launch (no GPU needed to get the error)"""
    import ctypes
    import ali_hip
    lib = ali_hip.load()
    one = ctypes.c_void_p(16)
    assert lib.ali_vae_loglik(one, one, 0, 1, 4, -5.0, None, 1.0, 1.0, one, None, one, 1 << 20, None) != 0
    assert lib.ali_vae_loglik(one, one, 4, 1, 4, -5.0, None, 1.0, 1.0, one, None, one, 16, None) != 0     # workspace
    assert lib.ali_vae_latent_bwd(one, 8, one, one, one, 4, 1, 2, 16, 0.5, 1.0, None, one, one, 16, 0, None, None) != 0
    assert b"ali_vae_latent_bwd" in lib.ali_last_error()
