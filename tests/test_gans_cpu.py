"""CPU-side checks of the ``gans/`` family (no GPU): the drop-in surface, the CPU semantics of the penalty and the
critic loss, and the closed form of the penalty's parameter gradients that ``ali_hip.gan`` runs on the device --
evaluated here with stock torch ops in fp64 against ``autograd.grad(create_graph=True)`` + ``backward``."""
import builtins
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's state_dict keys (gans/audio_mnist.py: Generator :175-189, Discriminator :203-216)
G_KEYS = [f"layers.{i}.{p}" for i in (0, 3, 5, 7, 9, 11) for p in ("weight", "bias")]
D_KEYS = [f"layers.{i}.{p}" for i in (0, 2, 4, 6, 8, 11) for p in ("weight", "bias")]


def test_imports_without_pyro_sklearn_torchaudio(monkeypatch):
    real = builtins.__import__

    def guarded(name, *a, **k):
        if name.split(".")[0] in ("pyro", "sklearn", "torchaudio", "librosa"):
            raise ImportError(f"{name} is not available in this test")
        return real(name, *a, **k)

    for mod in [m for m in sys.modules if m == "gans" or m.startswith("gans.")]:
        monkeypatch.delitem(sys.modules, mod)
    monkeypatch.setattr(builtins, "__import__", guarded)
    import gans.audio_mnist as gm
    assert gm.LATENT_DIM == 100 and gm.IMAGE_SHAPE == (128, 128)
    for name in ("init_weights", "Generator", "Discriminator", "compute_gradient_penalty", "wgan_loss_it", "train",
                 "AudioMNISTData", "VALIDATION_RUNS"):
        assert hasattr(gm, name), name
    with pytest.raises(ImportError):
        gm.AudioMNISTData("nowhere.zip")


def test_state_dict_keys_and_shapes():
    import gans.audio_mnist as gm
    d = 4
    G, D = gm.Generator(d), gm.Discriminator(d)
    assert list(G.state_dict()) == G_KEYS and list(D.state_dict()) == D_KEYS
    shapes_g = {"layers.0.weight": (256 * d, 100), "layers.3.weight": (16 * d, 8 * d, 5, 5),
                "layers.11.weight": (d, 1, 5, 5), "layers.11.bias": (1,)}
    shapes_d = {"layers.0.weight": (d, 1, 5, 5), "layers.8.weight": (16 * d, 8 * d, 5, 5), "layers.11.weight": (1, 16 * d)}
    for k, s in shapes_g.items():
        assert tuple(G.state_dict()[k].shape) == s, k
    for k, s in shapes_d.items():
        assert tuple(D.state_dict()[k].shape) == s, k
    # a state dict with the reference's names loads
    G.load_state_dict({k: torch.full_like(v, 0.5) for k, v in zip(G_KEYS, G.state_dict().values())})
    D.load_state_dict({k: torch.full_like(v, 0.25) for k, v in zip(D_KEYS, D.state_dict().values())})
    assert float(G.layers[0].weight.detach()[0, 0]) == 0.5 and float(D.layers[11].weight.detach()[0, 0]) == 0.25
    assert G.device.type == "cpu" and D.device.type == "cpu"
    assert gm.Generator().layers[0].out_features == 256 * 64 and gm.Discriminator().layers[11].in_features == 1024


def test_output_shapes_and_init():
    import gans.audio_mnist as gm
    torch.manual_seed(0)
    G, D = gm.Generator(4), gm.Discriminator(4)
    G.apply(gm.init_weights)
    D.apply(gm.init_weights)
    assert float(D.layers[0].bias.detach().abs().max()) == 0 and float(D.layers[0].weight.detach().std()) < 2e-3
    assert float(G.layers[0].weight.detach().std()) > 1e-2          # the Linear keeps torch's default initialisation
    x = G(torch.randn(3, 100, 1, 1))
    assert x.shape == (3, 1, 128, 128) and float(x.abs().max()) <= 1
    assert D(x).shape == (3, 1) and D(x.reshape(3, 128, 128)).shape == (3, 1)


def _models(d, seed, dtype=torch.float64):
    import gans.audio_mnist as gm
    torch.manual_seed(seed)
    D = gm.Discriminator(d)
    with torch.no_grad():
        for p in D.parameters():                 # weights large enough for gradient norms away from 0
            p.copy_(torch.randn(p.shape) * (0.12 if p.dim() > 1 else 0.1))
    return D.to(dtype)


def test_penalty_and_loss_equal_direct_autograd():
    import gans.audio_mnist as gm
    D = _models(4, 1)
    g = torch.Generator().manual_seed(2)
    x_real, x_fake = (torch.rand(2, 1, 128, 128, generator=g, dtype=torch.float64) * 2 - 1 for _ in range(2))
    xh = (0.3 * x_real + 0.7 * x_fake)
    pen = gm.compute_gradient_penalty(D, xh.clone())
    x = xh.clone().requires_grad_(True)
    grad = torch.autograd.grad(D(x).sum(), x, create_graph=True)[0]
    direct = ((grad.flatten(1).norm(dim=1) - 1) ** 2).mean()
    assert pen.requires_grad and torch.allclose(pen, direct, rtol=1e-12, atol=0)
    torch.manual_seed(5)
    loss = gm.wgan_loss_it(D, x_real, x_fake, penalty_weight=7.0)
    torch.manual_seed(5)
    eps = torch.rand((2, 1, 1, 1))
    xr = eps * x_real + (1 - eps) * x_fake
    want = D(x_fake) - D(x_real) + 7.0 * gm.compute_gradient_penalty(D, xr)
    assert loss.shape == (2, 1) and torch.allclose(loss, want, rtol=1e-12, atol=0)


def closed_form_penalty_grads(D, xhat, weight):
    """The contract of ``ali_hip.gan``: backward from gy = 1 keeping h_l, tangent v = d(weight * P)/d g0, tangent
    FORWARD pass u_l = act'(a_l) * conv(W_l, u_{l-1}) without bias, dW_l = conv weight gradient of (u_{l-1}, h_l),
    dw_head = sum_b flat(u_5).  Stock torch ops, no double backward.  Returns (penalty, {param name: grad})."""
    convs = [m for m in D.layers if isinstance(m, torch.nn.Conv2d)]
    head = D.layers[-1]
    B = xhat.shape[0]
    with torch.no_grad():
        a = [xhat]
        for c in convs:
            a.append(F.leaky_relu(F.conv2d(a[-1], c.weight, c.bias, stride=2), 0.2))
        mask = [torch.where(t > 0, torch.ones_like(t), torch.full_like(t, 0.2)) for t in a[1:]]
        g = head.weight.reshape(1, -1, 1, 1).expand(B, -1, 1, 1)           # g_5 = w, broadcast over the batch
        h = [None] * 5
        for l in range(4, -1, -1):
            h[l] = mask[l] * g
            g = F.conv_transpose2d(h[l], convs[l].weight, stride=2,
                                   output_padding=(a[l].shape[-1] - 5) % 2)       # dgrad(W_l, h_l)
        g0 = g
        n = g0.flatten(1).norm(dim=1)
        pen = ((n - 1) ** 2).mean()
        v = (weight * (2.0 / B) * (1 - 1 / n)).reshape(B, 1, 1, 1) * g0
        u = [v]
        for l in range(5):
            u.append(mask[l] * F.conv2d(u[-1], convs[l].weight, None, stride=2))
    grads = {}
    for l, c in enumerate(convs):                     # the conv weight gradient: autograd of the bilinear form
        w = c.weight.detach().clone().requires_grad_(True)
        (F.conv2d(u[l], w, None, stride=2) * h[l]).sum().backward()
        grads[f"layers.{2 * l}.weight"] = w.grad
        grads[f"layers.{2 * l}.bias"] = torch.zeros_like(c.bias)
    grads["layers.11.weight"] = u[5].flatten(1).sum(0, keepdim=True)
    grads["layers.11.bias"] = torch.zeros_like(head.bias)
    return pen, grads


def test_closed_form_of_the_penalty_gradient_equals_double_backward():
    """d=4, B=2, fp64: the tangent-pass closed form equals create_graph + backward to 1e-10 relative, every bias and
    the interpolates get exactly zero."""
    import gans.audio_mnist as gm
    D = _models(4, 3)
    g = torch.Generator().manual_seed(4)
    xhat = torch.rand(2, 1, 128, 128, generator=g, dtype=torch.float64) * 2 - 1
    lam = 10.0
    x = xhat.clone().requires_grad_(True)
    pen = gm.compute_gradient_penalty(D, x)
    D.zero_grad()
    (lam * pen).backward()
    pen_cf, grads = closed_form_penalty_grads(D, xhat, lam)
    assert abs(float(pen_cf) - float(pen)) <= 1e-12 * abs(float(pen))
    for name, p in D.named_parameters():
        want = p.grad if p.grad is not None else torch.zeros_like(p)
        err, scale = (grads[name] - want).abs().max().item(), want.abs().max().item()
        print(f"{name}: max err {err:.3e}, max |grad| {scale:.3e}")
        if name.endswith("bias"):
            assert scale == 0.0 and err == 0.0, name
        else:
            assert scale > 0 and err <= 1e-10 * scale, (name, err, scale)
    assert x.grad is None or float(x.grad.abs().max()) == 0.0


def test_gan_stepper_needs_a_device():
    import gans.audio_mnist as gm
    from ali_hip.gan import GanStepper
    G, D = gm.Generator(4), gm.Discriminator(4)
    with pytest.raises(RuntimeError, match="CUDA"):
        GanStepper(G, D)
    with pytest.raises(NotImplementedError):
        GanStepper(G, D, loss_mode="lsgan")
    with pytest.raises(NotImplementedError, match="weight_decay"):
        GanStepper(G, D, discriminator_weight_decay=1e-4)


def test_train_on_cpu_returns_the_four_objects():
    import gans.audio_mnist as gm
    from image_scms import _spect
    from image_scms.audio_mnist import STFT
    g = torch.Generator().manual_seed(0)
    data = _spect.WaveformData(torch.randn(2, 8000, generator=g) * 0.1, {}, **STFT, device="cpu")
    assert next(data.stream(batch_size=2))["audio"].shape[1:] == (128, 128)
    for mode in ("gan", "wgan"):
        G, D, oD, oG = gm.train(data, n_epochs=1, batch_size=2, generator_size=2, discriminator_size=2, loss_mode=mode,
                                save_images_every=None)
        assert isinstance(G, gm.Generator) and isinstance(D, gm.Discriminator)
        assert len(oD.state_dict()["state"]) == 12 and len(oG.state_dict()["state"]) == 12
    with pytest.raises(NotImplementedError):
        gm.train(data, n_epochs=1, loss_mode="hinge")


def test_uniform_reference_is_a_stream_of_its_own():
    from ali_hip import source
    a = source.uniform_reference(7, 3, 64)
    assert a.dtype == torch.float32 and float(a.min()) >= 0 and float(a.max()) < 1
    assert torch.equal(a[5:9], source.uniform_reference(7, 3, 4, offset=5))
    assert not torch.equal(a, source.uniform_reference(7, 4, 64)) and not torch.equal(a, source.uniform_reference(8, 3, 64))


def test_new_symbols_declared_bound_and_exported():
    import ali_hip
    from ali_hip import _lib, ops
    header = open(os.path.join(ROOT, "include", "ali_hip.h")).read()
    lib = ali_hip.load()
    for name in ("ali_gp_mix", "ali_gp_penalty", "ali_wgan_critic"):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("gp_mix", "gp_penalty", "wgan_critic"):
        assert callable(getattr(ops, name))
