"""The cf_metrics family without a GPU: the drop-in ``train_morphomnist_ae`` module, the two stage capabilities it
needs from ``ali_hip.chain`` (ReLU, Flatten + Linear on a map of more than 28 positions) as plans and routes, and the
CPU statement of ``ali_hip.cfmetrics`` against loops written here in the scripts' order.
"""
import math
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


def test_module_resolves_under_the_name_the_checkpoints_pickle():
    import train_morphomnist_ae as ae
    assert ae.Encoder.__module__ == "train_morphomnist_ae" and ae.Decoder.__module__ == "train_morphomnist_ae"
    names = {a.dest: a.default for a in ae.parser._actions}
    assert names["steps"] == 200 and names["cls"] is None and names["output_path"] == "morphomnist_ae.tar"
    assert names["latent_dim"] == 100 and names["batch_size"] == 64 and names["learning_rate"] == 1e-4
    assert names["data_dir"] == ""


@pytest.mark.parametrize("c,latent", [(64, 10), (8, 4)])
def test_state_dict_keys_shapes_and_output_shapes(c, latent):
    import train_morphomnist_ae as ae
    E, G = ae.Encoder(c, latent), ae.Decoder(c, latent)
    assert [(k, tuple(v.shape)) for k, v in E.state_dict().items()] == [
        ("conv1.weight", (c, 1, 4, 4)), ("conv1.bias", (c,)), ("conv2.weight", (2 * c, c, 4, 4)),
        ("conv2.bias", (2 * c,)), ("fc.weight", (latent, 2 * c * 49)), ("fc.bias", (latent,))]
    assert [(k, tuple(v.shape)) for k, v in G.state_dict().items()] == [
        ("fc.weight", (2 * c * 49, latent)), ("fc.bias", (2 * c * 49,)), ("conv2.weight", (2 * c, c, 4, 4)),
        ("conv2.bias", (c,)), ("conv1.weight", (c, 1, 4, 4)), ("conv1.bias", (1,))]
    x = torch.rand(3, 1, 28, 28) * 2 - 1
    z = E(x)
    assert tuple(z.shape) == (3, latent) and tuple(G(z).shape) == (3, 1, 28, 28)
    # the chain view shares the parameter objects and stays out of the module's state
    E.chain_view(), G.chain_view()
    assert len(E.state_dict()) == 6 and len(G.state_dict()) == 6
    assert E.chain_view()[0] is E.conv1 and G.chain_view()[0] is G.fc and E.chain_view() is E.chain_view()


def test_cpu_forward_is_the_functional_statement():
    import train_morphomnist_ae as ae
    torch.manual_seed(4)
    E, G = ae.Encoder(8, 4).double(), ae.Decoder(8, 4).double()
    x = torch.rand(5, 1, 28, 28, dtype=torch.float64) * 2 - 1
    h = F.relu(F.conv2d(x, E.conv1.weight, E.conv1.bias, 2, 1))
    h = F.relu(F.conv2d(h, E.conv2.weight, E.conv2.bias, 2, 1))
    z = F.linear(h.reshape(5, -1), E.fc.weight, E.fc.bias)
    assert torch.equal(E(x), z)
    u = F.linear(z, G.fc.weight, G.fc.bias).reshape(5, 16, 7, 7)
    u = F.relu(F.conv_transpose2d(u, G.conv2.weight, G.conv2.bias, 2, 1))
    y = torch.tanh(F.conv_transpose2d(u, G.conv1.weight, G.conv1.bias, 2, 1))
    assert torch.equal(G(z), y)
    # the Sequential view is the same function (it is what the device path parses)
    assert torch.equal(E.chain_view()(x), z) and torch.equal(G.chain_view()(z), y)


def test_chain_plan_takes_relu_as_leaky_with_slope_zero():
    from ali_hip.chain import ChainPlan
    from ali_hip.ops import ACT_LEAKY, ACT_NONE, ACT_TANH
    plan = ChainPlan(nn.Sequential(nn.Conv2d(1, 8, 3), nn.ReLU(), nn.Conv2d(8, 4, 3), nn.LeakyReLU(0.2),
                                   nn.ConvTranspose2d(4, 4, 3), nn.Tanh(), nn.Conv2d(4, 4, 1)))
    assert [(st.act, st.slope) for st in plan.stages] == [(ACT_LEAKY, 0.0), (ACT_LEAKY, 0.2), (ACT_TANH, 0.0),
                                                          (ACT_NONE, 0.0)]
    # a ReLU stage keeps the epilogue capabilities of a LeakyReLU stage
    from ali_hip.chain import route
    assert route(plan.stages[0], (2, 9, 9, 4), 1).fold_ok


def test_routes_of_the_large_and_the_small_flatten():
    import train_morphomnist_ae as ae
    from ali_hip.chain import get_plan, trace
    E, G = ae.Encoder(64, 10), ae.Decoder(64, 10)
    tr = trace(get_plan(E.chain_view()), (2, 28, 28, 4), 1)
    assert [t[1] for t in tr] == [(2, 14, 14, 64), (2, 7, 7, 128), (2, 1, 1, 10)]
    last = tr[-1][2]
    assert last.fwd == "flat_gemm" and last.dgrad == "flat_gemm" and last.wgrad == ("flat_repack", "colsum")
    assert last.wgrad_fold == last.wgrad
    assert [t[2].fwd for t in tr[:2]] == ["conv", "conv"]
    tg = trace(get_plan(G.chain_view()), (2, 1, 1, 12), 10)
    assert [t[1] for t in tg] == [(2, 7, 7, 128), (2, 14, 14, 64), (2, 28, 28, 1)]
    assert tg[0][2].wgrad == ("linear_repack", "unflat") and tg[1][2].fwd == "convT"
    assert tg[2][2].wgrad[0] == "convT_scatter" and tg[2][2].fwd in ("scatter", "scatter_gemm")
    # a map of <= 28 positions keeps the route it had: the (h, w) kernel of the conv GEMMs
    small = get_plan(nn.Sequential(nn.Conv2d(1, 8, 3), nn.ReLU(), nn.Flatten(), nn.Linear(8 * 4 * 7, 5)))
    ts = trace(small, (2, 6, 9, 4), 1)
    assert ts[-1][0] == (2, 4, 7, 8) and ts[-1][2].fwd == "conv" and ts[-1][2].wgrad == ("conv", "fused")
    assert ts[-1][2].dgrad == "conv"
    # 29 positions is the first size on the new route; padded channels in front of it are refused
    big = get_plan(nn.Sequential(nn.Conv2d(1, 8, 3), nn.ReLU(), nn.Flatten(), nn.Linear(8 * 29, 5)))
    assert trace(big, (2, 3, 31, 4), 1)[-1][2].fwd == "flat_gemm"
    first = get_plan(nn.Sequential(nn.Flatten(), nn.Linear(3 * 30, 5)))
    with pytest.raises(NotImplementedError, match="padded channels"):
        trace(first, (2, 5, 6, 4), 3)


def _scripts_js(p, q):
    """mnist_oracle_scores.py:19-28 restated"""
    p, q = p.softmax(1), q.softmax(1)
    m = 0.5 * (p + q)
    kl = lambda a, b: (a * ((a + 1e-6).log() - (b + 1e-6).log())).sum(1)      # noqa: E731
    return 0.5 * (kl(p, m) + kl(q, m))


def test_js_div_properties():
    from ali_hip.cfmetrics import js_div
    g = torch.Generator().manual_seed(2)
    p, q = torch.randn(7, 10, generator=g, dtype=torch.float64) * 3, torch.randn(7, 10, generator=g, dtype=torch.float64)
    assert torch.allclose(js_div(p, q), _scripts_js(p, q), rtol=1e-13, atol=0)
    assert torch.allclose(js_div(p, q), js_div(q, p), rtol=1e-13, atol=1e-16)
    assert torch.equal(js_div(p, p), torch.zeros(7, dtype=torch.float64))
    far = torch.zeros(2, 10, dtype=torch.float64)
    far[:, 0] = 1e4
    other = far.roll(1, 1)
    d = js_div(far, other)
    assert (d <= math.log(2.0)).all() and (d > 0.69).all()
    assert (js_div(p, q) >= 0).all() and (js_div(p, q) <= math.log(2.0)).all()


def metrics_case(dtype=torch.float64, B=5, J=2, seed=11):
    """10 classes, capacity 8, latent 4, J oracles, B rows: (clf, aes, oracles, x, cf, orig)"""
    import train_morphomnist_ae as ae
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(seed)
    clf = MNISTClassifier().to(dtype)
    aes = {k: (ae.Encoder(8, 4).to(dtype), ae.Decoder(8, 4).to(dtype)) for k in list(range(10)) + ["all"]}
    oracles = [MNISTClassifier().to(dtype) for _ in range(J)]
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.rand(B, 1, 28, 28, generator=g) * 2 - 1).to(dtype)
    cf = (torch.rand(B, 1, 28, 28, generator=g) * 2 - 1).to(dtype)
    orig = torch.randint(0, 10, (B,), generator=g)
    return clf, aes, oracles, x, cf, orig


def per_row_loop(clf, aes, oracles, x, cf, orig, target=None):
    """the scripts' statements, one row at a time (morphomnist_cf_metrics.py:104-118,192-231,
    mnist_oracle_scores.py:181-191)"""
    rows = []
    with torch.no_grad():
        for i in range(len(cf)):
            c, xi = cf[i:i + 1], x[i:i + 1]
            label = clf(c).argmax(1).item()
            t = label if target is None else int(target[i])
            rec = lambda k: aes[k][1](aes[k][0](c)).detach()      # noqa: E731
            row = {"label": label, "l1": c.abs().sum().item(),
                   "o_rec": (c - rec(int(orig[i]))).square().sum().item(),
                   "t_rec": (c - rec(t)).square().sum().item(),
                   "all_rec": (rec(t) - rec("all")).square().sum().item()}
            dists = [o(xi) for o in oracles]
            row["os"] = [int(label == o(c).argmax(1).item()) for o in oracles]
            row["lvs"] = [_scripts_js(dists[j], oracles[j](c)).item() for j in range(len(oracles))]
            rows.append(row)
    return rows


@pytest.mark.parametrize("with_target", [False, True])
def test_cfmetrics_on_cpu_fp64_equals_the_per_row_loop(with_target):
    from ali_hip.cfmetrics import CfMetrics
    clf, aes, oracles, x, cf, orig = metrics_case()
    target = (orig + 3) % 10 if with_target else None
    want = per_row_loop(clf, aes, oracles, x, cf, orig, target)
    m = CfMetrics(clf, aes, oracles)
    out = m.add(x, cf, orig, target)
    assert set(out) == {"label", "l1", "o_rec", "t_rec", "all_rec", "os", "lvs"}
    assert out["label"].tolist() == [r["label"] for r in want]
    assert out["os"].tolist() == [r["os"] for r in want] and tuple(out["lvs"].shape) == (5, 2)
    for k in ("l1", "o_rec", "t_rec", "all_rec"):
        np.testing.assert_allclose(out[k].numpy(), [r[k] for r in want], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["lvs"].numpy(), [r["lvs"] for r in want], rtol=1e-9, atol=1e-15)
    # a second batch, then the table: 2B rows in order under the scripts' names
    m.add(x.flip(0), cf.flip(0), orig.flip(0), None if target is None else target.flip(0))
    t = m.table("bigan")
    assert list(t) == (["bigan_label", "l1_bigan", "o_rec_bigan", "t_rec_bigan", "all_rec_bigan"]
                       + [n for j in range(2) for n in (f"bigan_os_{j}", f"bigan_lvs_{j}")])
    both = want + want[::-1]
    assert t["bigan_label"].tolist() == [r["label"] for r in both]
    assert t["bigan_os_1"].tolist() == [r["os"][1] for r in both]
    np.testing.assert_allclose(t["t_rec_bigan"], [r["t_rec"] for r in both], rtol=1e-12)
    np.testing.assert_allclose(t["bigan_lvs_0"], [r["lvs"][0] for r in both], rtol=1e-9, atol=1e-15)
    m.reset()
    assert all(len(v) == 0 for v in m.table("bigan").values())


def test_cfmetrics_constructor_checks():
    from ali_hip.cfmetrics import CfMetrics
    clf, aes, oracles, *_ = metrics_case(J=0)
    with pytest.raises(ValueError, match="all"):
        CfMetrics(clf, {k: v for k, v in aes.items() if k != "all"})
    with pytest.raises(ValueError, match=r"\[7\]"):
        CfMetrics(clf, {k: v for k, v in aes.items() if k != 7})
    m = CfMetrics(clf, aes)            # no oracles: the reconstruction table alone
    _, _, _, x, cf, orig = metrics_case(J=0)
    out = m.add(x, cf, orig)
    assert tuple(out["os"].shape) == (5, 0) and list(m.table("cf")) == ["cf_label", "l1_cf", "o_rec_cf", "t_rec_cf",
                                                                        "all_rec_cf"]


def test_ae_stepper_on_cpu_is_the_loop_body():
    import copy
    import train_morphomnist_ae as ae
    from ali_hip.cfmetrics import AeStepper
    torch.manual_seed(5)
    E, G = ae.Encoder(8, 4), ae.Decoder(8, 4)
    E2, G2 = copy.deepcopy(E), copy.deepcopy(G)
    x = torch.rand(6, 1, 28, 28) * 2 - 1
    r = AeStepper(E, G, lr=1e-3).step(x)
    opt = torch.optim.Adam(list(E2.parameters()) + list(G2.parameters()), lr=1e-3, betas=(0.5, 0.9))
    loss = (x - G2(E2(x))).square().mean()
    loss.backward()
    opt.step()
    assert torch.equal(r["loss"], loss.detach())
    for a, b in zip(list(E.parameters()) + list(G.parameters()), list(E2.parameters()) + list(G2.parameters())):
        assert torch.equal(a, b)


def test_train_on_synthetic_files(tmp_path, capsys):
    import train_morphomnist_ae as ae
    g = torch.Generator().manual_seed(8)
    for split, n in (("train", 96), ("test", 32)):
        digit = torch.arange(n) % 10
        # every digit is its own blob, so there is something to learn in two epochs
        base = torch.zeros(10, 28, 28)
        for d in range(10):
            base[d, 2 + 2 * d:8 + 2 * d, 4:24] = 255.0
        x = (base[digit] * (0.6 + 0.4 * torch.rand(n, 1, 1, generator=g))).reshape(n, 784)
        a = torch.cat([torch.eye(10)[digit], torch.rand(n, 3, generator=g)], dim=1)
        np.save(tmp_path / f"mnist-x-{split}.npy", x.numpy())
        np.save(tmp_path / f"mnist-a-{split}.npy", a.numpy())
    torch.manual_seed(0)
    E, G = ae.train(str(tmp_path), steps=2, latent_dim=4, batch_size=16, learning_rate=2e-3, device="cpu")
    out = capsys.readouterr().out
    assert "96 training and 32 test images" in out and "Epoch 2/2" in out
    losses = [float(v) for v in re.findall(r"test mse ([0-9.eE+-]+)", out)]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    x0 = 2 * torch.from_numpy(np.load(tmp_path / "mnist-x-test.npy")).float().reshape(-1, 1, 28, 28) / 255.0 - 1
    torch.manual_seed(0)
    with torch.no_grad():
        E0 = ae.Encoder(latent_dim=4)              # (the order train() builds them in)
        G0 = ae.Decoder(latent_dim=4)
        start = (G0(E0(x0)) - x0).square().mean().item()
    assert losses[1] < losses[0] < start
    assert isinstance(E, ae.Encoder) and isinstance(G, ae.Decoder) and E.fc.out_features == 4
    ae.train(str(tmp_path), steps=1, cls=3, latent_dim=4, batch_size=16, device="cpu")
    assert "10 training and 3 test images" in capsys.readouterr().out       # digits 3, 13, ... of 96 and of 32
