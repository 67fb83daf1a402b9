"""The attribute_shap family without a GPU: the estimator's torch statement (``ali_hip.attrib``) on a linear model, where
it has a closed form; the loop ``shap.GradientExplainer`` runs on the script's model class -- batches of samples, the
model's repeat / reshape grouping, one backward per class of ``outputs[:, c].sum()`` -- written out in fp64 against the
statement's formula (the proof that the grouping does not change the gradient in eval mode); ``AttributeModel.forward``
against the script's class body, bit for bit; the return type of the ``GradientExplainer`` shim; the row order of the
generator's input rows; the refusals; and the host references of the new RNG stream."""
import copy

import numpy as np
import pytest
import torch

SLICES = {"digit": (0, 10), "thickness": (10, 1), "intensity": (11, 1), "slant": (12, 1)}


def _models(seed=0):
    import image_scms.mnist as pm
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(seed)
    return pm.Generator().eval(), MNISTClassifier().eval()


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(n, 13)
    a[torch.arange(n), torch.randint(0, 10, (n,), generator=g)] = 1.0
    a[:, 10:] = torch.rand(n, 3, generator=g) * 2 - 1
    return a


def _draws(R, S, n_draws, Nb, seed, latent=512):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, Nb, (R, S), generator=g), torch.rand(R, S, generator=g),
            torch.randn(R, S, n_draws, latent, generator=g))


# ------------------------------------------------------------------------------------------------ the estimator
def test_linear_model_has_the_closed_form_and_is_complete():
    from ali_hip.attrib import expected_gradients
    g = torch.Generator().manual_seed(3)
    R, S, Nb, A, C = 3, 7, 5, 13, 4
    W = torch.randn(C, A, generator=g, dtype=torch.float64)
    x, bg = torch.randn(R, A, generator=g, dtype=torch.float64), torch.randn(Nb, A, generator=g, dtype=torch.float64)
    idx, t, _ = _draws(R, S, 1, Nb, 4, latent=1)
    phi = expected_gradients(lambda a: a @ W.T, x, bg, idx, t.double())
    want = W.unsqueeze(0) * (x - bg[idx].mean(dim=1)).unsqueeze(1)
    assert phi.shape == (R, C, A)
    assert (phi - want).abs().max().item() <= 1e-13 * want.abs().max().item()
    # completeness: sum_a phi[r, c, :] = f_c(x[r]) - mean_k f_c(bg[idx[r, k]])
    gap = phi.sum(dim=2) - (x @ W.T - (bg[idx] @ W.T).mean(dim=1))
    assert gap.abs().max().item() <= 1e-13 * (x @ W.T).abs().max().item()
    only = expected_gradients(lambda a: a @ W.T, x, bg, idx, t.double(), classes=[2])
    assert torch.equal(only[:, 2], phi[:, 2]) and not only[:, [0, 1, 3]].any()


def _script_model(G, clf, n_samples):
    """the body of the script's ``VaeShapClf.forward`` / ``BiganShapClf.forward`` with the z draw handed in"""
    def forward(a, z):
        a = {
            "digit": a[:, :, :10].repeat(n_samples, 1, 1).reshape((-1, 10)),
            "thickness": a[:, :, 10:11].repeat(n_samples, 1, 1).reshape((-1, 1)),
            "intensity": a[:, :, 11:12].repeat(n_samples, 1, 1).reshape((-1, 1)),
            "slant": a[:, :, 12:13].repeat(n_samples, 1, 1).reshape((-1, 1))
        }
        img = G(z, a)
        return clf(img).softmax(1).reshape((-1, n_samples, 10)).mean(dim=1)
    return forward


def test_the_shap_loop_written_out_equals_the_formula_in_fp64():
    """R=2, S=6, n_draws=2, Nb=5, batches of 4 samples.  In a batch of nb inputs the model's ``repeat`` puts input i at
    the rows s * nb + i, and its ``reshape((-1, n_draws, 10)).mean(1)`` averages the CONSECUTIVE rows o * n_draws ..:
    output row o mixes inputs.  ``outputs[:, c].sum()`` still holds every repeated row once with weight 1 / n_draws,
    so its gradient with respect to input i is the one of the per-input mean."""
    from ali_hip.attrib import eg_statement, mixed_rows
    R, S, nd, Nb, batch = 2, 6, 2, 5, 4
    G, clf = _models(0)
    G, clf = G.double(), clf.double()
    x, bg = _rows(R, 1).double(), _rows(Nb, 2).double()
    idx, t, z = _draws(R, S, nd, Nb, 5)
    t, z = t.double(), z.double()
    want = eg_statement(G, clf, x, bg, idx, t, z, SLICES)
    model = _script_model(G, clf, nd)
    a, delta = mixed_rows(x, bg, idx, t)
    phi = torch.zeros(R, 10, 13, dtype=torch.float64)
    for r in range(R):
        grads = [[] for _ in range(10)]
        for lo in range(0, S, batch):
            hi = min(S, lo + batch)
            nb = hi - lo
            X = a[r, lo:hi].reshape(nb, 1, 13).clone().requires_grad_(True)
            # the z of repeated row s * nb + i is draw s of sample lo + i
            zb = z[r, lo:hi].permute(1, 0, 2).reshape(nd * nb, 512, 1, 1)
            outputs = model(X, zb)
            assert outputs.shape == (nb, 10)
            for c in range(10):
                g, = torch.autograd.grad(outputs[:, c].sum(), X, retain_graph=True)
                grads[c].append(g.reshape(nb, 13))
        for c in range(10):
            phi[r, c] = (delta[r] * torch.cat(grads[c])).mean(dim=0)
    scale = want.abs().max().item()
    assert scale > 0
    assert (phi - want).abs().max().item() <= 1e-12 * scale
    # ... and the grouping is real: with more than one input per batch the model's rows are not the per-input means
    X = a[0, :batch].reshape(batch, 1, 13)
    zb = z[0, :batch].permute(1, 0, 2).reshape(nd * batch, 512, 1, 1)
    per_input = clf(G(zb, {k: X[:, 0, o:o + w].repeat(nd, 1) for k, (o, w) in SLICES.items()})).softmax(1)
    per_input = per_input.reshape(nd, batch, 10).mean(dim=0)
    with torch.no_grad():
        assert not torch.allclose(model(X, zb), per_input, rtol=1e-9, atol=0)


def test_executor_on_cpu_tensors_runs_the_statement_and_draws_the_device_streams():
    from ali_hip import rng
    from ali_hip.attrib import ExpectedGradients, eg_statement, value_statement
    G, clf = _models(1)
    x, bg = _rows(2, 3), _rows(5, 4)
    ex = ExpectedGradients(G, clf, bg, n_draws=2, nsamples=3, seed=11)
    idx, t, z = _draws(2, 3, 2, 5, 6)
    phi = ex.shap_values(x, draws={"idx": idx, "t": t, "z": z})
    assert phi.shape == (2, 10, 13) and phi.dtype == torch.float32
    assert torch.equal(phi, eg_statement(G, clf, x, bg, idx, t, z, SLICES))
    as_dict = ex.shap_values({k: x[:, o:o + w] for k, (o, w) in SLICES.items()}, draws={"idx": idx, "t": t, "z": z})
    assert torch.equal(as_dict, phi)
    assert ex._calls == 0                                       # nothing was drawn
    drawn = ex.shap_values(x.reshape(2, 1, 13))
    i0 = torch.from_numpy(rng.eg_index_reference(11, 0, 6, 5)).reshape(2, 3)
    t0 = rng.eg_t_reference(11, 0, 6).reshape(2, 3)
    z0 = rng.normal_reference(11, 0, 2 * 3 * 2 * 512).float().reshape(2, 3, 2, 512)
    assert torch.equal(drawn, eg_statement(G, clf, x, bg, i0, t0, z0, SLICES)) and ex._calls == 1
    assert not torch.equal(ex.shap_values(x), drawn) and ex._calls == 2      # the next call draws anew
    zv = torch.randn(2, 2, 512, generator=torch.Generator().manual_seed(2))
    assert torch.equal(ex.value(x, zv), value_statement(G, clf, x, zv, SLICES))
    assert all(p.grad is None for m in (G, clf) for p in m.parameters())


# ------------------------------------------------------------------------------------------------ drop-in surface
def test_attribute_model_forward_equals_the_scripts_class_body_bit_for_bit():
    from explain.attribute_shap import AttributeModel
    G, clf = _models(2)
    n_samples, N = 4, 3
    a = _rows(N, 7).reshape(N, 1, 13)
    z = torch.randn(N * n_samples, 512, 1, 1, generator=torch.Generator().manual_seed(8))
    model = AttributeModel(G, clf, n_samples)
    with torch.no_grad():
        got, want = model(a, z), _script_model(G, clf, n_samples)(a, z)
        assert got.shape == (N, 10) and torch.equal(got, want)
        assert torch.equal(model(a.numpy(), z), want)                       # (the script's numpy branch)
        torch.manual_seed(5)
        drawn = model(a)
        torch.manual_seed(5)
        assert torch.equal(drawn, model(a, torch.randn((N * n_samples, 512, 1, 1))))


def test_gradient_explainer_returns_what_the_scripts_reshape_expects():
    from explain.attribute_shap import AttributeModel, GradientExplainer
    G, clf = _models(3)
    bg = _rows(5, 9).reshape(5, 1, 13)
    ex = GradientExplainer(AttributeModel(G, clf, 2), bg, seed=4)
    a_expl = _rows(1, 10).reshape(1, 1, 13)
    vals = ex.shap_values(a_expl, nsamples=3)
    assert isinstance(vals, list) and len(vals) == 10
    assert all(isinstance(v, np.ndarray) and v.shape == (1, 1, 13) for v in vals)
    picked = np.array(vals).reshape((10, 13))[:, [10, 11, 12]]               # the script's line, unchanged
    assert picked.shape == (3 * 0 + 10, 3) and np.isfinite(picked).all()
    two = ex.shap_values(_rows(2, 11).reshape(2, 1, 13), nsamples=3)
    assert len(two) == 10 and two[0].shape == (2, 1, 13)
    every = ex.explain_all(_rows(5, 12).reshape(5, 1, 13), batch=2, nsamples=3)
    assert isinstance(every, np.ndarray) and every.shape == (5, 10, 13)
    with pytest.raises(TypeError):
        GradientExplainer(torch.nn.Linear(13, 10), bg)


def test_row_order_of_the_input_rows_and_delta():
    from ali_hip.attrib import input_rows_statement
    G, _ = _models(4)
    R, S, nd, Nb = 2, 3, 2, 5
    x, bg = _rows(R, 13), _rows(Nb, 14)
    idx, t, z = _draws(R, S, nd, Nb, 15)
    rows, delta = input_rows_statement(G, x, bg, idx, t, z, SLICES)
    assert rows.shape == (R * S * nd, 512 + 256 + 3) and delta.shape == (R, S, 13)
    for r in range(R):
        for k in range(S):
            b = bg[idx[r, k]]
            a = t[r, k] * x[r] + (1 - t[r, k]) * b
            assert torch.equal(delta[r, k], x[r] - b)
            for s in range(nd):
                row = rows[(r * S + k) * nd + s]
                assert torch.equal(row[:512], z[r, k, s])
                assert torch.allclose(row[512:768], a[:10] @ G.digit_embedding.weight, rtol=1e-5, atol=1e-6)
                # the generator reads its continuous planes in sorted key order: intensity, slant, thickness
                assert torch.equal(row[768:], torch.stack([a[11], a[12], a[10]]))
    # the statement's rows are the generator's own input: same image as the module computes from the attribute dict
    with torch.no_grad():
        a_all = (t.unsqueeze(-1) * x.unsqueeze(1) + (1 - t.unsqueeze(-1)) * bg[idx]).unsqueeze(2).expand(R, S, nd, 13)
        a_all = a_all.reshape(-1, 13)
        img = G(z.reshape(-1, 512, 1, 1), {k: a_all[:, o:o + w] for k, (o, w) in SLICES.items()})
        assert torch.allclose(G.layers(rows.reshape(-1, 771, 1, 1)), img, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    import image_scms.audio_mnist as am
    from ali_hip.attrib import ExpectedGradients
    G, clf = _models(5)
    bg = _rows(4, 1)
    with pytest.raises(ValueError, match="training mode"):
        ExpectedGradients(copy.deepcopy(G).train(), clf, bg)
    with pytest.raises(ValueError, match="training mode"):
        ExpectedGradients(G, copy.deepcopy(clf).train(), bg)
    ex = ExpectedGradients(G, clf, bg, nsamples=2, n_draws=1)
    G.train()
    with pytest.raises(ValueError, match="training mode"):                  # switched after construction
        ex.shap_values(_rows(1, 2))
    with pytest.raises(ValueError, match="training mode"):
        ex.value(_rows(1, 2))
    G.eval()
    with pytest.raises(TypeError):
        ExpectedGradients(torch.nn.Sequential(torch.nn.Linear(3, 3)), clf, bg)          # a foreign decoder
    with pytest.raises(TypeError):
        ExpectedGradients(G, torch.nn.Sequential(*copy.deepcopy(clf)), bg)              # a foreign classifier
    with pytest.raises(TypeError, match="SpectGenerator"):
        ExpectedGradients(am.Generator(8).eval(), clf, bg)
    keyed = {"digit": bg[:, :10], "thickness": bg[:, 10:11], "intensity": bg[:, 11:12], "tilt": bg[:, 12:13]}
    with pytest.raises(ValueError, match="attributes"):
        ExpectedGradients(G, clf, {k: v for k, v in keyed.items() if k != "tilt"})      # too few for the decoder's row
    with pytest.raises(ValueError, match="attributes"):
        ExpectedGradients(G, clf, {k: v for k, v in keyed.items() if k != "digit"})     # no table key
    ok = ExpectedGradients(G, clf, {("slant" if k == "tilt" else k): v for k, v in keyed.items()}, nsamples=2, n_draws=1)
    with pytest.raises(ValueError, match="attributes"):
        ok.shap_values(keyed)                                                           # keys that are not the decoder's
    with pytest.raises(ValueError):
        ok.shap_values(torch.zeros(1, 12))
    with pytest.raises(ValueError, match="unknown"):
        ok.shap_values(bg[:1], draws={"index": torch.zeros(1, 2)})


# ------------------------------------------------------------------------------------------------ the "eg" stream
def test_eg_stream_references():
    from ali_hip import rng
    n = 4096
    for Nb in (1, 5, 200):
        i = rng.eg_index_reference(0x5EED, 3, n, Nb)
        assert i.dtype == np.int64 and i.shape == (n,) and i.min() >= 0 and i.max() < Nb
        assert Nb == 1 or (i.min() == 0 and i.max() == Nb - 1)              # both ends are reached
    t = rng.eg_t_reference(0x5EED, 3, n)
    assert t.dtype == torch.float32 and t.shape == (n,) and t.min() >= 0 and t.max() < 1
    assert 0.45 < t.mean().item() < 0.55
    # reproducible from (seed, counter, offset): a chunk drawn at offset k is the slice [k:] of the whole
    whole_i, whole_t = rng.eg_index_reference(7, 2, 64, 200), rng.eg_t_reference(7, 2, 64)
    for k in (5, 36):
        assert (rng.eg_index_reference(7, 2, 64 - k, 200, offset=k) == whole_i[k:]).all()
        assert torch.equal(rng.eg_t_reference(7, 2, 64 - k, offset=k), whole_t[k:])
    assert (rng.eg_index_reference(7, None, 64, 200) == rng.eg_index_reference(7, 0, 64, 200)).all()
    assert not (rng.eg_index_reference(8, 2, 64, 200) == whole_i).all()
    assert not torch.equal(rng.eg_t_reference(7, 3, 64), whole_t)
    # a key of its own under every (seed, counter) of the recorded cases
    import rng_cases as rc
    for seed, counter in rc.KEYS:
        keys = {name: rng.key(seed, counter, name) for name in rng.STREAMS}
        assert len(set(keys.values())) == len(keys)
        assert all(keys["eg"] != v for k, v in keys.items() if k != "eg")
    assert rng.STREAMS["eg"] == (rng.EG_STREAM,) and rng.EG_STREAM == int.from_bytes(b"EGBRIDX1", "big")
    src = open(rng.__file__.replace("ali_hip/rng.py", "csrc/ali_rng.h")).read()
    assert f"kEgStream = 0x{rng.EG_STREAM:016X}ull" in src                  # the header and the module, together
