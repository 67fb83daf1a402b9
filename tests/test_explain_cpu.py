"""The explain family without a GPU: the drop-in classes of ``explain/cf_example.py`` on CPU tensors against this file's
own torch statement of the two loops (bit for bit under one seed: RNG order, ``features_to_ignore`` /
``categorical_features`` handling, ``train_z``), the return shapes of the sweep for all three metrics with and without
a hit, ``explain_batch`` against single calls, and the host-side argument checks of the new kernels."""
import pytest
import torch


def _models(seed=0):
    import image_scms.mnist as pm
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(seed)
    E, G, clf = pm.Encoder(), pm.Generator(), MNISTClassifier()
    return E.eval(), G.eval(), clf.eval()


def _batch(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(B, 1, 28, 28, generator=g))
    digit = torch.zeros(B, 10)
    digit[torch.arange(B), torch.randint(0, 10, (B,), generator=g)] = 1.0
    attrs = {"digit": digit}
    for k in ("thickness", "intensity", "slant"):
        attrs[k] = torch.rand(B, 1, generator=g) * 2 - 1
    return x, attrs


def _first_max_without(row, t):
    best = None
    for i in range(row.shape[1]):
        if i != t and (best is None or row[0, i].item() > best.item()):
            best = row[0, i]
    return best


def hinge_statement(E, G, clf, x, attrs, target, train_z, steps, lr, categorical, ignored, c=10.0, init=None,
                    update_z=False):
    """The loop as the reference states it, for one image.  z joins the optimiser without requires_grad (it is made
    after the other variables were switched on), so it stays what it was drawn as unless ``update_z``."""
    codes = E(x, attrs).detach()
    with torch.no_grad():
        p0 = clf(x).softmax(1)
    if init is None:
        var = {k: 0.01 * torch.randn((1, attrs[k].shape[1])) for k in attrs if k not in ignored}
        if train_z:
            var["z"] = torch.randn(codes.shape)
    else:
        var = {k: v.clone() for k, v in init.items()}
    for k, v in var.items():
        if k != "z" or update_z:
            v.requires_grad = True
    opt = torch.optim.Adam(list(var.values()), lr=lr)

    def decode():
        a = {}
        for k in attrs:
            a[k] = attrs[k] if k in ignored else (var[k].softmax(1) if k in categorical else var[k].tanh())
        return G(var["z"].tanh() if train_z else codes, a)

    last = None
    for _ in range(steps):
        opt.zero_grad()
        xc = decode()
        pred = clf(xc)
        if target is None:
            h = (pred - p0).square().mean()
        else:
            h = (_first_max_without(pred, target) - pred[0, target]).mean()
        m = (x - xc).abs().mean()
        loss = c * h + m
        loss.backward()
        opt.step()
        last = (loss.detach(), h.detach(), m.detach())
    return decode().detach(), {k: v.detach() for k, v in var.items()}, last


HINGE_CASES = [
    dict(target=3, train_z=True, categorical=["digit"], ignored=["thickness", "slant"]),
    dict(target=7, train_z=False, categorical=["digit"], ignored=[]),
    dict(target=None, train_z=True, categorical=[], ignored=["intensity"]),
]


@pytest.mark.parametrize("case", HINGE_CASES, ids=["ignore2-z", "codes", "no-target"])
def test_hinge_explain_equals_the_torch_statement_bit_for_bit(case):
    from explain.cf_example import HingeLossCFExplainer
    E, G, clf = _models()
    x, attrs = _batch(1)
    ex = HingeLossCFExplainer(E, G, clf, "digit", 512, categorical_features=case["categorical"],
                              features_to_ignore=case["ignored"])
    torch.manual_seed(11)
    got = ex.explain(x, attrs, target_class=case["target"], train_z=case["train_z"], steps=3, lr=0.1)
    torch.manual_seed(11)
    want, _, _ = hinge_statement(E, G, clf, x, attrs, case["target"], case["train_z"], 3, 0.1, case["categorical"],
                                 case["ignored"])
    assert got.shape == (1, 1, 28, 28)
    assert torch.equal(got.detach(), want)
    # the draws moved something, and the loop moved it further
    torch.manual_seed(11)
    zero, _, _ = hinge_statement(E, G, clf, x, attrs, case["target"], case["train_z"], 0, 0.1, case["categorical"],
                                 case["ignored"])
    assert not torch.equal(zero, want)


def test_hinge_explain_batch_equals_single_calls():
    from explain.cf_example import HingeLossCFExplainer
    E, G, clf = _models()
    x, attrs = _batch(3)
    ex = HingeLossCFExplainer(E, G, clf, "digit", 512, categorical_features=["digit"], features_to_ignore=["slant"])
    g = torch.Generator().manual_seed(5)
    init = {k: 0.01 * torch.randn(3, attrs[k].shape[1], generator=g) for k in attrs if k != "slant"}
    init["z"] = torch.randn(3, 512, 1, 1, generator=g)
    target = torch.tensor([2, 9, 4])
    got = ex.explain_batch(x, attrs, target, train_z=True, steps=2, lr=0.05, init=init)
    assert got.shape == (3, 1, 28, 28)
    for b in range(3):
        want, _, _ = hinge_statement(E, G, clf, x[b:b + 1], {k: v[b:b + 1] for k, v in attrs.items()}, int(target[b]),
                                     True, 2, 0.05, ["digit"], ["slant"], init={k: v[b:b + 1] for k, v in init.items()})
        assert torch.equal(got[b:b + 1].detach(), want), b
    # update_z: z is optimised too, which the reference's loop never does
    moved = ex.explain_batch(x, attrs, target, train_z=True, steps=2, lr=0.05, init=init, update_z=True)
    want, _, _ = hinge_statement(E, G, clf, x[:1], {k: v[:1] for k, v in attrs.items()}, 2, True, 2, 0.05, ["digit"],
                                 ["slant"], init={k: v[:1] for k, v in init.items()}, update_z=True)
    assert torch.equal(moved[:1].detach(), want) and not torch.equal(moved, got)


def test_max_excluding_takes_the_first_maximum_and_skips_the_class():
    from explain.cf_example import hinge, max_excluding, mse
    y = torch.tensor([[1.0, 5.0, 5.0, 7.0]])
    assert max_excluding(y, 3).item() == 5.0 and max_excluding(y, 3).data_ptr() == y[:, 1].data_ptr()
    assert max_excluding(y, 0).item() == 7.0
    assert torch.equal(hinge(torch.tensor([1.0, -1.0]), torch.tensor([0.25, 3.0])), torch.tensor([0.75, 4.0]))
    a, b = torch.arange(12.0).reshape(2, 1, 2, 3), torch.zeros(2, 1, 2, 3)
    assert torch.equal(mse(a, b), a.square().reshape(2, -1).mean(1))


def sweep_statement(E, G, clf, x, attrs, target, S):
    """samples, predictions and the three metrics of the mixture sweep, stated here"""
    from ali_hip.ssim import ssim
    with torch.no_grad():
        codes = E(x, attrs).repeat(S, 1, 1, 1)
        orig = int(clf(x).argmax(1))
        eye = torch.eye(10)
        p = torch.linspace(0, 1, S).reshape(S, 1)
        a = {k: v.repeat(S, 1) for k, v in attrs.items()}
        a["digit"] = (1 - p) * eye[orig].reshape(1, 10).repeat(S, 1) + p * eye[target].reshape(1, 10).repeat(S, 1)
        samples = G(codes, a)
        preds = clf(samples).argmax(1)
        metrics = {"mixture": p, "mse": (x - samples).square().mean(dim=[1, 2, 3]),
                   "ssim": 1 - ssim((x.repeat(S, 1, 1, 1) + 1) / 2, (samples + 1) / 2, data_range=1.0, size_average=False)}
    return samples, preds, metrics


def _sweep_case():
    """models, one image, and two target classes: one that some but not all sweep rows are classified as (or, failing
    that, all rows), and one that none is"""
    E, G, clf = _models(seed=4)
    x, attrs = _batch(1, seed=2)
    S = 12
    found = {}
    for t in range(10):
        _, preds, _ = sweep_statement(E, G, clf, x, attrs, t, S)
        n = int((preds == t).sum())
        found.setdefault("miss" if n == 0 else "hit", (t, n))
    assert "hit" in found and "miss" in found, found
    return E, G, clf, x, attrs, S, found["hit"][0], found["miss"][0]


@pytest.mark.parametrize("metric", ["mixture", "mse", "ssim"])
def test_sweep_return_shapes_and_contents(metric):
    from explain.cf_example import DeepCounterfactualExplainer
    E, G, clf, x, attrs, S, t_hit, t_miss = _sweep_case()
    ex = DeepCounterfactualExplainer(E, G, clf, "digit")
    # ---- nothing hits: everything comes back, unsorted
    samples, preds, metrics = sweep_statement(E, G, clf, x, attrs, t_miss, S)
    got_s, got_m = ex.explain(x, attrs, t_miss, sample_points=S, metric=metric)
    assert torch.equal(got_s, samples) and torch.equal(got_m, metrics[metric])
    assert got_m.shape == ((S, 1) if metric == "mixture" else (S,))
    # ---- hits
    samples, preds, metrics = sweep_statement(E, G, clf, x, attrs, t_hit, S)
    hit = preds == t_hit
    n = int(hit.sum())
    got_s, got_m = ex.explain(x, attrs, t_hit, sample_points=S, metric=metric)
    if metric == "mixture":
        # the [n, 1] metric is sorted along its last axis: zeros, so every entry is the first hit
        assert got_s.shape == (n, 1, 1, 28, 28) and got_m.shape == (n, 1, 1)
        first = int(hit.nonzero()[0])
        assert torch.equal(got_s, samples[first].expand(n, 1, 1, 28, 28))
        assert torch.equal(got_m, metrics[metric][first].expand(n, 1, 1))
    else:
        order = metrics[metric][hit].argsort()
        assert got_s.shape == (n, 1, 28, 28) and got_m.shape == (n,)
        assert torch.equal(got_s, samples[hit][order]) and torch.equal(got_m, metrics[metric][hit][order])
        assert bool((got_m[1:] >= got_m[:-1]).all())
    # what the callers index
    assert got_s[0][0].shape[-2:] == (28, 28) and got_m.flatten()[0].dim() == 0
    with pytest.raises(ValueError):
        ex.explain(x, attrs, t_hit, sample_points=S, metric="psnr")


def test_sweep_explain_batch_is_a_list_of_single_results():
    from explain.cf_example import DeepCounterfactualExplainer
    E, G, clf = _models(seed=4)
    x, attrs = _batch(2, seed=2)
    ex = DeepCounterfactualExplainer(E, G, clf, "digit")
    out = ex.explain_batch(x, attrs, [1, 6], sample_points=5, metric="mse")
    for b, t in enumerate([1, 6]):
        s, m = ex.explain(x[b:b + 1], {k: v[b:b + 1] for k, v in attrs.items()}, t, sample_points=5, metric="mse")
        assert torch.equal(out[b][0], s) and torch.equal(out[b][1], m)


def test_the_module_needs_neither_tqdm_nor_pytorch_msssim(monkeypatch):
    import builtins
    import importlib
    import sys
    real = builtins.__import__

    def guarded(name, *args, **kwargs):
        if name.split(".")[0] in ("tqdm", "pytorch_msssim"):
            raise ImportError(name)
        return real(name, *args, **kwargs)
    monkeypatch.setattr(builtins, "__import__", guarded)
    monkeypatch.delitem(sys.modules, "explain.cf_example", raising=False)
    mod = importlib.import_module("explain.cf_example")
    assert list(mod.progress(range(3))) == [0, 1, 2]
    for name in ("hinge", "mse", "max_excluding", "DeepCounterfactualExplainer", "HingeLossCFExplainer"):
        assert hasattr(mod, name)


def test_executors_refuse_models_they_do_not_know():
    import torch.nn as nn
    from ali_hip.explain import HingeCFStepper, MixtureSweep
    E, G, clf = _models()
    with pytest.raises(TypeError):
        HingeCFStepper(nn.Linear(2, 2), clf, "digit", ["digit"], [])
    with pytest.raises(TypeError):
        HingeCFStepper(G, nn.Sequential(nn.Flatten(), nn.Linear(784, 10)), "digit", ["digit"], [])
    with pytest.raises(TypeError):
        MixtureSweep(lambda z, a: G(z, a), clf, "digit")
    sweep = MixtureSweep(G, clf, "digit")
    with pytest.raises(ValueError):
        sweep.run(torch.zeros(1, 1, 28, 28), torch.zeros(1, 512, 1, 1), {}, 3, sample_points=1025)


def test_host_side_argument_checks_of_the_explain_kernels():
    from ali_hip import _lib
    lib = _lib.load()
    rc = lib.ali_cf_hinge(None, None, None, None, 10.0, 1, 1, None, None, None)
    assert rc == -1 and b"C = 1" in lib.ali_last_error()
    rc = lib.ali_cf_select(None, None, None, 1025, 10, None, None, None, None)
    assert rc == -1 and b"S = 1025" in lib.ali_last_error()
    rc = lib.ali_row_dist(None, 2, None, 3, 10, 0, None, None, 0, None)
    assert rc == -1 and b"xB = 2" in lib.ali_last_error()
    rc = lib.ali_cf_join(None, 4, None, None, 1, 1, 1 << 24, None, None)
    assert rc == -1 and b"ali_cf_join" in lib.ali_last_error()
    seg = (_lib.AliCfSegment * 1)(_lib.AliCfSegment(2, 2000, 0, 0, -1, 0))
    rc = lib.ali_cf_input_fwd(1, 2000, None, 0, seg, 1, None, 0, 1, 2000, 2016, 1, 1, 2000, None)
    assert rc == -1 and b"width 2000" in lib.ali_last_error()
    seg = (_lib.AliCfSegment * 1)(_lib.AliCfSegment(1, 8, 0, 28, -1, -1))
    rc = lib.ali_cf_input_fwd(1, 8, None, 0, seg, 1, None, 0, 1, 32, 32, 1, None, 0, None)
    assert rc == -1 and b"leaves its rows" in lib.ali_last_error()
