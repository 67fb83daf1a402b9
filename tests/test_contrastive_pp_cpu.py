"""Pertinent positives of the contrastive family without a GPU: ``ali_hip.contrast.cem_pp_statement`` and its pieces
(``attack_pp_statement``, ``pp_update_statement``) on a linear "classifier" in fp64, where one iteration can be written
out pixel by pixel; the hinge at zero margin, at ties and the sign of its seed; the shrink around the background at
exactly b +- beta; the box [min(b, x0), max(b, x0)] with x0 above, below and at b, for the iterate and the momentum
step; a whole search against the brute-force best of its recorded trajectory; the refusals; ``ContrastiveExplainer``
with ``positives=True``; a random-weight ``MNISTClassifier`` on the CPU; and the seed check the device tests rely on."""
import math

import numpy as np
import pytest
import torch

F64 = torch.float64


def _linear(N, C=2, seed=0, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(C, N, generator=g, dtype=dtype)
    b = torch.randn(C, generator=g, dtype=dtype)
    return W, b, (lambda x: x.reshape(x.shape[0], -1) @ W.T + b)


def _pixel_pp_gradient(W, b, point, t0, c, kappa):
    """c * dApos(f(point))/dpoint of the linear classifier, row by row and class by class"""
    out = []
    for r in range(point.shape[0]):
        s = [sum(W[j, i].item() * point[r, i].item() for i in range(point.shape[1])) + b[j].item()
             for j in range(W.shape[0])]
        t = int(t0[r])
        other = max((j for j in range(len(s)) if j != t), key=lambda j: (s[j], -j))
        active = s[other] - s[t] + kappa > 0
        out.append([c[r].item() * (W[other, i].item() - W[t, i].item()) if active else 0.0
                    for i in range(point.shape[1])])
    return out


def _box(x, bg):
    return min(bg, x), max(bg, x)


def _clamp(w, lo, hi):
    return lo if w < lo else (hi if w > hi else w)


# ------------------------------------------------------------------------------------------------ the hinge
def test_hinge_at_zero_margin_at_ties_and_the_sign_of_the_seed():
    from ali_hip.contrast import attack_pp_statement
    t = lambda *v: torch.tensor(v, dtype=F64)  # noqa: E731
    kappa = 0.5
    s = torch.stack([t(1.0, 0.5, 0.0, -2.0),        # other - own + kappa = 0.5 - 1 + 0.5 = 0 exactly: off
                     t(1.0, 1.25, 0.0, 1.25),       # tie of the others (columns 1 and 3): the first, column 1
                     t(-1.0, 3.0, 3.0, 3.0),        # own is column 2 of a three-way tie: other is column 1
                     t(5.0, 0.0, 0.0, 0.0)])        # own far above: off
    t0 = torch.tensor([0, 0, 2, 0])
    c = t(2.0, 3.0, 4.0, 5.0)
    A, seed, other = attack_pp_statement(s, t0, c, kappa)
    assert other.tolist() == [1, 1, 1, 1]
    assert torch.equal(A, t(0.0, 0.75, 0.5, 0.0))
    assert not seed[0].any() and not seed[3].any()                              # the hinge is off: no seed at all
    assert torch.equal(seed[1], t(-3.0, 3.0, 0.0, 0.0))                         # +c on other, -c on t0
    assert torch.equal(seed[2], t(0.0, 4.0, -4.0, 0.0))


def test_class_gradient_of_the_pp_hinge_matches_a_pixel_loop():
    from ali_hip.contrast import attack_pp_statement, class_gradient
    B, N = 3, 7
    W, b, f = _linear(N, C=3, seed=21)
    g = torch.Generator().manual_seed(22)
    point = torch.rand(B, N, generator=g, dtype=F64) * 2 - 1
    t0 = torch.tensor([0, 1, 2])
    c = torch.tensor([10.0, 0.5, 3.0], dtype=F64)
    kappa = 2.0
    got = class_gradient(f, point, t0, c, kappa, attack_pp_statement)
    want = torch.tensor(_pixel_pp_gradient(W, b, point, t0, c, kappa), dtype=F64)
    assert want.abs().sum() > 0
    assert (got - want).abs().max().item() <= 1e-13


# ------------------------------------------------------------------------------------------------ one iteration
@pytest.mark.parametrize("bg", [0.0, -1.0])
def test_one_pp_iteration_matches_a_pixel_loop(bg):
    from ali_hip.contrast import attack_pp_statement, class_gradient, pp_update_statement
    B, N, K, k = 3, 9, 5, 2
    lr, beta, clip, kappa = 0.3, 0.05, 1e3, 0.5
    W, b, f = _linear(N, C=3, seed=1)
    g = torch.Generator().manual_seed(2)
    x0 = torch.rand(B, N, generator=g, dtype=F64) * 2 - 1
    x0[:, 0] = bg                                                                # x0 == b: the box is one point
    frac = lambda: torch.rand(B, N, generator=g, dtype=F64) * (torch.rand(B, N, generator=g) > 0.3)  # noqa: E731
    v, y = bg + frac() * (x0 - bg), bg + frac() * (x0 - bg)                      # inside the box
    t0 = f(x0).argmax(1)
    c = torch.tensor([10.0, 0.5, 3.0], dtype=F64)
    gcls = class_gradient(f, y, t0, c, kappa, attack_pp_statement)
    vn, yn, l1, l2, norm = pp_update_statement(v, y, x0, gcls, k, K, lr, beta, clip, bg)
    ga = _pixel_pp_gradient(W, b, y, t0, c, kappa)
    assert any(any(row) for row in ga)                                          # the hinge is active somewhere
    for r in range(B):
        gr = [ga[r][i] + 2 * (y[r, i].item() - bg) for i in range(N)]
        nrm = math.sqrt(sum(a * a for a in gr))
        assert abs(nrm - norm[r].item()) <= 1e-12 * nrm
        s1 = s2 = 0.0
        for i in range(N):
            lo, hi = _box(x0[r, i].item(), bg)
            u = y[r, i].item() - lr * math.sqrt(1 - k / K) * gr[i]
            d = u - bg
            w = u - beta if d > beta else (u + beta if d < -beta else bg)
            nv = _clamp(w, lo, hi)
            ny = _clamp(nv + k / (k + 3) * (nv - v[r, i].item()), lo, hi)
            assert abs(nv - vn[r, i].item()) <= 1e-13 and abs(ny - yn[r, i].item()) <= 1e-13, (r, i)
            s1, s2 = s1 + abs(nv - bg), s2 + (nv - bg) ** 2
        assert abs(s1 - l1[r].item()) <= 1e-12 and abs(s2 - l2[r].item()) <= 1e-12
    assert (vn == bg).any() and (vn != bg).any()
    assert (vn[:, 0] == bg).all() and (yn[:, 0] == bg).all()


# ------------------------------------------------------------------------------------------------ the operators
def _pp_from_u(x0, u, beta, bg, v=None, k=0, K=4):
    """the update with y = b, lr = 1 and k = 0 (unless given), so that u = b - gcls exactly: gcls = b - u"""
    from ali_hip.contrast import pp_update_statement
    y = torch.full_like(x0, bg)
    v = y if v is None else v
    return pp_update_statement(v, y, x0, bg - u, k, K, 1.0, beta, 1e30, bg)


@pytest.mark.parametrize("bg", [0.0, -1.0])
def test_shrink_at_b_plus_minus_beta_and_both_ends_of_the_box(bg):
    beta = 0.25
    #                 d = beta   just above  -beta     just below  far above  far below  x0 == b   inside
    x0 = bg + torch.tensor([[1.0, 1.0, -1.0, -1.0, 0.5, -0.5, 0.0, 1.0]], dtype=F64)
    d = torch.tensor([[0.25, 0.375, -0.25, -0.375, 4.0, -4.0, 2.0, 0.75]], dtype=F64)
    vn, yn, l1, l2, _ = _pp_from_u(x0, bg + d, beta, bg)
    # w: b at |d| <= beta, u -+ beta beyond it; then the box: above b for x0 > b, below b for x0 < b, b for x0 == b
    want = bg + torch.tensor([[0.0, 0.125, 0.0, -0.125, 0.5, -0.5, 0.0, 0.5]], dtype=F64)
    assert torch.equal(vn, want)
    assert torch.equal(yn, vn)                                                   # k = 0: no momentum
    assert l1.item() == 0.125 + 0.125 + 0.5 + 0.5 + 0.5
    assert l2.item() == 2 * 0.125 ** 2 + 3 * 0.5 ** 2
    # the wrong side of b: x0 above b and a step below it (and the mirror) end at b, the box's other end
    x0 = bg + torch.tensor([[0.5, -0.5]], dtype=F64)
    vn, _, _, _, _ = _pp_from_u(x0, bg + torch.tensor([[-2.0, 2.0]], dtype=F64), beta, bg)
    assert torch.equal(vn, torch.full_like(x0, bg))


@pytest.mark.parametrize("bg", [0.0, -1.0])
def test_the_momentum_step_is_clamped_to_the_box(bg):
    beta = 0.25
    x0 = bg + torch.tensor([[1.0, 1.0, -1.0, 1.0, 0.0]], dtype=F64)
    v = bg + torch.tensor([[0.0, 0.9, -0.9, 0.2, 0.0]], dtype=F64)
    d = torch.tensor([[0.75, 0.75, -0.75, 0.25, 1.0]], dtype=F64)
    vn, yn, _, _, _ = _pp_from_u(x0, bg + d, beta, bg, v=v, k=3, K=1e30)
    assert torch.equal(vn, bg + torch.tensor([[0.5, 0.5, -0.5, 0.0, 0.0]], dtype=F64))
    # y' = v' + 3/6 (v' - v): 0.75; 0.5 - 0.2 = 0.3; -0.5 + 0.2 = -0.3; 0 - 0.1 = -0.1 -> b (below b for x0 > b); b
    want = bg + torch.tensor([[0.75, 0.3, -0.3, 0.0, 0.0]], dtype=F64)
    assert (yn - want).abs().max().item() <= 1e-15
    assert yn[0, 3].item() == bg and yn[0, 4].item() == bg
    # and the other end: far beyond x0 the slack stops at x0 itself
    v = bg + torch.tensor([[-4.0, 0.0, 0.0, 0.0, 0.0]], dtype=F64)
    vn, yn, _, _, _ = _pp_from_u(x0, bg + d, beta, bg, v=v, k=3, K=1e30)
    assert yn[0, 0].item() == x0[0, 0].item()


# ------------------------------------------------------------------------------------------------ whole searches
def _search_case():
    N, B = 12, 4
    W, b, f = _linear(N, C=3, seed=11)
    g = torch.Generator().manual_seed(12)
    x = torch.rand(B, 1, 3, 4, generator=g, dtype=F64) * 2 - 1
    hyper = dict(num_iterations=4, binary_search_steps=2, kappa=0.1, c0=1.0, learning_rate=0.2)
    return f, x, hyper


@pytest.mark.parametrize("bg", [0.0, -1.0])
def test_the_best_is_the_smallest_distance_success_of_the_trajectory(bg):
    from ali_hip.contrast import cem_pp_statement
    f, x, hyper = _search_case()
    rec = []
    out = cem_pp_statement(f, x, background=bg, record=rec, **hyper)
    B = x.shape[0]
    assert len(rec) == 8 and [(e["round"], e["k"]) for e in rec] == [(r, k) for r in range(2) for k in range(4)]
    t0 = f(x).argmax(1)
    x0 = x.reshape(B, -1)
    beta = 0.1
    n_found = n_nontrivial = 0
    for r in range(B):
        cands = []
        for e in rec:
            v = e["v"][r]
            assert torch.equal(f(v.reshape(1, -1)).argmax(1)[0], e["pred"][r])
            d = (v - bg).pow(2).sum() + beta * (v - bg).abs().sum()
            assert abs(d.item() - e["dist"][r].item()) <= 1e-12
            assert bool(e["succ"][r]) == bool(e["pred"][r] == t0[r])
            if e["pred"][r] == t0[r]:
                cands.append((e["dist"][r].item(), len(cands), e))
        if not cands:
            assert out["found"][r] == 0 and torch.equal(out["image"][r].reshape(-1), x0[r])
            assert out["label"][r] == t0[r] and out["dist"][r] == 0
            continue
        n_found += 1
        _, _, e = min(cands, key=lambda c: (c[0], c[1]))                      # the first of equal distances
        assert out["found"][r] == 1
        assert torch.equal(out["image"][r].reshape(-1), e["v"][r])
        assert out["label"][r] == t0[r]
        assert out["dist"][r].item() == e["dist"][r].item()
        n_nontrivial += int(out["dist"][r] > 0)
    assert n_found > 0 and n_nontrivial > 0
    succ0 = torch.stack([e["succ"] for e in rec[:4]]).any(dim=0)
    assert torch.equal(rec[4]["c"], torch.where(succ0, torch.tensor(0.5, dtype=F64), torch.tensor(10.0, dtype=F64)))
    lo, hi = torch.minimum(x0, torch.full_like(x0, bg)), torch.maximum(x0, torch.full_like(x0, bg))
    assert all(((e["v"] >= lo) & (e["v"] <= hi)).all() for e in rec)


def test_unfound_rows_return_x0_bit_for_bit():
    from ali_hip.contrast import cem_pp_statement
    # a background the classifier labels otherwise than every row, and an attack too weak to move off it
    f = lambda x: torch.stack([x.reshape(x.shape[0], -1).sum(1), torch.zeros(x.shape[0], dtype=x.dtype)], 1)  # noqa
    x = torch.rand(3, 1, 3, 4, generator=torch.Generator().manual_seed(4), dtype=F64) + 0.5      # class 0
    out = cem_pp_statement(f, x, background=-1.0, num_iterations=4, binary_search_steps=1, kappa=0.1, c0=1e-9)
    assert not out["found"].any() and out["found"].dtype == torch.int32
    assert torch.equal(out["image"], x) and out["image"].shape == x.shape
    assert out["label"].tolist() == [0, 0, 0] and out["label"].dtype == torch.int32
    assert not out["dist"].any()
    assert torch.equal(out["c"], torch.full((3,), 1e-8, dtype=F64))            # one failed round: c * 10


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from ali_hip.contrast import ContrastiveSearch, cem_pp_statement, hyper_parameters
    from classifiers._stack import ClassifierStack
    nn = torch.nn
    plain = ClassifierStack(nn.Conv2d(1, 4, 3), nn.LeakyReLU(0.2), nn.Flatten(), nn.Linear(16, 2)).eval()
    with pytest.raises(ValueError, match="bounds"):
        ContrastiveSearch(plain, "pp", bounds=(-1.0, 1.0))
    for mode in ("pn", "ce"):
        with pytest.raises(ValueError, match="background"):
            ContrastiveSearch(plain, mode, background=0.0)
    assert ContrastiveSearch(plain, "pp").background == 0.0
    assert ContrastiveSearch(plain, "pp", background=0.1).background == float(np.float32(0.1))
    bn = ClassifierStack(nn.Conv2d(1, 4, 3), nn.BatchNorm2d(4), nn.LeakyReLU(0.2), nn.Flatten(), nn.Linear(16, 2)).eval()
    with pytest.raises(ValueError, match="BatchNorm"):
        ContrastiveSearch(bn, "pp")
    with pytest.raises(ValueError):
        hyper_parameters("pp", {})
    with pytest.raises(TypeError):
        cem_pp_statement(lambda x: x, torch.zeros(1, 2), gamma=1.0)               # gamma belongs to "ce"
    assert ContrastiveSearch(plain, "pp").hp == hyper_parameters("pn", {})       # pn's defaults


# ------------------------------------------------------------------------------------------------ the shim
class _Wrapper:
    """a callable "model" that is no module: the statement's route"""

    def __init__(self, f):
        self.f = f

    def __call__(self, x):
        assert x.shape[1:] == (1, 3, 4)
        return self.f(x)


def test_shim_with_positives_keys_pn_part_and_rows():
    from explain.contrastive import ContrastiveExplainer, Image
    _, _, f = _linear(12, C=3, seed=11, dtype=torch.float32)
    g = torch.Generator().manual_seed(13)
    x_test = (torch.rand(5, 3, 4, 1, generator=g) * 2 - 1).numpy()
    hyper = dict(num_iterations=4, binary_search_steps=2, kappa=0.1, c0=1.0, learning_rate=0.2)
    pre = lambda x_: x_.data.reshape((-1, 1, 3, 4))  # noqa: E731
    ex = ContrastiveExplainer(_Wrapper(f), preprocess_function=pre, positives=True, background=-1.0, **hyper)
    plain = ContrastiveExplainer(_Wrapper(f), preprocess_function=pre, **hyper)
    rows = []
    for i in range(5):
        img = Image(x_test[i].reshape((1, 3, 4, 1)), batched=True)
        e = ex.explain(img).explanations[0]
        assert set(e) == {"pn", "pn_label", "found", "pp", "pp_label", "pp_found"}
        assert e["pp"].shape == (3, 4, 1) and e["pp"].dtype == np.float32
        p = plain.explain(img).explanations[0]
        assert set(p) == {"pn", "pn_label", "found"}
        assert np.array_equal(e["pn"], p["pn"]) and e["pn_label"] == p["pn_label"] and e["found"] == p["found"]
        lo, hi = np.minimum(x_test[i], -1.0), np.maximum(x_test[i], -1.0)
        assert ((e["pp"] >= lo) & (e["pp"] <= hi)).all()
        rows.append(e)
    every = ex.explain_all(x_test, batch=2)
    assert set(every) == {"pn", "pn_label", "found", "pp", "pp_label", "pp_found"}
    for i, e in enumerate(rows):                                                 # rows of a batch are independent
        for k in ("pn", "pp"):
            assert np.array_equal(every[k][i], e[k]) and every[k + "_label"][i] == e[k + "_label"]
        assert every["found"][i] == e["found"] and every["pp_found"][i] == e["pp_found"]
    assert every["pp_found"].any()
    assert set(plain.explain_all(x_test, batch=2)) == {"pn", "pn_label", "found"}


def test_a_random_weight_mnist_classifier_runs_the_pp_statement_on_the_cpu():
    from classifiers.mnist import MNISTClassifier
    from explain.contrastive import ContrastiveExplainer, Image
    torch.manual_seed(0)
    clf = MNISTClassifier().eval()
    x = (torch.rand(2, 28, 28, 1, generator=torch.Generator().manual_seed(1)) * 2 - 1).numpy()
    pre = lambda x_: x_.data.reshape((-1, 1, 28, 28))  # noqa: E731
    before = [p.clone() for p in clf.parameters()]
    ex = ContrastiveExplainer(clf, preprocess_function=pre, positives=True, background=0.0, num_iterations=3,
                              binary_search_steps=2, kappa=0.0, c0=1e4, learning_rate=0.1)
    assert not ex.on_device
    res = ex.explain(Image(x, batched=True)).explanations
    with torch.no_grad():
        t0 = clf(torch.from_numpy(x).reshape(-1, 1, 28, 28)).argmax(1)
    for i, e in enumerate(res):
        assert e["pp"].shape == (28, 28, 1)
        with torch.no_grad():
            label = clf(torch.from_numpy(e["pp"]).reshape(1, 1, 28, 28)).argmax(1).item()
        assert e["pp_label"] == t0[i].item()
        if e["pp_found"]:
            assert label == t0[i].item()
            assert ((e["pp"] >= np.minimum(x[i], 0)) & (e["pp"] <= np.maximum(x[i], 0))).all()
        else:
            assert np.array_equal(e["pp"], x[i])
    assert all(torch.equal(a, b) for a, b in zip(before, clf.parameters()))
    assert all(p.grad is None for p in clf.parameters())


# ------------------------------------------------------------------------------------------------ the seed check
HYPER = dict(num_iterations=3, binary_search_steps=2, kappa=0.0, c0=1e4, learning_rate=0.1)
UNFOUND = dict(num_iterations=3, binary_search_steps=1, kappa=0.0, c0=1e-6)


@pytest.mark.parametrize("bg", [0.0, -1.0])
def test_cpu_fp32_statement_finds_and_misses_on_the_chosen_seeds(bg):
    """the classifier, images and hyper-parameters of test_gpu_contrastive_pp.py: HYPER finds every row, one at a
    nonzero distance; UNFOUND leaves a row unfound"""
    from ali_hip.contrast import cem_pp_statement
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(0)
    clf = MNISTClassifier().eval()
    x = torch.rand(3, 1, 28, 28, generator=torch.Generator().manual_seed(1)) * 2 - 1
    out = cem_pp_statement(clf, x, background=bg, **HYPER)
    assert out["found"].all() and (out["dist"] > 0).any()
    assert not cem_pp_statement(clf, x, background=bg, **UNFOUND)["found"].all()
