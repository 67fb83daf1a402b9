"""The contrastive family without a GPU: the torch statements of ``ali_hip.contrast`` (pertinent negatives of the
contrastive explanation method; the counterfactual search) on a linear two-class "classifier", where one iteration can
be written out pixel by pixel; the shrink operator at its thresholds and clamps, both projections, sign(0), the norm
clip, the binary-search table; what a search returns with and without a success (brute force over a recorded
trajectory); the drop-in surface of ``explain/contrastive.py``; and a random-weight ``MNISTClassifier`` on the CPU."""
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


def _row_state(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, N, generator=g, dtype=F64) * 2 - 1
    v = x0 + torch.rand(B, N, generator=g, dtype=F64) * 0.3 * (torch.rand(B, N, generator=g) > 0.4)
    y = x0 + torch.rand(B, N, generator=g, dtype=F64) * 0.3 * (torch.rand(B, N, generator=g) > 0.4)
    return x0, v, y


def _pixel_attack_gradient(W, b, point, t0, c, kappa):
    """c * dA(f(point))/dpoint of the linear classifier, row by row and class by class"""
    out = []
    for r in range(point.shape[0]):
        s = [sum(W[j, i].item() * point[r, i].item() for i in range(point.shape[1])) + b[j].item()
             for j in range(W.shape[0])]
        t = int(t0[r])
        other = max((j for j in range(len(s)) if j != t), key=lambda j: (s[j], -j))
        active = s[t] - s[other] + kappa > 0
        out.append([c[r].item() * (W[t, i].item() - W[other, i].item()) if active else 0.0
                    for i in range(point.shape[1])])
    return out


# ------------------------------------------------------------------------------------------------ one iteration
def test_one_cem_iteration_matches_a_pixel_loop():
    from ali_hip.contrast import cem_update_statement, class_gradient
    B, N, K, k = 3, 7, 5, 2
    lr, beta, clip, kappa = 0.3, 0.05, 1e3, 0.5
    W, b, f = _linear(N, seed=1)
    x0, v, y = _row_state(B, N, 2)
    t0 = f(x0).argmax(1)
    c = torch.tensor([10.0, 0.5, 3.0], dtype=F64)
    lo, hi = x0.amin(1), x0.amax(1)
    gcls = class_gradient(f, y, t0, c, kappa)
    vn, yn, l1, l2, norm = cem_update_statement(v, y, x0, gcls, k, K, lr, beta, clip, lo, hi)
    ga = _pixel_attack_gradient(W, b, y, t0, c, kappa)
    assert any(any(row) for row in ga)                                          # the hinge is active somewhere
    for r in range(B):
        g = [ga[r][i] + 2 * (y[r, i].item() - x0[r, i].item()) for i in range(N)]
        nrm = math.sqrt(sum(a * a for a in g))
        assert abs(nrm - norm[r].item()) <= 1e-12 * nrm
        s1 = s2 = 0.0
        for i in range(N):
            x = x0[r, i].item()
            u = y[r, i].item() - lr * math.sqrt(1 - k / K) * g[i]
            d = u - x
            w = min(u - beta, hi[r].item()) if d > beta else (max(u + beta, lo[r].item()) if d < -beta else x)
            nv = w if w > x else x
            ny = nv + k / (k + 3) * (nv - v[r, i].item())
            ny = ny if ny > x else x
            assert abs(nv - vn[r, i].item()) <= 1e-13 and abs(ny - yn[r, i].item()) <= 1e-13, (r, i)
            s1, s2 = s1 + abs(nv - x), s2 + (nv - x) ** 2
        assert abs(s1 - l1[r].item()) <= 1e-12 and abs(s2 - l2[r].item()) <= 1e-12
    assert (vn > x0).any() and (vn == x0).any()


def test_one_ce_iteration_matches_a_pixel_loop():
    from ali_hip.contrast import ce_update_statement, class_gradient
    B, N, t = 3, 7, 3
    lr, gamma, clip, kappa = 0.05, 1.0, 1e3, 0.5
    W, b, f = _linear(N, seed=4)
    x0, v, _ = _row_state(B, N, 5)
    v = v - 0.1
    v[:, 0] = x0[:, 0]                                                           # sign(0) pixels
    g0 = torch.Generator().manual_seed(6)
    m, v2 = torch.randn(B, N, generator=g0, dtype=F64) * 0.1, torch.rand(B, N, generator=g0, dtype=F64) * 0.01
    t0 = f(x0).argmax(1)
    c = torch.tensor([10.0, 0.5, 3.0], dtype=F64)
    lo, hi = x0.amin(1), x0.amax(1)
    gcls = class_gradient(f, v, t0, c, kappa)
    vn, mn, v2n, l1, norm = ce_update_statement(v, x0, gcls, m, v2, t, lr, gamma, clip, lo, hi)
    ga = _pixel_attack_gradient(W, b, v, t0, c, kappa)
    clamped = 0
    for r in range(B):
        sgn = [(v[r, i] > x0[r, i]).item() - (v[r, i] < x0[r, i]).item() for i in range(N)]
        assert sgn[0] == 0
        g = [ga[r][i] + gamma * sgn[i] for i in range(N)]
        assert abs(math.sqrt(sum(a * a for a in g)) - norm[r].item()) <= 1e-12 * norm[r].item()
        s1 = 0.0
        for i in range(N):
            m1 = 0.9 * m[r, i].item() + 0.1 * g[i]
            s = 0.999 * v2[r, i].item() + 0.001 * g[i] * g[i]
            nv = v[r, i].item() - lr / (1 - 0.9 ** t) * m1 / (math.sqrt(s) / math.sqrt(1 - 0.999 ** t) + 1e-8)
            cl = min(max(nv, lo[r].item()), hi[r].item())
            clamped += cl != nv
            assert abs(m1 - mn[r, i].item()) <= 1e-14 and abs(s - v2n[r, i].item()) <= 1e-14
            assert abs(cl - vn[r, i].item()) <= 1e-13, (r, i)
            s1 += abs(cl - x0[r, i].item())
        assert abs(s1 - l1[r].item()) <= 1e-12
    assert clamped > 0


# ------------------------------------------------------------------------------------------------ the operators
def _cem_from_u(x0, u, beta, lo, hi, v=None, k=0, K=4):
    """the update with y = x0, lr = 1 and k = 0 (unless given), so that u = x0 - gcls exactly: gcls = x0 - u"""
    from ali_hip.contrast import cem_update_statement
    v = x0 if v is None else v
    return cem_update_statement(v, x0.clone(), x0, x0 - u, k, K, 1.0, beta, 1e30, lo, hi)


def test_shrink_at_its_thresholds_and_on_both_clamps():
    beta = 0.25
    x0 = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, -0.5]], dtype=F64)
    #                   d = beta, just above, -beta, just below, far above (hi clamp), far below (lo clamp), inside, inside
    u = torch.tensor([[0.25, 0.375, -0.25, -0.375, 4.0, -4.0, 0.625, -0.5]], dtype=F64)
    lo, hi = torch.tensor([-0.5], dtype=F64), torch.tensor([0.5], dtype=F64)
    vn, yn, l1, l2, _ = _cem_from_u(x0, u, beta, lo, hi)
    # the shrink alone: d = +-beta falls to x0, beyond it moves by beta, far beyond it stops at hi / lo; then the
    # "only additions" projection puts every w <= x0 back to x0
    want_w = torch.tensor([[0.0, 0.125, 0.0, -0.125, 0.5, -0.5, 0.5, -0.5]], dtype=F64)
    want_v = torch.where(want_w > x0, want_w, x0)
    assert torch.equal(vn, want_v)
    assert torch.equal(vn, torch.tensor([[0.0, 0.125, 0.0, 0.0, 0.5, 0.0, 0.5, -0.5]], dtype=F64))
    assert torch.equal(yn, vn)                                                   # k = 0: no momentum
    assert l1.item() == 0.625 and l2.item() == 0.125 ** 2 + 0.5 ** 2


def test_both_projections():
    beta = 0.25
    x0 = torch.zeros(1, 4, dtype=F64)
    lo, hi = torch.tensor([-1.0], dtype=F64), torch.tensor([1.0], dtype=F64)
    u = torch.tensor([[0.75, -0.75, 0.75, 0.1]], dtype=F64)
    v = torch.tensor([[0.0, 0.0, 2.5, 0.0]], dtype=F64)                        # pixel 2: the momentum points below x0
    vn, yn, _, _, _ = _cem_from_u(x0, u, beta, lo, hi, v=v, k=3, K=1e30)
    assert torch.equal(vn, torch.tensor([[0.5, 0.0, 0.5, 0.0]], dtype=F64))     # w = -0.5 < x0 -> x0
    # y' = v' + 3/6 (v' - v): 0.75, 0, 0.5 - 1 = -0.5 -> x0, 0
    assert torch.equal(yn, torch.tensor([[0.75, 0.0, 0.0, 0.0]], dtype=F64))


def test_sign_of_zero_is_zero():
    from ali_hip.contrast import ce_update_statement
    x0 = torch.tensor([[0.5, -0.25, 0.0]], dtype=F64)
    z = torch.zeros_like(x0)
    lo, hi = torch.tensor([-1.0], dtype=F64), torch.tensor([1.0], dtype=F64)
    vn, m, v2, l1, norm = ce_update_statement(x0.clone(), x0, z, z, z, 1, 0.1, 1.0, 1e3, lo, hi)
    assert torch.equal(vn, x0) and not m.any() and not v2.any() and l1.item() == 0 and norm.item() == 0
    v = x0 + torch.tensor([[0.1, 0.0, -0.1]], dtype=F64)
    vn, m, _, _, norm = ce_update_statement(v, x0, z, z, z, 1, 0.1, 1.0, 1e3, lo, hi)
    assert torch.equal(m.sign(), torch.tensor([[1.0, 0.0, -1.0]], dtype=F64)) and abs(norm.item() - math.sqrt(2.0)) <= 1e-15
    assert vn[0, 1].item() == x0[0, 1].item() and vn[0, 0] < v[0, 0] and vn[0, 2] > v[0, 2]


def test_norm_clip_on_and_off():
    from ali_hip.contrast import clip_statement
    g = torch.tensor([[3.0, 4.0], [0.3, 0.4], [6.0, 8.0]], dtype=F64)
    out, norm = clip_statement(g, 5.0)
    assert torch.equal(norm, torch.tensor([5.0, 0.5, 10.0], dtype=F64))
    assert torch.equal(out[:2], g[:2])                                           # at the bound and below: untouched
    assert torch.equal(out[2], torch.tensor([3.0, 4.0], dtype=F64))
    assert torch.equal(clip_statement(g, 1e3)[0], g)


def test_binary_search_table():
    from ali_hip.contrast import c_table_statement
    t = lambda *v: torch.tensor(v, dtype=F64)  # noqa: E731
    #            success            failure, c_hi open   failure after a success   success above c_hi   failure below c_lo
    c, c_lo, c_hi = t(10, 10, 5, 8, 1), t(0, 0, 0, 0, 2), t(1e10, 1e10, 10, 6, 10)
    ok = torch.tensor([True, False, False, True, False])
    c2, lo2, hi2 = c_table_statement(c, c_lo, c_hi, ok)
    assert torch.equal(c2, t(5, 100, 7.5, 3, 6))
    assert torch.equal(lo2, t(0, 10, 5, 0, 2))
    assert torch.equal(hi2, t(10, 1e10, 10, 6, 10))
    # five failing rounds from the defaults: c grows tenfold each time
    c, c_lo, c_hi = t(10), t(0), t(1e10)
    for _ in range(5):
        c, c_lo, c_hi = c_table_statement(c, c_lo, c_hi, torch.tensor([False]))
    assert c.item() == 1e6 and c_lo.item() == 1e5 and c_hi.item() == 1e10


# ------------------------------------------------------------------------------------------------ whole searches
def _search_case(mode):
    from ali_hip.contrast import ce_statement, cem_pn_statement
    N, B = 12, 4
    W, b, f = _linear(N, C=3, seed=11)
    g = torch.Generator().manual_seed(12)
    x = torch.rand(B, 1, 3, 4, generator=g, dtype=F64) * 2 - 1
    hyper = dict(num_iterations=4, binary_search_steps=2, kappa=0.1, c0=1.0, learning_rate=0.2)
    return f, x, (cem_pn_statement if mode == "pn" else ce_statement), hyper


@pytest.mark.parametrize("mode", ["pn", "ce"])
def test_unfound_rows_return_x0_bit_for_bit(mode):
    f, x, statement, hyper = _search_case(mode)
    out = statement(f, x, **dict(hyper, c0=1e-9, binary_search_steps=1))
    assert not out["found"].any() and out["found"].dtype == torch.int32
    assert torch.equal(out["image"], x) and out["image"].shape == x.shape
    assert torch.equal(out["label"].long(), f(x).argmax(1)) and out["label"].dtype == torch.int32
    assert not out["dist"].any()
    assert torch.equal(out["c"], torch.full((x.shape[0],), 1e-8, dtype=F64))   # one failed round: c * 10


@pytest.mark.parametrize("mode", ["pn", "ce"])
def test_the_best_is_the_smallest_distance_success_of_the_trajectory(mode):
    f, x, statement, hyper = _search_case(mode)
    rec = []
    out = statement(f, x, record=rec, **hyper)
    B = x.shape[0]
    assert len(rec) == 8 and [(e["round"], e["k"]) for e in rec] == [(r, k) for r in range(2) for k in range(4)]
    t0 = f(x).argmax(1)
    x0 = x.reshape(B, -1)
    beta = 0.1
    n_found = 0
    for r in range(B):
        cands = []
        for e in rec:
            v = e["v"][r]
            assert torch.equal(f(v.reshape(1, -1)).argmax(1)[0], e["pred"][r])
            d = (v - x0[r]).abs().sum()
            if mode == "pn":
                d = (v - x0[r]).pow(2).sum() + beta * d
            assert abs(d.item() - e["dist"][r].item()) <= 1e-12
            if e["pred"][r] != t0[r]:
                cands.append((e["dist"][r].item(), len(cands), e))
        if not cands:
            assert out["found"][r] == 0 and torch.equal(out["image"][r].reshape(-1), x0[r])
            continue
        n_found += 1
        _, _, e = min(cands, key=lambda c: (c[0], c[1]))                      # the first of equal distances
        assert out["found"][r] == 1
        assert torch.equal(out["image"][r].reshape(-1), e["v"][r])
        assert out["label"][r] == e["pred"][r] and out["label"][r] != t0[r]
        assert out["dist"][r].item() == e["dist"][r].item()
    assert 0 < n_found                                                           # the case has successes to choose from
    # the c of round 1 follows the table from round 0's successes
    succ0 = torch.stack([e["succ"] for e in rec[:4]]).any(dim=0)
    assert torch.equal(rec[4]["c"], torch.where(succ0, torch.tensor(0.5, dtype=F64), torch.tensor(10.0, dtype=F64)))
    if mode == "pn":
        assert all((e["v"] >= x0).all() for e in rec)
    lo, hi = x0.amin(1, keepdim=True), x0.amax(1, keepdim=True)
    assert all(((e["v"] >= lo) & (e["v"] <= hi)).all() for e in rec)


def test_unknown_hyper_parameters_and_modes_are_refused():
    from ali_hip.contrast import ContrastiveSearch, cem_pn_statement, hyper_parameters
    with pytest.raises(TypeError):
        cem_pn_statement(lambda x: x, torch.zeros(1, 2), gamma=1.0)               # gamma belongs to "ce"
    with pytest.raises(ValueError):
        hyper_parameters("pp", {})
    assert hyper_parameters("pn", {})["num_iterations"] == 1000 and hyper_parameters("ce", {})["num_iterations"] == 100
    with pytest.raises(TypeError):
        ContrastiveSearch(torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(4, 2)))


def test_the_executor_refuses_batchnorm_in_pn_and_training_mode_when_it_is_built():
    from ali_hip.contrast import ContrastiveSearch
    from classifiers._stack import ClassifierStack
    nn = torch.nn
    bn = ClassifierStack(nn.Conv2d(1, 4, 3), nn.BatchNorm2d(4), nn.LeakyReLU(0.2), nn.Flatten(), nn.Linear(16, 2)).eval()
    with pytest.raises(ValueError, match="BatchNorm"):
        ContrastiveSearch(bn, "pn")
    ContrastiveSearch(bn, "ce")                                                  # one pass of B rows: no rows are cut out
    with pytest.raises(ValueError, match="eval"):
        ContrastiveSearch(bn.train(), "ce")


# ------------------------------------------------------------------------------------------------ the shim
class _Wrapper:
    """a callable "model" that is no module: the statement's route"""

    def __init__(self, f):
        self.f = f

    def __call__(self, x):
        assert x.shape[1:] == (1, 3, 4)
        return self.f(x)


def test_shim_shapes_keys_and_row_order():
    from explain.contrastive import ContrastiveExplainer, CounterfactualExplainer, Image
    _, _, f = _linear(12, C=3, seed=11, dtype=torch.float32)
    g = torch.Generator().manual_seed(13)
    x_test = (torch.rand(5, 3, 4, 1, generator=g) * 2 - 1).numpy()
    hyper = dict(num_iterations=4, binary_search_steps=2, kappa=0.1, c0=1.0, learning_rate=0.2)
    pre = lambda x_: x_.data.reshape((-1, 1, 3, 4))  # noqa: E731
    for cls, key in ((ContrastiveExplainer, "pn"), (CounterfactualExplainer, "cf")):
        ex = cls(_Wrapper(f), preprocess_function=pre, **hyper)
        rows = []
        for i in range(5):                                                       # the scripts' call pattern
            res = ex.explain(Image(x_test[i].reshape((1, 3, 4, 1)), batched=True))
            e = res.explanations[0]
            assert set(e) == {key, key + "_label", "found"} and len(res.explanations) == 1
            assert isinstance(e[key], np.ndarray) and e[key].shape == (3, 4, 1) and e[key].dtype == np.float32
            e[key].reshape((1, 1, 3, 4))
            rows.append(e)
        every = ex.explain_all(x_test, batch=2)
        assert every[key].shape == x_test.shape and every["found"].shape == (5,)
        for i, e in enumerate(rows):                                             # rows of a batch are independent searches
            assert np.array_equal(every[key][i], e[key]) and every[key + "_label"][i] == e[key + "_label"]
            assert every["found"][i] == e["found"]
        assert every["found"].any()
        unbatched = ex.explain(Image(x_test[0])).explanations
        assert len(unbatched) == 1 and np.array_equal(unbatched[0][key], rows[0][key])


def test_shim_refuses_a_preprocess_function_that_is_no_reshape():
    from explain.contrastive import ContrastiveExplainer, Image
    _, _, f = _linear(12, C=3, seed=11, dtype=torch.float32)
    img = Image(np.zeros((1, 3, 4, 1), dtype=np.float32), batched=True)
    for bad in (lambda x_: x_.data.transpose(0, 2, 1, 3).reshape((-1, 1, 3, 4)),      # reorders
                lambda x_: x_.data[:, :2],                                             # drops elements
                lambda x_: 2 * x_.data):                                               # rescales
        with pytest.raises(ValueError):
            ContrastiveExplainer(_Wrapper(f), preprocess_function=bad, num_iterations=1).explain(img)
    with pytest.raises(TypeError):
        ContrastiveExplainer(_Wrapper(f), steps=3)
    with pytest.raises(TypeError):
        ContrastiveExplainer(_Wrapper(f), c=10.0)                                # omnixai's name: it is c0 here
    with pytest.raises(TypeError):                                               # explain takes the images alone
        ContrastiveExplainer(_Wrapper(f), num_iterations=1).explain(img, kappa=1.0)


def test_a_random_weight_mnist_classifier_runs_the_statement_on_the_cpu():
    from classifiers.mnist import MNISTClassifier
    from explain.contrastive import ContrastiveExplainer, CounterfactualExplainer, Image
    torch.manual_seed(0)
    clf = MNISTClassifier().eval()
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 28, 28, 1, generator=g) * 2 - 1).numpy()
    pre = lambda x_: x_.data.reshape((-1, 1, 28, 28))  # noqa: E731
    before = [p.clone() for p in clf.parameters()]
    for cls, key in ((ContrastiveExplainer, "pn"), (CounterfactualExplainer, "cf")):
        ex = cls(clf, preprocess_function=pre, num_iterations=3, binary_search_steps=2, kappa=0.0, c0=100.0,
                 learning_rate=0.1)
        assert not ex.on_device
        res = ex.explain(Image(x, batched=True)).explanations
        assert len(res) == 2
        with torch.no_grad():
            t0 = clf(torch.from_numpy(x).reshape(-1, 1, 28, 28)).argmax(1)
        for i, e in enumerate(res):
            assert e[key].shape == (28, 28, 1)
            with torch.no_grad():
                label = clf(torch.from_numpy(e[key]).reshape(1, 1, 28, 28)).argmax(1).item()
            assert label == e[key + "_label"]
            if e["found"]:
                assert label != t0[i].item()
                if key == "pn":
                    assert (e[key] >= x[i]).all()
            else:
                assert np.array_equal(e[key], x[i]) and label == t0[i].item()
    assert all(torch.equal(a, b) for a, b in zip(before, clf.parameters()))
    assert all(p.grad is None for p in clf.parameters())
