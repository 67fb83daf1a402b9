"""Pertinent positives on the device: ``ali_hip.contrast.ContrastiveSearch(..., mode="pp", background=b)`` and
``explain.contrastive.ContrastiveExplainer(..., positives=True)``; the method of test_gpu_contrastive.py.  A
``MNISTClassifier`` with seeded random weights, 28 x 28 images in [-1, 1], B = 1 and 3, b = 0.0 and -1.0, K = 3.

One replay taken apart: from the device's own state after two replays, the third one's logits and input gradient are
compared with the classifier in fp64 on the CPU, its update with ``pp_update_statement`` in fp64 on the device's own
gradient, under the CPU-fp32 yardstick (``_check`` of test_gpu_xent.py); arg-max, success (pred == t0), the seed, the
bookkeeping and the c table are recomputed from the device's own logits and distances and compared exactly; pixels
at b and at x0 exactly; the replay at k == K resets the rows to b bit for bit.  ``TieWatch`` keeps LeakyReLU inputs
within fp32 noise of zero out of the compared state.

Whole runs by their properties: a found row's image gets t0 from the same classifier on the device, fed in the
search's 2B-row batch shape; every image lies in its box [min(b, x0), max(b, x0)]; ``dist`` is the elastic-net
distance of the returned image from b; unfound rows are x0 bit for bit with t0.  ``HYPER`` finds rows; ``UNFOUND``
leaves a row unfound wherever the fp32 statement on the CPU does (test_contrastive_pp_cpu.py holds it to that at
B = 3).  Captured runs equal eager runs and their own repetition bit for bit; parameters and ``.grad`` are untouched;
the explainer with ``positives=True`` equals the executor bit for bit and its pn part a ``positives=False`` run."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_explain import _check_pooled
from test_gpu_modules import TieWatch
from test_gpu_xent import _check

gpu = pytest.mark.gpu

K, ROUNDS = 3, 2
HYPER = dict(num_iterations=K, binary_search_steps=ROUNDS, kappa=0.0, c0=1e4, learning_rate=0.1)
UNFOUND = dict(num_iterations=K, binary_search_steps=1, kappa=0.0, c0=1e-6)
APART = dict(HYPER, kappa=10.0)         # the default kappa: far above this classifier's logit gaps, the hinge stays on
BETA, CLIP = 0.1, 1e3                                               # the defaults the cases leave alone
BGS = (0.0, -1.0)


def _clf():
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(0)
    return MNISTClassifier().eval()


def _x(B, seed=1):
    return (torch.rand(3, 1, 28, 28, generator=torch.Generator().manual_seed(seed)) * 2 - 1)[:B].contiguous()


def _search(bg, hyper=HYPER, **kw):
    from ali_hip.contrast import ContrastiveSearch
    clf = _clf().cuda()
    return ContrastiveSearch(clf, "pp", background=bg, **kw, **hyper), clf


def _snapshot(st):
    return {k: v.detach().clone().cpu() for k, v in st.items() if torch.is_tensor(v)}


# ------------------------------------------------------------------------------------------------ one replay
@gpu
@pytest.mark.parametrize("bg", BGS)
@pytest.mark.parametrize("B", [1, 3])
def test_one_replay_taken_apart(B, bg):
    from ali_hip.contrast import attack_pp_statement, c_table_statement, pp_update_statement
    cpu = _clf()
    clf64 = copy.deepcopy(cpu).double()
    search, clf = _search(bg, APART, capture=False)
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    label = f"contrast pp B={B} b={bg}"
    for variant in range(12):                                   # a start whose state after two replays has no tie
        x = _x(B, seed=1 + variant)
        st = search.start(x.cuda())
        search.advance(2)
        old = _snapshot(st)
        with TieWatch(clf64) as tw, torch.no_grad():
            logits64 = clf64(old["rows"].double())
        if tw.ties == 0:
            break
    else:
        pytest.fail("no tie-free state in 12 draws")
    assert old["it"].tolist() == [2] * B and old["rnd"].tolist() == [0] * B
    x0 = x.reshape(B, -1)
    assert torch.equal(old["x0"], x0)
    with torch.no_grad():
        assert torch.equal(old["t0"].long(), clf64(x.double()).argmax(1)), label
        logits32 = cpu(old["rows"])
    t0, c = old["t0"], old["ctab"][0]
    rows_old = old["rows"].reshape(-1, 784)
    v_old, point = rows_old[:B], rows_old[B:]                   # the gradient is taken at the slack rows
    lo, hi = torch.minimum(x0, torch.full_like(x0, bg)), torch.maximum(x0, torch.full_like(x0, bg))
    assert ((rows_old >= lo.repeat(2, 1)) & (rows_old <= hi.repeat(2, 1))).all(), label

    search.advance(1)
    new, probe = _snapshot(st), {k: v.detach().cpu() for k, v in st["probe"].items()}
    # ---- the forward chain, and what is decided from its logits
    _check(label + " logits", probe["logits"], logits64, logits32)
    lg = probe["logits"]
    pred = lg[:B].argmax(1)
    succ = pred == t0.long()
    assert torch.equal(probe["pred"].long(), pred) and torch.equal(probe["succ"].bool(), succ), label
    A64, seed64, _ = attack_pp_statement(lg[B:].double(), t0, c.double(), APART["kappa"])
    A32, _, _ = attack_pp_statement(lg[B:], t0, c, APART["kappa"])
    assert (A64 > 0).all(), label                               # every row's gradient path is exercised
    assert torch.equal(probe["seed"].double(), seed64), label
    _check_pooled(label + " A", [(probe["A"], A64, A32)])

    # ---- the data gradient of the device's seed
    def grad(model, dt):
        p = point.to(dt).reshape(B, 1, 28, 28).requires_grad_(True)
        g, = torch.autograd.grad(model(p), p, probe["seed"].to(dt))
        return g.reshape(B, -1)
    gx = probe["gx"].reshape(B, 784, -1)[:, :, 0]
    _check(label + " gx", gx, grad(clf64, torch.float64), grad(cpu, torch.float32))
    # ---- bookkeeping of v_2: from the device's own distances and flags
    better = succ & (old["dist"] < old["best_dist"])
    assert torch.equal(new["copied"].bool(), better), label
    assert torch.equal(new["best"], torch.where(better.unsqueeze(1), v_old, old["best"])), label
    assert torch.equal(new["best_dist"], torch.where(better, old["dist"], old["best_dist"])), label
    assert torch.equal(new["best_label"].long(), torch.where(better, pred, old["best_label"].long())), label
    assert torch.equal(new["found"].bool(), old["found"].bool() | better), label
    assert torch.equal(new["round_succ"].bool(), old["round_succ"].bool() | succ), label
    assert torch.equal(new["ctab"], old["ctab"]), label
    # ---- the update (k = 2), continued from the device's state and gradient
    assert new["it"].tolist() == [K] * B
    rows_new = new["rows"].reshape(-1, 784)

    def upd(dt):
        return pp_update_statement(v_old.to(dt), point.to(dt), x0.to(dt), gx.to(dt), 2, K, APART["learning_rate"],
                                   BETA, CLIP, bg)
    (v64, y64, l1_64, l2_64, n64), (v32, y32, l1_32, l2_32, n32) = upd(torch.float64), upd(torch.float32)
    _check(label + " v", rows_new[:B], v64, v32)
    _check(label + " y", rows_new[B:], y64, y32)
    for got, r64 in ((rows_new[:B], v64), (rows_new[B:], y64)):                # pixels at b and at x0, exactly
        assert torch.equal(got == bg, r64.float() == bg) and torch.equal(got == x0, r64.float() == x0), label
    _check_pooled(label + " distances", [(new["l1"], l1_64, l1_32), (new["l2"], l2_64, l2_32),
                                         (new["dist"], l2_64 + BETA * l1_64, l2_32 + BETA * l1_32),
                                         (new["gnorm"], n64, n32)])
    # ---- the replay at k == K: v_3 is booked, the table moves, the next round starts from b
    search.advance(1)
    end, probe = _snapshot(st), {k: v.detach().cpu() for k, v in st["probe"].items()}
    rs = new["round_succ"].bool() | probe["succ"].bool()
    want = c_table_statement(*[t.double() for t in new["ctab"]], rs)
    assert torch.equal(end["ctab"], torch.stack(want).float()), label
    assert end["it"].tolist() == [0] * B and end["rnd"].tolist() == [1] * B and not end["round_succ"].any()
    assert torch.equal(end["rows"], torch.full_like(end["rows"], bg)), label
    after = clf.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in clf.parameters())


# ------------------------------------------------------------------------------------------------ whole runs
def _check_run(clf, x, bg, out, label):
    B = x.shape[0]
    xd = x.cuda()
    assert out["image"].shape == (B, 1, 28, 28) and out["image"].dtype == torch.float32 and out["image"].is_cuda
    for k, dt in (("label", torch.int32), ("found", torch.int32), ("dist", torch.float32), ("c", torch.float32)):
        assert out[k].shape == (B,) and out[k].dtype == dt and out[k].is_cuda, k
    with torch.no_grad():                                       # the search's batch shape: 2B rows
        t0 = clf(xd.repeat(2, 1, 1, 1))[:B].argmax(1)
        got = clf(out["image"].repeat(2, 1, 1, 1))[:B].argmax(1)
    found = out["found"].bool()
    assert torch.equal(got[found], t0[found]), label
    assert torch.equal(out["label"].long(), t0), label
    assert torch.equal(out["image"][~found], xd[~found]), label               # unfound: x0 bit for bit
    b = torch.full_like(xd, bg)
    assert ((out["image"] >= torch.minimum(xd, b)) & (out["image"] <= torch.maximum(xd, b))).all(), label
    img = out["image"].cpu().reshape(B, -1)

    def en(dt):
        d = img.to(dt) - bg
        return torch.where(found.cpu(), d.pow(2).sum(1) + BETA * d.abs().sum(1), torch.zeros(B, dtype=dt))
    _check_pooled(label + " dist", [(out["dist"], en(torch.float64), en(torch.float32))])
    assert not out["dist"][~found].any(), label


@gpu
@pytest.mark.parametrize("bg", BGS)
@pytest.mark.parametrize("B", [1, 3])
def test_properties_of_found_and_unfound_runs_captured_against_eager(B, bg):
    from ali_hip.contrast import cem_pp_statement
    x = _x(B)
    cap, clf = _search(bg, capture=True)
    eager, _ = _search(bg, capture=False)
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    out = cap.run(x.cuda())
    label = f"contrast pp run B={B} b={bg}"
    _check_run(clf, x, bg, out, label)
    assert out["found"].any(), label                                            # HYPER finds rows
    want = eager.run(x.cuda())
    assert all(torch.equal(out[k], want[k]) for k in out), label                # captured == eager, bit for bit
    again = cap.run(x.cuda())
    assert all(torch.equal(out[k], again[k]) for k in out), label               # and its own repetition
    assert len(cap._graphs) == 1 and len(eager._graphs) == 0
    # c0 = 1e-6 and one round: the attack is too weak to leave b
    weak, wclf = _search(bg, UNFOUND, capture=True)
    none = weak.run(x.cuda())
    _check_run(wclf, x, bg, none, label + " unfound")
    if not cem_pp_statement(_clf(), x, background=bg, **UNFOUND)["found"].all():
        assert (none["found"] == 0).any(), label
    grown = (torch.tensor(1e-6).double() * 10).float().item()                   # one failed round: c * 10
    assert (none["c"][none["found"] == 0] == grown).all(), label
    after = clf.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in clf.parameters())


@gpu
def test_the_background_is_part_of_the_graph_key():
    cap, _ = _search(0.0, capture=True)
    cap.run(_x(1).cuda())
    assert len(cap._graphs) == 1
    cap.background = -1.0                                                      # (as another search would have it)
    out = cap.run(_x(1).cuda())
    assert len(cap._graphs) == 2
    other, _ = _search(-1.0, capture=True)
    want = other.run(_x(1).cuda())
    assert all(torch.equal(out[k], want[k]) for k in out)


# ------------------------------------------------------------------------------------------------ the shim
@gpu
@pytest.mark.parametrize("bg", BGS)
def test_shim_with_positives_equals_the_executors(bg):
    import explain.contrastive as xc
    from ali_hip.contrast import ContrastiveSearch
    x = _x(3)
    pp, _ = _search(bg, capture=True)
    want = pp.run(x.cuda())
    pre = lambda x_: x_.data.reshape((-1, 1, 28, 28))  # noqa: E731
    ex = xc.ContrastiveExplainer(_clf().cuda(), preprocess_function=pre, positives=True, background=bg, **HYPER)
    plain = xc.ContrastiveExplainer(_clf().cuda(), preprocess_function=pre, **HYPER)
    assert ex.on_device
    nhwc = x.numpy().reshape((3, 28, 28, 1))                                    # one channel: the same element order
    res = ex.explain(xc.Image(nhwc, batched=True)).explanations
    base = plain.explain(xc.Image(nhwc, batched=True)).explanations
    assert len(res) == 3
    for i, (e, p) in enumerate(zip(res, base)):
        assert set(e) == {"pn", "pn_label", "found", "pp", "pp_label", "pp_found"} and e["pp"].shape == (28, 28, 1)
        assert np.array_equal(e["pp"].reshape(1, 28, 28), want["image"][i].cpu().numpy())
        assert e["pp_label"] == int(want["label"][i]) and e["pp_found"] == int(want["found"][i])
        assert set(p) == {"pn", "pn_label", "found"}
        assert np.array_equal(e["pn"], p["pn"]) and e["pn_label"] == p["pn_label"] and e["found"] == p["found"]
    every = ex.explain_all(nhwc, batch=2)
    assert every["pp"].shape == (3, 28, 28, 1) and every["pp_found"].tolist() == [e["pp_found"] for e in res]
    parts = torch.cat([pp.run(x[lo:lo + 2].cuda())["image"] for lo in (0, 2)]).cpu().numpy()
    assert np.array_equal(every["pp"].reshape(3, 1, 28, 28), parts)
    pn = ContrastiveSearch(_clf().cuda(), "pn", **HYPER)
    pn_parts = torch.cat([pn.run(x[lo:lo + 2].cuda())["image"] for lo in (0, 2)]).cpu().numpy()
    assert np.array_equal(every["pn"].reshape(3, 1, 28, 28), pn_parts)
