"""The executor ``ali_hip.contrast.ContrastiveSearch`` and the drop-in surface of ``explain/contrastive.py`` on the
device: a ``MNISTClassifier`` with seeded random weights, 28 x 28 images, B = 1 and 3, K = 3 iterations, two rounds.

One replay taken apart (the method of test_gpu_explain.py): from the device's own state after two replays, everything
the third one produces is compared with the statement continued from that state -- the logits and the input gradient
against the classifier in fp64 on the CPU, the update against ``cem_update_statement`` / ``ce_update_statement`` in fp64
on the device's own gradient -- under the CPU-fp32 yardstick (``_check`` of test_gpu_xent.py).  Discrete decisions (arg-max,
success, where the seed lands, what goes into the best, the c table) are recomputed from the device's own logits and
distances and are therefore exact.  The cases are seeded so that the fp64 forward at the device's state has no
LeakyReLU input within fp32 noise of zero (``TieWatch``).

Whole runs are held to their properties: a found row's image gets the returned label from the same classifier on the
device (fed in the batch shape the search used, so the logits are the search's own bits) and that label is not t0;
pertinent negatives only add and stay inside [lo, hi]; unfound rows are x0 bit for bit; ``dist`` is the distance of the
returned image.  ``HYPER`` (small kappa, large c0) finds rows and ``UNFOUND`` (c0 = 1e-6, one round) leaves rows
unfound: the fp32 statement on the CPU says so for these seeds (the first test, which needs no GPU) and the device
tests assert it.  Captured runs equal eager runs and their own repetition bit for bit; parameters and ``.grad`` are
untouched."""
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
BETA, GAMMA, CLIP = 0.1, 1.0, 1e3                                   # the defaults the cases leave alone


def _clf():
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(0)
    return MNISTClassifier().eval()


def _x(B, seed=1):
    return (torch.rand(3, 1, 28, 28, generator=torch.Generator().manual_seed(seed)) * 2 - 1)[:B].contiguous()


def _statement(mode):
    from ali_hip.contrast import ce_statement, cem_pn_statement
    return cem_pn_statement if mode == "pn" else ce_statement


def _search(mode, hyper=HYPER, **kw):
    from ali_hip.contrast import ContrastiveSearch
    clf = _clf().cuda()
    return ContrastiveSearch(clf, mode, **kw, **hyper), clf


@pytest.mark.parametrize("mode", ["pn", "ce"])
@pytest.mark.parametrize("B", [1, 3])
def test_cpu_fp32_statement_finds_and_misses_on_the_chosen_seeds(mode, B):
    clf, x = _clf(), _x(B)
    assert _statement(mode)(clf, x, **HYPER)["found"].all()
    assert not _statement(mode)(clf, x, **UNFOUND)["found"].any()


# ------------------------------------------------------------------------------------------------ one replay
def _snapshot(st):
    return {k: v.detach().clone().cpu() for k, v in st.items() if torch.is_tensor(v)}


@gpu
@pytest.mark.parametrize("mode", ["pn", "ce"])
@pytest.mark.parametrize("B", [1, 3])
def test_one_replay_taken_apart(mode, B):
    from ali_hip.contrast import (attack_statement, c_table_statement, ce_update_statement, cem_update_statement)
    pn = mode == "pn"
    cpu = _clf()
    clf64 = copy.deepcopy(cpu).double()
    search, clf = _search(mode, APART, capture=False)
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    label = f"contrast {mode} B={B}"
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
    assert torch.equal(old["x0"], x0) and torch.equal(old["lo"], x0.amin(1)) and torch.equal(old["hi"], x0.amax(1))
    with torch.no_grad():
        assert torch.equal(old["t0"].long(), clf64(x.double()).argmax(1)), label
        logits32 = cpu(old["rows"])
    t0, c = old["t0"], old["ctab"][0]
    rows_old = old["rows"].reshape(-1, 784)
    v_old = rows_old[:B]
    point = rows_old[B:] if pn else v_old                       # where the gradient is taken

    search.advance(1)
    new, probe = _snapshot(st), {k: v.detach().cpu() for k, v in st["probe"].items()}
    # ---- the forward chain, and what is decided from its logits
    _check(label + " logits", probe["logits"], logits64, logits32)
    lg = probe["logits"]
    pred = lg[:B].argmax(1)
    succ = pred != t0.long()
    assert torch.equal(probe["pred"].long(), pred) and torch.equal(probe["succ"].bool(), succ), label
    lg_point = lg[B:] if pn else lg
    A64, seed64, _ = attack_statement(lg_point.double(), t0, c.double(), APART["kappa"])
    A32, _, _ = attack_statement(lg_point, t0, c, APART["kappa"])
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
    dist_old = old["dist"] if pn else old["l1"]
    better = succ & (dist_old < old["best_dist"])
    assert torch.equal(new["copied"].bool(), better), label
    assert torch.equal(new["best"], torch.where(better.unsqueeze(1), v_old, old["best"])), label
    assert torch.equal(new["best_dist"], torch.where(better, dist_old, old["best_dist"])), label
    assert torch.equal(new["best_label"].long(), torch.where(better, pred, old["best_label"].long())), label
    assert torch.equal(new["found"].bool(), old["found"].bool() | better), label
    assert torch.equal(new["round_succ"].bool(), old["round_succ"].bool() | succ), label
    assert torch.equal(new["ctab"], old["ctab"]), label
    # ---- the update (k = 2), continued from the device's state and gradient
    assert new["it"].tolist() == [K] * B
    rows_new = new["rows"].reshape(-1, 784)
    lo, hi = old["lo"], old["hi"]
    if pn:
        def upd(dt):
            return cem_update_statement(v_old.to(dt), point.to(dt), x0.to(dt), gx.to(dt), 2, K, APART["learning_rate"],
                                        BETA, CLIP, lo.to(dt), hi.to(dt))
        (v64, y64, l1_64, l2_64, n64), (v32, y32, l1_32, l2_32, n32) = upd(torch.float64), upd(torch.float32)
        _check(label + " v", rows_new[:B], v64, v32)
        _check(label + " y", rows_new[B:], y64, y32)
        assert torch.equal(rows_new[:B] == x0, v64.float() == x0), label         # pixels back at x0, exactly
        _check_pooled(label + " distances", [(new["l1"], l1_64, l1_32), (new["l2"], l2_64, l2_32),
                                             (new["dist"], l2_64 + BETA * l1_64, l2_32 + BETA * l1_32),
                                             (new["gnorm"], n64, n32)])
    else:
        def upd(dt):
            return ce_update_statement(v_old.to(dt), x0.to(dt), gx.to(dt), old["m"].to(dt), old["v2"].to(dt), 3,
                                       APART["learning_rate"], GAMMA, CLIP, lo.to(dt), hi.to(dt))
        (v64, m64, s64, l1_64, n64), (v32, m32, s32, l1_32, n32) = upd(torch.float64), upd(torch.float32)
        _check(label + " v", rows_new, v64, v32)
        _check(label + " m", new["m"], m64, m32)
        _check(label + " v2", new["v2"], s64, s32)
        _check_pooled(label + " distances", [(new["l1"], l1_64, l1_32), (new["gnorm"], n64, n32)])
    # ---- the replay at k == K: v_3 is booked, the table moves, the next round starts from x0
    search.advance(1)
    end, probe = _snapshot(st), {k: v.detach().cpu() for k, v in st["probe"].items()}
    rs = new["round_succ"].bool() | probe["succ"].bool()
    want = c_table_statement(*[t.double() for t in new["ctab"]], rs)
    assert torch.equal(end["ctab"], torch.stack(want).float()), label
    assert end["it"].tolist() == [0] * B and end["rnd"].tolist() == [1] * B and not end["round_succ"].any()
    assert torch.equal(end["rows"].reshape(-1, 784), x0.repeat(2 if pn else 1, 1)), label
    if not pn:
        assert not end["m"].any() and not end["v2"].any()
    after = clf.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in clf.parameters())


# ------------------------------------------------------------------------------------------------ whole runs
def _distance(mode, img, x0, dt):
    d = (img.to(dt) - x0.to(dt)).reshape(x0.shape[0], -1)
    return d.pow(2).sum(1) + BETA * d.abs().sum(1) if mode == "pn" else d.abs().sum(1)


def _check_run(mode, clf, x, out, label):
    B = x.shape[0]
    xd = x.cuda()
    assert out["image"].shape == (B, 1, 28, 28) and out["image"].dtype == torch.float32 and out["image"].is_cuda
    for k, dt in (("label", torch.int32), ("found", torch.int32), ("dist", torch.float32), ("c", torch.float32)):
        assert out[k].shape == (B,) and out[k].dtype == dt and out[k].is_cuda, k
    rep = 2 if mode == "pn" else 1                              # the batch shape the search evaluated its iterates in
    with torch.no_grad():
        t0 = clf(xd.repeat(rep, 1, 1, 1))[:B].argmax(1)        # (t0 is taken in that batch shape too)
        got = clf(out["image"].repeat(rep, 1, 1, 1))[:B].argmax(1)
    found = out["found"].bool()
    assert torch.equal(got[found], out["label"][found].long()), label
    assert (out["label"][found].long() != t0[found]).all(), label
    assert torch.equal(out["label"][~found].long(), t0[~found]), label
    assert torch.equal(out["image"][~found], xd[~found]), label               # unfound: x0 bit for bit
    lo, hi = xd.amin(dim=(1, 2, 3), keepdim=True), xd.amax(dim=(1, 2, 3), keepdim=True)
    assert ((out["image"] >= lo) & (out["image"] <= hi)).all(), label
    if mode == "pn":
        assert (out["image"] >= xd).all(), label
    img = out["image"].cpu()
    _check_pooled(label + " dist", [(out["dist"], _distance(mode, img, x, torch.float64),
                                     _distance(mode, img, x, torch.float32))])
    assert (out["dist"][found] > 0).all() and not out["dist"][~found].any(), label


@gpu
@pytest.mark.parametrize("mode", ["pn", "ce"])
@pytest.mark.parametrize("B", [1, 3])
def test_properties_of_found_and_unfound_runs_captured_against_eager(mode, B):
    x = _x(B)
    cap, clf = _search(mode, capture=True)
    eager, _ = _search(mode, capture=False)
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    out = cap.run(x.cuda())
    label = f"contrast run {mode} B={B}"
    _check_run(mode, clf, x, out, label)
    assert out["found"].any(), label                                            # HYPER finds rows
    want = eager.run(x.cuda())
    assert all(torch.equal(out[k], want[k]) for k in out), label                # captured == eager, bit for bit
    again = cap.run(x.cuda())
    assert all(torch.equal(out[k], again[k]) for k in out), label               # and its own repetition
    assert len(cap._graphs) == 1 and len(eager._graphs) == 0
    first = next(iter(cap._graphs.entries.values()))
    other = _x(3, seed=5)[3 - B:].contiguous()                                  # other images, the same signature
    out2 = cap.run(other.cuda())
    assert len(cap._graphs) == 1 and next(iter(cap._graphs.entries.values())) is first
    _check_run(mode, clf, other, out2, label + " other")
    want2 = eager.run(other.cuda())
    assert all(torch.equal(out2[k], want2[k]) for k in out2) and not torch.equal(out2["image"], out["image"]), label
    # c0 = 1e-6 and one round: the attack is too weak, rows stay unfound
    weak, wclf = _search(mode, UNFOUND, capture=True)
    none = weak.run(x.cuda())
    _check_run(mode, wclf, x, none, label + " unfound")
    assert (none["found"] == 0).any(), label
    grown = (torch.tensor(1e-6).double() * 10).float().item()                   # one failed round: c * 10
    assert (none["c"][none["found"] == 0] == grown).all(), label
    after = clf.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in clf.parameters())


@gpu
def test_one_graph_per_signature():
    cap, _ = _search("ce", capture=True)
    cap.run(_x(1).cuda())
    cap.run(_x(1, seed=2).cuda())
    assert len(cap._graphs) == 1
    cap.run(_x(3).cuda())
    assert len(cap._graphs) == 2
    cap.run(_x(1).cuda())
    assert len(cap._graphs) == 2


@gpu
def test_refusals_on_the_device():
    from ali_hip.contrast import ContrastiveSearch
    clf = _clf().cuda()
    with pytest.raises(TypeError):
        ContrastiveSearch(torch.nn.Sequential(*list(clf.children())).cuda(), "pn")
    with pytest.raises(ValueError):
        ContrastiveSearch(clf.train(), "pn")
    search = ContrastiveSearch(clf.eval(), "pn", **HYPER)
    with pytest.raises(ValueError):
        search.run(_x(1))                                                       # CPU tensors: the statement serves them
    clf.train()
    with pytest.raises(ValueError):
        search.run(_x(1).cuda())
    import explain.contrastive as xc
    with pytest.raises(ValueError, match=r"eval\(\)"):                           # the shim says so where it is built
        xc.ContrastiveExplainer(clf)
    assert xc.CounterfactualExplainer(clf.eval()).on_device


# ------------------------------------------------------------------------------------------------ the shim
@gpu
@pytest.mark.parametrize("name", ["ContrastiveExplainer", "CounterfactualExplainer"])
def test_shim_on_a_cuda_model_equals_the_executor(name):
    import explain.contrastive as xc
    mode, key = ("pn", "pn") if name == "ContrastiveExplainer" else ("ce", "cf")
    x = _x(3)
    search, _ = _search(mode, capture=True)
    want = search.run(x.cuda())
    clf = _clf().cuda()
    ex = getattr(xc, name)(clf, preprocess_function=lambda x_: x_.data.reshape((-1, 1, 28, 28)), **HYPER)
    assert ex.on_device
    nhwc = x.numpy().reshape((3, 28, 28, 1))                                    # one channel: the same element order
    res = ex.explain(xc.Image(nhwc, batched=True)).explanations
    assert len(res) == 3
    for i, e in enumerate(res):
        assert set(e) == {key, key + "_label", "found"} and e[key].shape == (28, 28, 1)
        assert np.array_equal(e[key].reshape(1, 28, 28), want["image"][i].cpu().numpy())
        assert e[key + "_label"] == int(want["label"][i]) and e["found"] == int(want["found"][i])
    # the scripts' own line, one image at a time
    one = ex.explain(xc.Image(nhwc[:1].reshape((1, 28, 28, 1)), batched=True)).explanations[0][key].reshape((1, 1, 28, 28))
    assert one.shape == (1, 1, 28, 28)
    every = ex.explain_all(nhwc, batch=2)
    assert every[key].shape == (3, 28, 28, 1) and every["found"].tolist() == [e["found"] for e in res]
    parts = torch.cat([search.run(x[lo:lo + 2].cuda())["image"] for lo in (0, 2)]).cpu().numpy()
    assert np.array_equal(every[key].reshape(3, 1, 28, 28), parts)
