"""The executors of ``ali_hip.explain`` and the drop-in classes of ``explain/cf_example.py`` on the device.

Reference: this file's own torch statement of the hinge loop's step and of the mixture sweep, evaluated on the CPU in
fp64 on copies of the same modules; yardstick: the same statement in CPU fp32 (``_check`` of test_gpu_xent.py: at most
YARD times the CPU-fp32 error and at most RTOL of max|ref64|).

What is compared how:

* One hinge step is taken apart: the image and the attributes of the closing forward at the initial variables, the
  step's (loss, h, m), the gradient of every raw variable -- all through ``_check`` --, the Adam update at the DEVICE's
  gradient against an fp64 statement of torch.optim.Adam with the bound of test_gpu_classifiers.py (1e-6 * lr +
  6e-8 * max|w|), the step counters, and the weights of G and the classifier bit for bit before and after.
* A yardstick taken on one number is luck: the CPU's own fp32 error on a single value is as often a tenth of an ulp as
  three ulps, and e(device) <= 4 e(CPU) then decides nothing.  Tensors of a handful of numbers -- the gradient of a
  continuous attribute (one number per row), the digit's ten, the three scalars (loss, h, m) next to the ten logits
  they are made of -- are therefore pooled (``_check_pooled``): each is divided by its own max|ref64|, so that none
  hides behind a larger one, and the pool is held to both bounds as one tensor.  z (512 per row) and the images stand
  alone.
* Discrete decisions are compared at equal inputs: which logit the hinge gradient lands on is checked against the
  device's own logits, the sweep's pred / order / n_hit against torch's argmax / stable argsort of the device's own
  logits and metric.  No arg-max of fp32 logits is compared with one of fp64 logits.
* The MNIST cases are seeded (``TieWatch``) so that the fp64 forward has no LeakyReLU input within fp32 noise of zero and
  the two largest non-target logits of every row lie further apart than 1e-4 of the largest logit: no row is left out,
  and the CPU-fp32 statement is asserted to pick the same index.
* Nothing compares a multi-step trajectory with fp64 (Adam turns gradient rounding into O(lr) differences); multi-step
  runs are compared captured against eager, bit for bit.
* The AudioMNIST-sized case (SpectGenerator, six categoricals, 3.4 M LeakyReLU inputs in its classifier) has no
  tie-free draw (test_gpu_classifiers.py): its gradients are printed and held to ten times RTOL of their own scale
  (what a few sign ties can move, measured there, and far below what a wrong table row or Jacobian term would); the
  yardstick bounds are asserted on what a tie cannot move beyond noise -- forward values, (loss, h, m) --, and the
  update at the device's gradient and the discrete decisions at equal inputs as everywhere.
"""
import copy

import pytest
import torch

from test_gpu_conv_geometry import RTOL
from test_gpu_modules import TieWatch
from test_gpu_xent import _check

gpu = pytest.mark.gpu

LR = 0.1
C_HINGE = 10.0
CATEGORICAL = ["digit"]
IGNORED = ["slant"]


def _mnist_models(seed=0):
    import image_scms.mnist as pm
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(seed)
    E, G, clf = pm.Encoder(), pm.Generator(), MNISTClassifier()
    return E.eval(), G.eval(), clf.eval()


def _mnist_batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(B, 1, 28, 28, generator=g))
    digit = torch.zeros(B, 10)
    digit[torch.arange(B), torch.randint(0, 10, (B,), generator=g)] = 1.0
    attrs = {"digit": digit}
    for k in ("thickness", "intensity", "slant"):
        attrs[k] = torch.rand(B, 1, generator=g) * 2 - 1
    init = {k: 0.3 * torch.randn(B, attrs[k].shape[1], generator=g) for k in attrs if k not in IGNORED}
    init["z"] = torch.randn(B, 512, 1, 1, generator=g)
    target = torch.randint(0, 10, (B,), generator=g)
    return x, attrs, init, target


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _first_max_index(row, t):
    """index of the largest entry of the 1-D ``row`` other than ``t``; the first one on ties"""
    best, bi = None, -1
    for i in range(row.shape[0]):
        if i != t and (best is None or row[i].item() > best):
            best, bi = row[i].item(), i
    return bi


def hinge_statement(G, clf, x, attrs, codes, target, p0, init, train_z, categorical, ignored, dt, c=C_HINGE):
    """One evaluation of the loop's loss per row (rows are independent explanations): the image, the transformed
    attributes, the logits, (loss, h, m), the index the hinge picks and the gradient of every raw variable."""
    B = x.shape[0]
    raw = {k: v.to(dt).clone().requires_grad_(True) for k, v in init.items() if k != "z" or train_z}
    a = {}
    for k in attrs:
        a[k] = attrs[k].to(dt) if k in ignored else (raw[k].softmax(1) if k in categorical else raw[k].tanh())
    z = raw["z"].tanh() if train_z else codes.to(dt)
    x_cf = G(z, a)
    logits = clf(x_cf)
    hs, picks = [], []
    for b in range(B):
        if target is None:
            hs.append((logits[b] - p0[b].to(dt)).square().mean())
            picks.append(-1)
        else:
            t = int(target[b])
            i = _first_max_index(logits[b].detach(), t)
            hs.append(logits[b, i] - logits[b, t])
            picks.append(i)
    h = torch.stack(hs)
    m = (x.to(dt) - x_cf).abs().reshape(B, -1).mean(dim=1)
    loss = c * h + m
    grads = torch.autograd.grad(loss.sum(), list(raw.values()))
    return dict(x_cf=x_cf.detach(), attrs={k: v.detach() for k, v in a.items()}, logits=logits.detach(),
                out3=torch.stack([loss, h, m], dim=1).detach(), picks=picks,
                grads={k: g for k, g in zip(raw, grads)})


def _adam_first_step(p, g, lr, b1=0.9, b2=0.999, eps=1e-8):
    m = (1 - b1) * g
    v = (1 - b2) * g * g
    return p - (lr / (1 - b1)) * m / (v.sqrt() / (1 - b2) ** 0.5 + eps)


def _check_pooled(label, triples):
    """``_check`` on several small tensors at once, each (got, ref64, cpu32) scaled by its own max|ref64|"""
    got, ref, f32 = [], [], []
    for g, r, f in triples:
        s = r.abs().max().item() or 1.0
        got.append(g.detach().double().cpu().reshape(-1) / s)
        ref.append(r.double().reshape(-1) / s)
        f32.append(f.double().reshape(-1) / s)
    _check(label, torch.cat(got), torch.cat(ref), torch.cat(f32))


_CASES = {}


def _hinge_case(B, train_z, with_target=True):
    """models, inputs and both statements of a tie-free, well-separated draw"""
    key = (B, train_z, with_target)
    if key in _CASES:
        return _CASES[key]
    E, G, clf = _mnist_models(0)
    G64, clf64 = copy.deepcopy(G).double(), copy.deepcopy(clf).double()
    for v in range(24):
        x, attrs, init, target = _mnist_batch(B, seed=100 * v + B)
        if not with_target:
            target = None
        with torch.no_grad():
            codes = E(x, attrs)
            p0 = clf(x).softmax(1)
        with TieWatch(G64.layers, clf64) as tw:
            ref = hinge_statement(G64, clf64, x, attrs, codes, target, p0, init, train_z, CATEGORICAL, IGNORED,
                                  torch.float64)
        scale = ref["logits"].abs().max().item()
        apart = True
        for b in range(B if target is not None else 0):
            others = ref["logits"][b].clone()
            others[int(target[b])] = float("-inf")
            top2 = others.topk(2).values
            apart = apart and (top2[0] - top2[1]).item() > 1e-4 * scale
        if tw.ties == 0 and apart:
            break
    else:
        pytest.fail("no tie-free, well-separated case in 24 draws")
    f32 = hinge_statement(G, clf, x, attrs, codes, target, p0, init, train_z, CATEGORICAL, IGNORED, torch.float32)
    assert f32["picks"] == ref["picks"]            # the CPU-fp32 statement stays inside the margin: no row is left out
    _CASES[key] = dict(E=E, G=G, clf=clf, x=x, attrs=attrs, init=init, target=target, codes=codes, p0=p0, ref=ref,
                       f32=f32)
    return _CASES[key]


def _stepper(case, capture=False):
    from ali_hip.explain import HingeCFStepper
    G, clf = copy.deepcopy(case["G"]).cuda(), copy.deepcopy(case["clf"]).cuda()
    return HingeCFStepper(G, clf, "digit", CATEGORICAL, IGNORED, c=C_HINGE, capture=capture), G, clf


def _run(stepper, case, steps, train_z, update_z=True, lr=LR):
    t = None if case["target"] is None else case["target"].cuda()
    return stepper.run(case["x"].cuda(), _cuda(case["attrs"]), case["codes"].cuda(), t, _cuda(case["init"]), steps, lr,
                       train_z, update_z=update_z)


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", ["train_z", "codes", "no_target"])
def test_one_hinge_step_taken_apart(B, mode):
    train_z = mode != "codes"
    case = _hinge_case(B, train_z, with_target=mode != "no_target")
    ref, f32 = case["ref"], case["f32"]
    stepper, G, clf = _stepper(case)
    before = {k: v.clone() for m_ in (G, clf) for k, v in m_.state_dict().items()}
    label = f"hinge B={B} {mode}"

    # ---- the closing forward at the initial variables
    x_cf, attrs_cf, _ = _run(stepper, case, 0, train_z)
    assert x_cf.shape == (B, 1, 28, 28)
    _check(label + " x_cf", x_cf, ref["x_cf"], f32["x_cf"])
    for k in case["attrs"]:
        assert attrs_cf[k].shape == case["attrs"][k].shape
        if k in IGNORED:
            assert torch.equal(attrs_cf[k].cpu(), case["attrs"][k])
        else:
            _check(f"{label} attr {k}", attrs_cf[k], ref["attrs"][k], f32["attrs"][k])

    # ---- one step
    _, _, out3 = _run(stepper, case, 1, train_z)
    var = stepper.variables(_cuda(case["attrs"]), train_z, True, B=B)
    probe = var["probe"]
    _check_pooled(label + " logits, (loss, h, m)", [(probe["logits"], ref["logits"], f32["logits"]),
                                                    (out3, ref["out3"], f32["out3"])])
    if case["target"] is not None:                            # where the hinge gradient lands: the device's own logits
        lg, gl = probe["logits"].cpu(), probe["glogit"].cpu()
        for b in range(B):
            t = int(case["target"][b])
            i = _first_max_index(lg[b], t)
            want = torch.zeros(10)
            want[i], want[t] = C_HINGE, -C_HINGE
            assert torch.equal(gl[b], want), (label, b)
            assert i == ref["picks"][b], (label, b)            # (the draw keeps the two candidates 1e-4 apart)
    assert var["step"].tolist() == [1] * B
    small = [(var[k]["graw"], g64, f32["grads"][k]) for k, g64 in ref["grads"].items() if k != "z"]
    _check_pooled(label + " grad attributes", small)
    for k, g64 in ref["grads"].items():
        w = g64.reshape(B, -1).shape[1]
        got = var[k]["graw"]
        if k == "z":
            _check(f"{label} grad z", got, g64.reshape(B, w), f32["grads"][k].reshape(B, w))
        p0 = case["init"][k].reshape(B, w).double()
        want = _adam_first_step(p0, got.double().cpu(), LR)
        err = (var[k]["raw"].double().cpu() - want).abs().max().item()
        bound = 1e-6 * LR + 6e-8 * p0.abs().max().item()
        print(f"EXPLAIN {label} {k} update err={err:.3e} bound={bound:.3e}")
        assert err <= bound, (label, k, err, bound)
    after = {k: v for m_ in (G, clf) for k, v in m_.state_dict().items()}
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for m_ in (G, clf) for p in m_.parameters())


@gpu
def test_a_fixed_z_is_not_a_variable():
    """update_z=False (what the drop-in class passes): tanh(init z) is the latent, nothing of it is updated"""
    case = _hinge_case(1, True)
    stepper, _, _ = _stepper(case)
    x_cf, _, _ = _run(stepper, case, 0, True, update_z=False)
    _check("fixed z x_cf", x_cf, case["ref"]["x_cf"], case["f32"]["x_cf"])
    _run(stepper, case, 1, True, update_z=False)
    var = stepper.variables(_cuda(case["attrs"]), True, False, B=1)
    assert "z" not in var and set(var) == {"step", "probe", "digit", "thickness", "intensity"}
    _check_pooled("fixed z grad attributes", [(var[k]["graw"], case["ref"]["grads"][k], case["f32"]["grads"][k])
                                              for k in ("digit", "thickness", "intensity")])


# ------------------------------------------------------------------------------------------------ capture
@gpu
def test_captured_steps_equal_eager_steps_bit_for_bit():
    case = _hinge_case(3, True)
    out = []
    for capture in (False, True):
        stepper, G, clf = _stepper(case, capture)
        x_cf, attrs_cf, out3 = _run(stepper, case, 5, True)
        var = stepper.variables(_cuda(case["attrs"]), True, True, B=3)
        snap = {k: {n: t.clone() for n, t in var[k].items()} for k in case["ref"]["grads"]}
        out.append((x_cf, attrs_cf, out3, snap, var["step"].clone()))
        if capture:
            assert len(stepper._graphs) == 1
            first = next(iter(stepper._graphs.entries.values()))
            # new inputs of the same signature: the one graph again
            other = dict(case, x=-case["x"], target=(case["target"] + 1) % 10)
            y_cap, _, o_cap = _run(stepper, other, 2, True)
            assert len(stepper._graphs) == 1 and next(iter(stepper._graphs.entries.values())) is first
            eager, _, _ = _stepper(case)
            y_eag, _, o_eag = _run(eager, other, 2, True)
            assert torch.equal(y_cap, y_eag) and torch.equal(o_cap, o_eag)
            # a changed classifier weight drops the graph
            with torch.no_grad():
                clf[0].weight.mul_(1.5)
            y_new, _, o_new = _run(stepper, other, 2, True)
            assert len(stepper._graphs) == 1 and next(iter(stepper._graphs.entries.values())) is not first
            with torch.no_grad():
                eager.classifier[0].weight.mul_(1.5)
            y_eag2, _, o_eag2 = _run(eager, other, 2, True)
            assert torch.equal(y_new, y_eag2) and torch.equal(o_new, o_eag2) and not torch.equal(o_new, o_cap)
    (xe, ae, oe, se, ne), (xc, ac, oc, sc, nc) = out
    assert ne.tolist() == nc.tolist() == [5, 5, 5]
    assert torch.equal(xe, xc) and torch.equal(oe, oc)
    assert all(torch.equal(ae[k], ac[k]) for k in ae)
    for k in se:
        for n in ("raw", "graw", "m", "v"):
            assert torch.equal(se[k][n], sc[k][n]), (k, n)
    assert not torch.equal(se["z"]["raw"].cpu(), case["init"]["z"].reshape(3, -1))


@gpu
def test_batch_sizes_do_not_share_a_graph_when_nothing_is_given():
    """no ignored feature and a trained z: no ``given`` columns, so no argument of the closing forward names the batch;
    B = 1 and then B = 3 through one captured stepper must each get their own variables"""
    from ali_hip.explain import HingeCFStepper
    case = _hinge_case(3, True)
    init = dict(case["init"], slant=0.3 * torch.randn(3, 1, generator=torch.Generator().manual_seed(8)))
    out = {}
    for capture in (False, True):
        G, clf = copy.deepcopy(case["G"]).cuda(), copy.deepcopy(case["clf"]).cuda()
        stepper = HingeCFStepper(G, clf, "digit", CATEGORICAL, [], c=C_HINGE, capture=capture)
        for lo, hi in ((0, 1), (0, 3), (1, 2)):
            r = stepper.run(case["x"][lo:hi].cuda(), {k: v[lo:hi].cuda() for k, v in case["attrs"].items()},
                            case["codes"][lo:hi].cuda(), case["target"][lo:hi].cuda(),
                            {k: v[lo:hi].cuda() for k, v in init.items()}, 2, LR, True, update_z=True)
            out[capture, lo, hi] = r
            assert r[0].shape == (hi - lo, 1, 28, 28) and r[2].shape == (hi - lo, 3)
            assert all(v.shape[0] == hi - lo for v in r[1].values())
        if capture:
            assert len(stepper._graphs) == 2 and len(stepper._final_graphs) == 2
    for lo, hi in ((0, 1), (0, 3), (1, 2)):
        (xe, ae, oe), (xc, ac, oc) = out[False, lo, hi], out[True, lo, hi]
        assert torch.equal(xe, xc) and torch.equal(oe, oc) and all(torch.equal(ae[k], ac[k]) for k in ae), (lo, hi)
    assert not torch.equal(out[True, 0, 1][0], out[True, 1, 2][0])


# ------------------------------------------------------------------------------------------------ the sweep
def sweep_statement(G, clf, x, attrs, codes, orig, target, S, dt):
    from ali_hip.ssim import ssim
    with torch.no_grad():
        eye = torch.eye(10, dtype=dt)
        p = torch.linspace(0, 1, S).reshape(S, 1).to(dt)
        a = {k: v.to(dt).repeat(S, 1) for k, v in attrs.items()}
        a["digit"] = (1 - p) * eye[orig].reshape(1, 10).repeat(S, 1) + p * eye[target].reshape(1, 10).repeat(S, 1)
        samples = G(codes.to(dt).repeat(S, 1, 1, 1), a)
        logits = clf(samples)
        xd = x.to(dt)
        metrics = {"mixture": p.reshape(S), "mse": (xd - samples).square().mean(dim=[1, 2, 3]),
                   "ssim": 1 - ssim((xd.repeat(S, 1, 1, 1) + 1) / 2, (samples + 1) / 2, data_range=1.0,
                                    size_average=False)}
    return samples, logits, metrics


def _select(logits, metric, target):
    pred = logits.argmax(1)
    hit = pred == target
    rows = torch.arange(logits.shape[0])
    return pred.int(), torch.cat([rows[hit][metric[hit].argsort(stable=True)], rows[~hit]]).int(), int(hit.sum())


def _sweep_case():
    if "sweep" not in _CASES:
        E, G, clf = _mnist_models(4)
        x, attrs, _, _ = _mnist_batch(1, seed=2)
        with torch.no_grad():
            codes = E(x, attrs)
            orig = int(copy.deepcopy(clf).double()(x.double()).argmax(1))
        _CASES["sweep"] = dict(E=E, G=G, clf=clf, x=x, attrs=attrs, codes=codes, orig=orig)
    return _CASES["sweep"]


@gpu
@pytest.mark.parametrize("metric", ["mixture", "mse", "ssim"])
@pytest.mark.parametrize("S", [12, 100])
def test_sweep_values_against_fp64_and_decisions_at_equal_inputs(metric, S):
    from ali_hip.explain import MixtureSweep
    case = _sweep_case()
    G, clf = copy.deepcopy(case["G"]).cuda(), copy.deepcopy(case["clf"]).cuda()
    G64, clf64 = copy.deepcopy(case["G"]).double(), copy.deepcopy(case["clf"]).double()
    orig_t = torch.tensor([case["orig"]], dtype=torch.int32, device="cuda")
    out = {}
    for capture in (False, True):
        sweep = MixtureSweep(G, clf, "digit", capture=capture)
        for target in (3, 8):
            r = sweep.run(case["x"].cuda(), case["codes"].cuda(), _cuda(case["attrs"]), target, S, metric, orig=orig_t)
            out[(capture, target)] = {k: v.clone() for k, v in r.items()}
        if capture:
            assert len(sweep._graphs) == 1
    for target in (3, 8):
        r = out[(False, target)]
        label = f"sweep {metric} S={S} t={target}"
        s64, l64, m64 = sweep_statement(G64, clf64, case["x"], case["attrs"], case["codes"], case["orig"], target, S,
                                        torch.float64)
        s32, l32, m32 = sweep_statement(case["G"], case["clf"], case["x"], case["attrs"], case["codes"], case["orig"],
                                        target, S, torch.float32)
        assert r["samples"].shape == (S, 1, 28, 28) and r["metric"].shape == (S,)
        _check(label + " samples", r["samples"], s64, s32)
        _check(label + " logits", r["logits"], l64, l32)
        _check(label + " metric", r["metric"], m64[metric], m32[metric])
        pred, order, n_hit = _select(r["logits"].cpu(), r["metric"].cpu(), target)     # the device's own values
        assert torch.equal(r["pred"].cpu(), pred) and torch.equal(r["order"].cpu(), order)
        assert int(r["n_hit"].item()) == n_hit
        c = out[(True, target)]
        assert all(torch.equal(r[k], c[k]) for k in r), label    # captured == eager, bit for bit


@gpu
def test_sweep_finds_the_original_class_itself_and_limits_sample_points():
    from ali_hip.chain import run_chain
    from ali_hip.classify import nhwc_input
    from ali_hip.explain import MixtureSweep
    case = _sweep_case()
    G, clf = copy.deepcopy(case["G"]).cuda(), copy.deepcopy(case["clf"]).cuda()
    sweep = MixtureSweep(G, clf, "digit")
    x = case["x"].cuda()
    r = sweep.run(x, case["codes"].cuda(), _cuda(case["attrs"]), 3, 7, "mse")
    with torch.no_grad():
        own = run_chain(clf, nhwc_input(x), 1).reshape(1, -1)
    assert int(r["orig"].item()) == int(own.argmax(1))
    given = sweep.run(x, case["codes"].cuda(), _cuda(case["attrs"]), 3, 7, "mse", orig=r["orig"].clone())
    assert torch.equal(given["samples"], r["samples"]) and torch.equal(given["order"], r["order"])
    with pytest.raises(ValueError):
        sweep.run(x, case["codes"].cuda(), _cuda(case["attrs"]), 3, 1025, "mse")


# ------------------------------------------------------------------------------------------------ drop-in classes
@gpu
@pytest.mark.parametrize("metric", ["mixture", "mse", "ssim"])
def test_sweep_drop_in_returns_the_shapes_of_the_cpu_statement(metric):
    from explain.cf_example import DeepCounterfactualExplainer
    case = _sweep_case()
    E, G, clf = (copy.deepcopy(case[k]) for k in ("E", "G", "clf"))
    with torch.no_grad():
        clf[-1].bias[7] += 100.0                     # every row is classified as 7: both branches, whatever the noise
    cpu = DeepCounterfactualExplainer(copy.deepcopy(E), copy.deepcopy(G), copy.deepcopy(clf), "digit")
    E, G, clf = E.cuda(), G.cuda(), clf.cuda()
    ex = DeepCounterfactualExplainer(E, G, clf, "digit")
    x, attrs, S = case["x"].cuda(), _cuda(case["attrs"]), 12
    seen = set()
    for target in range(10):
        got_s, got_m = ex.explain(x, attrs, target, sample_points=S, metric=metric)
        assert ex._sweep and len(ex._sweep._graphs) == 1                  # the executor ran, from one graph
        r = {k: v.clone() for k, v in ex._sweep.run(x, E(x, attrs).detach(), attrs, target, S, metric).items()}
        n = int(r["n_hit"].item())
        seen.add(n > 0)
        hits = r["order"][:n].long()
        if n == 0:
            assert torch.equal(got_s, r["samples"]) and torch.equal(got_m.reshape(-1), r["metric"])
            assert got_s.shape == (S, 1, 28, 28) and got_m.shape == ((S, 1) if metric == "mixture" else (S,))
        elif metric == "mixture":
            assert got_s.shape == (n, 1, 1, 28, 28) and got_m.shape == (n, 1, 1)
            assert torch.equal(got_s, r["samples"][hits[0]].expand(n, 1, 1, 28, 28))
            assert torch.equal(got_m, r["metric"][hits[0]].expand(n, 1, 1))
            assert int(hits[0]) == int((r["pred"] == target).nonzero()[0])
        else:
            assert got_s.shape == (n, 1, 28, 28) and got_m.shape == (n,)
            assert torch.equal(got_s, r["samples"][hits]) and torch.equal(got_m, r["metric"][hits])
            assert bool((got_m[1:] >= got_m[:-1]).all())
        # the layouts the CPU statement can return (its hit count may differ: the logits' margins are within noise)
        cpu_s, cpu_m = cpu.explain(case["x"], case["attrs"], target, sample_points=S, metric=metric)
        allowed = {(5, 3), (4, 2)} if metric == "mixture" else {(4, 1)}
        assert (got_s.dim(), got_m.dim()) in allowed and (cpu_s.dim(), cpu_m.dim()) in allowed
        assert got_s.shape[-3:] == cpu_s.shape[-3:] and got_s.dtype == cpu_s.dtype and got_m.dtype == cpu_m.dtype
    assert seen == {True, False}, "class 7 hits on every row, the other nine on none"


@gpu
def test_hinge_drop_in_on_the_device():
    from explain.cf_example import HingeLossCFExplainer
    case = _hinge_case(3, True)
    E, G, clf = (copy.deepcopy(case[k]).cuda() for k in ("E", "G", "clf"))
    ex = HingeLossCFExplainer(E, G, clf, "digit", 512, categorical_features=CATEGORICAL, features_to_ignore=IGNORED,
                              c=C_HINGE)
    x, attrs = case["x"].cuda(), _cuda(case["attrs"])
    # ---- explain(): the reference's draws, in its order, on its devices
    torch.manual_seed(21)
    got = ex.explain(x[:1], {k: v[:1] for k, v in attrs.items()}, target_class=int(case["target"][0]), steps=2, lr=LR)
    assert got.shape == (1, 1, 28, 28) and got.is_cuda and ex._stepper
    torch.manual_seed(21)
    draws = {k: 0.01 * torch.randn((1, attrs[k].shape[1]), device="cuda") for k in attrs if k not in IGNORED}
    draws["z"] = torch.randn(1, 512, 1, 1).cuda()
    again = ex.explain_batch(x[:1], {k: v[:1] for k, v in attrs.items()}, case["target"][:1].cuda(), steps=2, lr=LR,
                             init=draws)
    assert torch.equal(got, again)
    # ---- explain_batch rows and single calls against the one fp64 statement (zero steps: the closing forward; the
    # z of the drop-in is tanh of its draw and is not optimised)
    init = _cuda(case["init"])
    rows = ex.explain_batch(x, attrs, case["target"].cuda(), steps=0, lr=LR, init=init)
    _check("explain_batch x_cf", rows, case["ref"]["x_cf"], case["f32"]["x_cf"])
    for b in range(3):
        one = ex.explain_batch(x[b:b + 1], {k: v[b:b + 1] for k, v in attrs.items()}, case["target"][b:b + 1].cuda(),
                               steps=0, lr=LR, init={k: v[b:b + 1] for k, v in init.items()})
        _check(f"explain_batch row {b}", one, case["ref"]["x_cf"][b:b + 1], case["f32"]["x_cf"][b:b + 1])
    # ---- one step: the batch's and the single calls' variables against the same fp64 gradient
    st = ex._stepper
    ex.explain_batch(x, attrs, case["target"].cuda(), steps=1, lr=LR, init=init)
    names = ("digit", "thickness", "intensity")
    var = st.variables(attrs, True, False, B=3)
    _check_pooled("explain_batch grad attributes",
                  [(var[k]["graw"], case["ref"]["grads"][k], case["f32"]["grads"][k]) for k in names])
    single = {k: [] for k in names}
    for b in range(3):
        ab = {k: v[b:b + 1] for k, v in attrs.items()}
        ex.explain_batch(x[b:b + 1], ab, case["target"][b:b + 1].cuda(), steps=1, lr=LR,
                         init={k: v[b:b + 1] for k, v in init.items()})
        var = st.variables(ab, True, False, B=1)
        for k in names:
            single[k].append(var[k]["graw"].clone())
    _check_pooled("single calls grad attributes",
                  [(torch.cat(single[k]), case["ref"]["grads"][k], case["f32"]["grads"][k]) for k in names])


@gpu
def test_models_the_executors_do_not_know_run_the_torch_statement():
    from explain.cf_example import DeepCounterfactualExplainer, HingeLossCFExplainer
    case = _sweep_case()
    E, G, clf = (copy.deepcopy(case[k]).cuda() for k in ("E", "G", "clf"))
    x, attrs = case["x"].cuda(), _cuda(case["attrs"])
    ex = DeepCounterfactualExplainer(lambda *a: E(*a), lambda z, a: G(z, a), clf, "digit")
    s, m = ex.explain(x, attrs, 3, sample_points=5, metric="mse")
    assert ex._sweep is None and s.is_cuda and s.shape[1:] == (1, 28, 28) and m.dim() == 1
    hx = HingeLossCFExplainer(lambda *a: E(*a), lambda z, a: G(z, a), clf, "digit", 512, ["digit"], IGNORED)
    out = hx.explain(x, attrs, target_class=3, steps=1)
    assert hx._stepper is None and out.shape == (1, 1, 28, 28)


# ------------------------------------------------------------------------------------------------ AudioMNIST size
@gpu
def test_audio_sized_case_with_a_spect_generator_and_six_categoricals():
    import image_scms.audio_mnist as pm
    from ali_hip.explain import HingeCFStepper, MixtureSweep
    from classifiers.audio_mnist import AudioMNISTClassifier
    torch.manual_seed(3)
    G, clf = pm.Generator(8).eval(), AudioMNISTClassifier(10).eval()
    g = torch.Generator().manual_seed(6)
    x = torch.clip(torch.randn(1, 1, 128, 128, generator=g), -3, 3) / 3
    attrs = {k: torch.eye(n)[torch.randint(0, n, (1,), generator=g)] for k, n in pm.ATTRIBUTE_DIMS.items()}
    codes = torch.randn(1, 512, 1, 1, generator=g)
    keys = list(attrs)
    ignored = [keys[1]]
    init = {k: 0.3 * torch.randn(1, attrs[k].shape[1], generator=g) for k in keys if k not in ignored}
    init["z"] = torch.randn(1, 512, 1, 1, generator=g)
    target = torch.tensor([4])
    G64, clf64 = copy.deepcopy(G).double(), copy.deepcopy(clf).double()
    ref = hinge_statement(G64, clf64, x, attrs, codes, target, None, init, True, keys, ignored, torch.float64)
    f32 = hinge_statement(G, clf, x, attrs, codes, target, None, init, True, keys, ignored, torch.float32)
    Gd, cd = copy.deepcopy(G).cuda(), copy.deepcopy(clf).cuda()
    stepper = HingeCFStepper(Gd, cd, "digit", keys, ignored, c=C_HINGE, capture=True)
    args = (x.cuda(), _cuda(attrs), codes.cuda(), target.cuda(), _cuda(init))
    x_cf, attrs_cf, _ = stepper.run(*args, 0, LR, True, update_z=True)
    _check("audio x_cf", x_cf, ref["x_cf"], f32["x_cf"])
    for k in keys:
        if k not in ignored:
            _check(f"audio attr {k}", attrs_cf[k], ref["attrs"][k], f32["attrs"][k])
    _, _, out3 = stepper.run(*args, 1, LR, True, update_z=True)
    var = stepper.variables(_cuda(attrs), True, True, B=1)
    lg = var["probe"]["logits"].cpu()
    _check("audio logits", lg, ref["logits"], f32["logits"])
    i = _first_max_index(lg[0], 4)
    want = torch.zeros(10)
    want[i], want[4] = C_HINGE, -C_HINGE
    assert torch.equal(var["probe"]["glogit"].cpu()[0], want)
    # this draw keeps the hinge's two candidates apart (fp64: by more than 1e-4 of the largest logit), so all three pick
    # the same one and (loss, h, m) is a matter of rounding
    others = ref["logits"][0].clone()
    others[4] = float("-inf")
    top2 = others.topk(2).values
    assert (top2[0] - top2[1]).item() > 1e-4 * ref["logits"].abs().max().item()
    assert i == ref["picks"][0] == f32["picks"][0]
    _check_pooled("audio logits, (loss, h, m)", [(lg, ref["logits"], f32["logits"]), (out3, ref["out3"], f32["out3"])])
    for k, g64 in ref["grads"].items():
        got = var[k]["graw"]
        scale = g64.abs().max().item()
        e_dev = (got.double().cpu() - g64.reshape(1, -1)).abs().max().item()
        e_cpu = (f32["grads"][k].double() - g64).abs().max().item()
        print(f"EXPLAIN audio grad {k} e_dev={e_dev:.3e} e_cpu={e_cpu:.3e} scale={scale:.3e}")
        # a sign tie moves one element's derivative in any fp32 evaluation; test_gpu_classifiers.py measured what that
        # does to this classifier's gradients: 2.3e-4 of their maximum, for the CPU and the device alike.  Ten times
        # RTOL leaves room for a few of them and still catches a wrong table row, Jacobian term or segment offset,
        # which are errors of the size of the gradient itself
        assert e_dev <= 10 * RTOL * scale, (k, e_dev, scale)
        p0 = init[k].reshape(1, -1).double()
        err = (var[k]["raw"].double().cpu() - _adam_first_step(p0, got.double().cpu(), LR)).abs().max().item()
        assert err <= 1e-6 * LR + 6e-8 * p0.abs().max().item(), (k, err)
    assert var["step"].tolist() == [1]
    # ---- the sweep, five points
    sweep = MixtureSweep(Gd, cd, "digit")
    r = sweep.run(x.cuda(), codes.cuda(), _cuda(attrs), 4, 5, "mse")
    orig = int(r["orig"].item())

    def stmt(Gm, cm, dt):
        with torch.no_grad():
            p = torch.linspace(0, 1, 5).reshape(5, 1).to(dt)
            a = {k: v.to(dt).repeat(5, 1) for k, v in attrs.items()}
            eye = torch.eye(10, dtype=dt)
            a["digit"] = (1 - p) * eye[orig].reshape(1, 10).repeat(5, 1) + p * eye[4].reshape(1, 10).repeat(5, 1)
            s = Gm(codes.to(dt).repeat(5, 1, 1, 1), a)
            return s, cm(s), (x.to(dt) - s).square().mean(dim=[1, 2, 3])
    s64, l64, m64 = stmt(G64, clf64, torch.float64)
    s32, l32, m32 = stmt(G, clf, torch.float32)
    _check("audio sweep samples", r["samples"], s64, s32)
    _check("audio sweep logits", r["logits"], l64, l32)
    _check("audio sweep mse", r["metric"], m64, m32)
    pred, order, n_hit = _select(r["logits"].cpu(), r["metric"].cpu(), 4)
    assert torch.equal(r["pred"].cpu(), pred) and torch.equal(r["order"].cpu(), order) and int(r["n_hit"]) == n_hit
