"""The three classifiers of ``classifiers/`` and the executors of ``ali_hip.classify`` on the device.

Reference: the stock modules of the same class in fp64 on the CPU (CPU inputs never touch the kernels) with
``CrossEntropyLoss`` and ``torch.optim.Adam`` -- the statements of classifiers/mnist.py:48-56; yardstick: the same in
CPU fp32; bounds as in test_gpu_xent.py.  One stepper step is taken apart so that every part has a bound that follows
from fp32 arithmetic: the loss and every parameter gradient against fp64 autograd (yardstick), and the updated weights
against an fp64 Adam step fed the gradient the device computed (Adam's first step is -lr * g / (|g| + eps): for
|g| ~ eps it amplifies gradient rounding by 1 / eps, on the host as on the device, so the update is compared at equal
gradients; 1e-6 relative of the step size lr bounds the kernel's own fp32 rounding of w - lr * m / (sqrt(v) + eps)
plus the fp32 spacing of the weights, 6e-8 * max|w|).  Against the reference's own updated weights the statistics of
test_gpu_callers.py (``_check_encoder_update``) apply.

Sign ties (``TieWatch`` of test_gpu_modules.py): the MNIST case (0.4 M LeakyReLU inputs at B = 8) is re-seeded until the
fp64 forward has none, and all of the above holds.  The spectrogram classifiers have 3.4 M (AudioMNIST, B = 2) and 7 M
(whale, B = 1) LeakyReLU inputs; about one in a million lies within fp32 noise of zero, so no draw is tie free (24 of 24
were not).  A tie flips one element's derivative between 1 and 0.2 in every fp32 evaluation that rounds it the other way
than fp64 -- measured on AudioMNIST: the first layer's bias gradient of the CPU-fp32 pass and of the device both lie
4.9e-8 (2.3e-4 of its maximum) from fp64 and within 2e-10 of each other -- so a per-parameter gradient comparison with
fp64 says nothing there.  For these two the gradient figures are printed, and what is asserted is what a tie cannot
move beyond noise: logits and loss (both bounds), the Adam update at the device's gradient, and the updated weights
against the fp64 restatement's by the statistics of ``_check_encoder_update``.  The gradients of these layer shapes are
pinned per stage by test_gpu_conv_geometry.py and, end to end and tie free, by the MNIST case and
test_gpu_classifier_chain.py.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_callers import _check_encoder_update
from test_gpu_classifier_chain import compare_with_autograd
from test_gpu_modules import paired_models, tie_free, to_dev
from test_gpu_xent import _check

gpu = pytest.mark.gpu
LR = 1e-4


def _family(name):
    from classifiers import audio_mnist, mnist, whalecalls
    cls, hw, B, n = {"mnist": (mnist.MNISTClassifier, 28, 8, 10), "audio": (audio_mnist.AudioMNISTClassifier, 128, 2, 10),
                     "whale": (whalecalls.NARWClassifier, 256, 1, 3)}[name]
    torch.manual_seed(31)
    model = cls()
    ref64 = copy.deepcopy(model).double()

    def make(v):
        g = torch.Generator().manual_seed(60 + v)
        x = torch.rand(B, 1, hw, hw, generator=g) * 2 - 1
        return x, torch.eye(n)[torch.randint(0, n, (B,), generator=g)]
    x, y = tie_free([ref64], make, lambda x, y: ref64(x.double())) if name == "mnist" else make(0)
    return model, x, y


def _reference_step(model, x, y, dtype):
    m = copy.deepcopy(model).to(dtype)
    opt = torch.optim.Adam(m.parameters(), lr=LR)
    opt.zero_grad()
    pred = m(x.to(dtype))
    loss = nn.CrossEntropyLoss()(pred, y.to(dtype))
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    opt.step()
    return m, pred.detach(), loss.detach(), grads


@gpu
@pytest.mark.parametrize("name", ["mnist", "audio", "whale"])
def test_forward_and_one_stepper_step_vs_fp64(name):
    from ali_hip.classify import ClassifierStepper
    model, x, y = _family(name)
    m64, pred64, loss64, g64 = _reference_step(model, x, y, torch.float64)
    m32, pred32, loss32, g32 = _reference_step(model, x, y, torch.float32)
    dev = copy.deepcopy(model).cuda()
    with torch.no_grad():
        _check(f"{name} logits", dev(x.cuda()), pred64, pred32)
    before = {k: v.detach().cpu().clone() for k, v in dev.state_dict().items()}
    stepper = ClassifierStepper(dev, lr=LR)
    r = stepper.step(x.cuda(), y.cuda())
    _check(f"{name} loss", r["loss"], loss64, loss32)
    assert r["hits"].item() == (pred64.argmax(1) == y.argmax(1)).sum().item()
    for k, p in dev.named_parameters():
        gd = stepper.opt.grad_views[id(p)].detach().cpu()
        if name == "mnist":
            _check(f"{name} {k}.grad", gd, g64[k], g32[k])
        else:
            print(f"CLF {name} {k}.grad e_dev={(gd.double() - g64[k]).abs().max().item():.3e} "
                  f"e_cpu={(g32[k].double() - g64[k]).abs().max().item():.3e} scale={g64[k].abs().max().item():.3e}")
            assert torch.isfinite(gd).all()
        g = gd.double()
        want = before[k].double() - LR * (g / (g.abs() + 1e-8))          # Adam's first step at the device's gradient
        err = (p.detach().cpu().double() - want).abs().max().item()
        bound = 1e-6 * LR + 6e-8 * before[k].abs().max().item()
        print(f"CLF {name} {k} update err={err:.3e} bound={bound:.3e}")
        assert err <= bound, (name, k, err, bound)
    _check_encoder_update(m64.float(), dev, before, LR, 1)


@gpu
def test_input_gradient_of_the_mnist_classifier():
    """what HingeLossCFExplainer needs (explain/cf_example.py): d sum(clf(x) * cot) / dx through ``run_chain``"""
    model, x, _ = _family("mnist")
    cot = torch.randn(x.shape[0], 10, generator=torch.Generator().manual_seed(3))
    compare_with_autograd(model, x, cot, "mnist")


@gpu
@pytest.mark.parametrize("name", ["mnist", "audio"])
def test_captured_and_eager_steps_agree_bit_for_bit(name):
    from ali_hip.classify import ClassifierStepper
    model, x, y = _family(name)
    xs = [x.cuda(), (x * 0.5).cuda(), (-x).cuda()]
    out = []
    for capture in (False, True):
        dev = copy.deepcopy(model).cuda()
        stepper = ClassifierStepper(dev, lr=LR, capture=capture)
        res = []
        for xi in xs:
            r = stepper.step(xi, y.cuda())
            res.append((r["loss"].clone(), r["hits"].clone()))
        out.append((res, [p.detach().clone() for p in dev.parameters()], int(stepper.opt.step_t.item())))
        if capture:
            assert len(stepper._graphs) == 1
    (res_e, w_e, n_e), (res_c, w_c, n_c) = out
    assert n_e == n_c == 3
    for (le, he), (lc, hc) in zip(res_e, res_c):
        assert torch.equal(le, lc) and torch.equal(he, hc)
    for a, b in zip(w_e, w_c):
        assert torch.equal(a, b)


@gpu
def test_checkpoint_saved_from_the_cpu_module_gives_the_same_logits(tmp_path):
    model, x, _ = _family("mnist")
    torch.save({"model": model}, tmp_path / "clf.tar")
    back = torch.load(tmp_path / "clf.tar", map_location="cuda", weights_only=False)["model"]
    assert next(back.parameters()).is_cuda
    with torch.no_grad():
        _check("checkpoint logits", back(x.cuda()), copy.deepcopy(model).double()(x.double()), model(x))


SCORE_SEED = 9


def _score_case(R):
    """MNIST generator (oracle weights of test_gpu_modules.paired_models) + a freshly initialised classifier, B = 32;
    returns the fp64 and CPU-fp32 logits of the mc-round mean image."""
    from classifiers.mnist import MNISTClassifier
    (_, Go, _), (_, G, _), _, c, _ = paired_models("mnist", B=32)
    torch.manual_seed(SCORE_SEED)
    clf = MNISTClassifier()
    zs = torch.randn(R, 32, 512, 1, 1, generator=torch.Generator().manual_seed(SCORE_SEED + R))
    logits = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            Gd, cd = copy.deepcopy(Go).to(dt).eval(), {k: v.to(dt) for k, v in c.items()}
            gen = sum(Gd(zs[r].to(dt), cd) for r in range(R)) / R
            logits[dt] = copy.deepcopy(clf).to(dt)(gen)
    return G.eval(), clf, c, zs, logits


def _left_out(l64):
    top = l64.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < 1e-3 * l64.abs().max()


@gpu
@pytest.mark.parametrize("R", [1, 3])
def test_generator_score_counters_equal_the_fp64_count(R):
    """``GeneratorScore`` / ``ClassifierScorer`` on MNIST, B = 32, mc_rounds = R: the device counters equal the count of
    the fp64 restatement of audiomnist_generator_score.py:83-98.  A row whose fp64 top-two logit gap is below
    1e-3 * max|logit| may be left out (at most 1 in 32).  SCORE_SEED = 9 was picked on the CPU so that NO row is
    left out for R = 1 and R = 3 and the CPU-fp32 restatement predicts every row like fp64 (both asserted below), so the
    comparison is exact.  ``add`` twice then ``result`` is the sum of both batches; ``reset`` clears it."""
    from ali_hip.classify import ClassifierScorer, GeneratorScore
    G, clf, c, zs, logits = _score_case(R)
    l64 = logits[torch.float64]
    out = _left_out(l64)
    assert int(out.sum()) <= 1
    assert int(out.sum()) == 0 and torch.equal(l64.argmax(1), logits[torch.float32].argmax(1)), "pick another SCORE_SEED"
    want = int((l64.argmax(1) == c["digit"].argmax(1)).sum())
    clf_d = copy.deepcopy(clf).cuda()
    score = GeneratorScore(G, {"digit": clf_d}, mc_rounds=R)
    gen = score.add(to_dev(c), zs.cuda())
    assert score.result() == {"digit": want / 32}
    score.add(to_dev(c), zs.cuda())
    assert score.scorer.counters.tolist() == [2 * want] and score.result() == {"digit": want / 32}
    assert len(score._graphs) == 1
    score.reset()
    assert score.scorer.counters.tolist() == [0] and score.scorer.seen == 0
    # the scorer on its own, fed the image the graph produced; a second, different classifier beside the first
    torch.manual_seed(SCORE_SEED + 100)
    other = type(clf)()
    with torch.no_grad():
        lo = copy.deepcopy(other).double()(gen.detach().cpu().double())
    assert int(_left_out(lo).sum()) == 0, "pick another SCORE_SEED"
    want_o = int((lo.argmax(1) == c["digit"].argmax(1)).sum())
    scorer = ClassifierScorer({"digit": clf_d, "other": other.cuda()})
    labels = {"digit": c["digit"].cuda(), "other": c["digit"].cuda()}
    scorer.add(gen, labels)
    scorer.add(gen, labels)
    assert scorer.result() == {"digit": want / 32, "other": want_o / 32}
    assert scorer.counters.tolist() == [2 * want, 2 * want_o]
    scorer.reset()
    assert scorer.result() == {"digit": 0.0, "other": 0.0}
