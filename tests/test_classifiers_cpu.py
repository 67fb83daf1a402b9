"""The classifier family without a GPU: stage parsing and routing of ``Flatten -> Linear``, the drop-in classes
(``state_dict`` keys and shapes of the reference's ``classifiers/*.py``, output shapes, pickles), the executors of
``ali_hip.classify`` on CPU tensors against the plain torch loop, and the host-side checks of ``ali_softmax_xent``."""
import ctypes
import io

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


def _stack(flatten=True):
    mods = [nn.Conv2d(1, 8, 3), nn.LeakyReLU(0.2), nn.Conv2d(8, 12, 3, 2), nn.LeakyReLU(0.2)]
    if flatten:
        mods += [nn.Flatten(), nn.Linear(240, 7), nn.LeakyReLU(0.2), nn.Linear(7, 5)]
    return nn.Sequential(*mods)


def test_flatten_linear_parses_into_a_gemm_stage():
    from ali_hip import chain
    from ali_hip.ops import ACT_LEAKY, ACT_NONE
    seq = _stack()
    plan = chain.get_plan(seq)
    assert [st.kind for st in plan.stages] == ["conv", "conv", "flat", "linear"]
    assert [st.act for st in plan.stages] == [ACT_LEAKY, ACT_LEAKY, ACT_LEAKY, ACT_NONE]
    assert plan.stages[2].mod is seq[5] and plan.stages[3].mod is seq[7]
    assert [id(p) for p in plan.params()] == [id(p) for p in seq.parameters()]
    tr = chain.trace(plan, (3, 11, 14, 4), 1)
    assert [t[1] for t in tr] == [(3, 9, 12, 8), (3, 4, 5, 12), (3, 1, 1, 7), (3, 1, 1, 5)]
    rt = tr[2][2]
    assert (rt.fwd, rt.wgrad, rt.dgrad) == ("conv", ("conv", "fused"), "conv")
    assert plan.stages[2].hw == (4, 5)
    g = chain._geom(plan.stages[2], tr[2][0], tr[2][1])
    assert (g.B, g.H, g.W, g.C, g.P, g.Q, g.K, g.R, g.S, g.stride, g.pad) == (3, 4, 5, 12, 1, 1, 7, 4, 5, 1, 0)
    assert plan.out_channels == 5


def test_a_stack_without_flatten_is_parsed_and_routed_as_before():
    """the convolution stages of the stack with and without the Flatten tail: same kinds, shapes and Routes, and the
    Routes are what the rules of ``route`` give for plain Conv2d stages (computed here, not stored)"""
    from ali_hip import chain
    plain, full = chain.get_plan(_stack(False)), chain.get_plan(_stack(True))
    a, b = chain.trace(plain, (3, 11, 14, 4), 1), chain.trace(full, (3, 11, 14, 4), 1)
    assert a == b[:2]
    assert [st.kind for st in plain.stages] == ["conv", "conv"]
    for i, (cin, cout, route) in enumerate(a):
        first = i == 0
        want = chain.Route(fwd="conv", wgrad=("conv", "fused"), wgrad_fold=("conv", "fused"), dgrad="conv",
                           planes="scatter" if first else None, fold_ok=True, bn_leave=True, bn_reduce=True)
        assert route == want, (i, route)
    # the first classifier layer, Conv2d(1, 32, 3) with one real input channel: the direct weight-gradient route
    first = chain.trace(chain.get_plan(nn.Sequential(nn.Conv2d(1, 32, 3), nn.LeakyReLU(0.2))), (8, 28, 28, 4), 1)[0][2]
    assert first.wgrad == ("first_direct", "colsum") and first.planes == "direct"


def test_flatten_misuse_is_rejected():
    from ali_hip import chain
    bad = nn.Sequential(nn.Conv2d(1, 8, 3), nn.LeakyReLU(0.2), nn.Flatten(), nn.Linear(241, 7))
    with pytest.raises(ValueError, match="in_features=241"):
        chain.trace(chain.get_plan(bad), (3, 8, 7, 4), 1)
    for seq in (nn.Sequential(nn.Conv2d(1, 8, 3), nn.Flatten()),
                nn.Sequential(nn.Conv2d(1, 8, 3), nn.Flatten(), nn.LeakyReLU(0.2), nn.Linear(8, 2)),
                nn.Sequential(nn.Conv2d(1, 8, 3), nn.Flatten(0), nn.Linear(8, 2)),
                nn.Sequential(nn.Conv2d(1, 8, 3), nn.Flatten(1, 2), nn.Linear(8, 2))):
        with pytest.raises(NotImplementedError, match="Flatten"):
            chain.ChainPlan(seq)


def _conv_keys(widths):
    out, cin = [], 1
    for i, co in enumerate(widths):
        out += [(f"{2 * i}.weight", (co, cin, 3, 3)), (f"{2 * i}.bias", (co,))]
        cin = co
    return out


MNIST_KEYS = _conv_keys([32, 64, 128, 256]) + [("9.weight", (10, 4096)), ("9.bias", (10,))]
AUDIO_KEYS = _conv_keys([32, 64, 128, 256, 512, 1024, 1024]) + [
    ("15.weight", (1024, 4096)), ("15.bias", (1024,)), ("17.weight", (10, 1024)), ("17.bias", (10,))]
WHALE_KEYS = _conv_keys([32, 64, 128, 256, 512, 1024, 1024, 1024]) + [
    ("17.weight", (1024, 4096)), ("17.bias", (1024,)), ("19.weight", (3, 1024)), ("19.bias", (3,))]


def _classes():
    from classifiers import audio_mnist, mnist, whalecalls
    return [(mnist.MNISTClassifier, MNIST_KEYS, 28, 10), (audio_mnist.AudioMNISTClassifier, AUDIO_KEYS, 128, 10),
            (whalecalls.NARWClassifier, WHALE_KEYS, 256, 3)]


def test_classes_have_the_reference_state_dict_and_output_shapes():
    from classifiers import audio_mnist, training_utils
    for cls, keys, hw, n in _classes():
        model = cls()
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys, cls.__name__
        assert isinstance(model, nn.Sequential)
        with torch.no_grad():
            assert model(torch.zeros(2, 1, hw, hw)).shape == (2, n)
    assert audio_mnist.AudioMNISTClassifier(num_classes=60)[17].out_features == 60
    assert audio_mnist.ATTRIBUTE_DIMS == {"country_of_origin": 13, "native_speaker": 2, "accent": 15, "digit": 10,
                                          "age": 5, "gender": 2}
    assert audio_mnist.VALIDATION_RUNS == [38, 7, 42, 10, 14, 18, 20, 22, 28]
    parts = list(training_utils.batchify(torch.arange(10), torch.arange(12), batch_size=4))
    assert [len(a) for a, _ in parts] == [4, 4, 2] and torch.equal(parts[2][0], torch.tensor([8, 9]))


def test_pickled_model_dict_round_trip():
    from classifiers.mnist import MNISTClassifier
    model = MNISTClassifier()
    from ali_hip import chain
    chain.get_plan(model)                       # (a plan exists: it must not travel with, or break, the pickle)
    buf = io.BytesIO()
    torch.save({"model": model}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)["model"]
    assert type(back) is MNISTClassifier
    x = torch.randn(2, 1, 28, 28)
    with torch.no_grad():
        assert torch.equal(back(x), model(x))


def test_stepper_and_scorer_on_cpu_tensors_equal_the_plain_loop():
    import copy
    from ali_hip.classify import ClassifierScorer, ClassifierStepper
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(5)
    model = MNISTClassifier()
    ref = copy.deepcopy(model)
    xs = torch.randn(3, 6, 1, 28, 28)
    ys = torch.eye(10)[torch.randint(0, 10, (3, 6))]
    ys[1] = torch.softmax(torch.randn(6, 10), 1)                    # soft rows
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    crit = nn.CrossEntropyLoss()
    stepper = ClassifierStepper(model, lr=1e-4)
    for x, y in zip(xs, ys):
        opt.zero_grad()
        pred = ref(x)
        loss = crit(pred, y)
        loss.backward()
        opt.step()
        r = stepper.step(x, y)
        assert r["loss"].dim() == 0 and r["hits"].dim() == 0
        torch.testing.assert_close(r["loss"], loss.detach(), rtol=1e-6, atol=0)
        assert r["hits"].item() == (pred.argmax(1) == y.argmax(1)).sum().item()
    for a, b in zip(model.parameters(), ref.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9)
    other = MNISTClassifier()
    scorer = ClassifierScorer({"digit": model, "other": other})
    want = {"digit": 0, "other": 0}
    with torch.no_grad():
        for x, y in zip(xs, ys):
            scorer.add(x, {"digit": y, "other": y, "unused": y})
            for k, m in (("digit", ref), ("other", other)):
                want[k] += (y.argmax(1) == m(x).argmax(1)).sum().item()
    assert scorer.result() == {k: v / 18 for k, v in want.items()}
    scorer.reset()
    assert scorer.seen == 0 and scorer.result() == {"digit": 0.0, "other": 0.0}


def test_softmax_xent_rejects_bad_class_counts_before_any_launch():
    import ali_hip
    lib = ali_hip.load()
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for C in (0, 4097, -3):
        rc = lib.ali_softmax_xent(ptr, ptr, 1, C, 1.0, ptr, None, None, None, None, 0, None)
        assert rc < 0
        msg = lib.ali_last_error().decode()
        assert "ali_softmax_xent" in msg and str(C) in msg
    assert lib.ali_softmax_xent(ptr, ptr, 0, 10, 1.0, ptr, None, None, None, None, 0, None) < 0
    assert lib.ali_softmax_xent(ptr, ptr, 2, 4, 1.0, ptr, None, None, None, None, 0, None) == -2      # no workspace
    assert "workspace" in lib.ali_last_error().decode()
