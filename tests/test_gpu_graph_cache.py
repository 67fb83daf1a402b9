"""Graph replay per input signature, through the public calls of every class that has one (``ali_hip.graphs``).

What is pinned here is the protocol, not the arithmetic (the per-family files do that): a captured call equals the eager
one bit for bit, the warm-up pass counts as no step / batch / call, an optional argument given or not selects another
graph, and an inference cache is dropped when a watched parameter is written.  Everything is ``torch.equal``; the
smallest models the per-family files build (MNIST pair at B = 4, GAN ``models(4, .)`` at B = 2, ``_gl``)."""
import copy

import pytest
import torch

from test_gpu_gans import BETAS, LR, _same_state, make_draws, models
from test_gpu_griffinlim import _gl
from test_gpu_modules import paired_models, to_dev
from test_griffinlim_cpu import SHAPES, inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("metric", ["mse", "ssim"])
def test_finetune_captured_steps_equal_the_eager_ones(metric):
    from ali_hip.step import FinetuneStepper
    out = []
    for capture in (False, True):
        _, (E, G, _), images, c, _ = paired_models("mnist", d=64, B=4)
        E.train(), G.eval()
        ft = FinetuneStepper(E, G, lr=1e-4, capture=capture, metric=metric)
        res = []
        for s in (1.0, 0.5, -1.0):
            r = ft.step((images * s).cuda(), to_dev(c))
            res += [r["rec"].clone(), r["latent"].clone()]
        assert int(ft.opt_e.step_t.item()) == 3                 # the warm-up pass counted as no step
        out.append(res + [p.detach().clone() for p in E.parameters()] + [ft.opt_e.m, ft.opt_e.v, ft.opt_e.step_t])
        if capture:
            assert len(ft._graphs) == 1
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_sampler_drops_its_graph_when_a_parameter_is_written():
    from ali_hip.step import GeneratorSampler
    _, (_, G, _), _, c, _ = paired_models("mnist", d=64, B=4)
    G.eval()
    zs = torch.randn(3, 4, 512, 1, 1, generator=torch.Generator().manual_seed(17)).cuda()
    cd = to_dev(c)
    graphed, eager = GeneratorSampler(G), GeneratorSampler(G, capture=False)
    first = graphed(zs, cd).clone()
    assert torch.equal(graphed(zs, cd), first) and len(graphed._graphs) == 1
    assert torch.equal(first, eager(zs, cd))
    with torch.no_grad():
        next(G.parameters()).mul_(1.0)
    assert torch.equal(graphed(zs, cd), first) and len(graphed._graphs) == 1       # recorded again, not added
    with torch.no_grad():
        next(G.layers.parameters()).mul_(0.5)
    got = graphed(zs, cd).clone()
    assert len(graphed._graphs) == 1 and not torch.equal(got, first)
    assert torch.equal(got, eager(zs, cd))


def test_scorer_drops_its_graph_when_a_parameter_is_written():
    from classifiers.mnist import MNISTClassifier
    from ali_hip.classify import ClassifierScorer
    torch.manual_seed(9)
    clf = MNISTClassifier().cuda()
    g = torch.Generator().manual_seed(4)
    images = (torch.rand(4, 1, 28, 28, generator=g) * 2 - 1).cuda()
    labels = {"digit": torch.eye(10)[torch.randint(0, 10, (4,), generator=g)].cuda()}
    graphed, eager = ClassifierScorer({"digit": clf}), ClassifierScorer({"digit": clf}, capture=False)

    def both():
        graphed.add(images, labels)
        eager.add(images, labels)
        assert len(graphed._graphs) == 1
        assert graphed.counters.tolist() == eager.counters.tolist() and graphed.seen == eager.seen
    both()
    both()
    with torch.no_grad():
        next(clf.parameters()).mul_(1.0)
    both()
    with torch.no_grad():
        list(clf.parameters())[-1].add_(torch.linspace(-3, 3, 10).cuda())       # the last bias: other predictions
    both()
    assert graphed.seen == 16 and graphed.result() == eager.result()


def test_reconstructor_has_one_graph_per_combination_of_optional_arguments(golden_dir):
    from ali_hip.vae import VaeReconstructor
    from test_gpu_vae import case
    vae, _, x, c, _ = case("mnist", golden_dir)
    dev = copy.deepcopy(vae).cuda().eval()
    R, B = 3, x.shape[0]
    eps = torch.randn(R, B, 512, 1, 1, generator=torch.Generator().manual_seed(R)).cuda()
    xd, cd, cfd = x.cuda(), to_dev(c), to_dev(dict(c, digit=c["digit"].roll(1, 0)))
    graphed, eager = VaeReconstructor(dev, rounds=R), VaeReconstructor(dev, rounds=R, capture=False)
    drawn, seen = 0, []
    for n, (cf, e) in enumerate([(None, eps), (cfd, eps), (None, None), (cfd, None)]):
        got = graphed.add(xd, cd, cf, e).clone()
        assert len(graphed._graphs) == n + 1
        again = graphed.add(xd, cd, cf, e).clone()
        assert len(graphed._graphs) == n + 1
        assert got.shape == (B, 1, 28, 28) and bool(torch.isfinite(got).all())
        if e is not None:
            assert torch.equal(again, got) and torch.equal(got, eager.add(xd, cd, cf, e))
        else:
            drawn += 2
            assert not torch.equal(again, got)                  # the counter moved: new draws
        assert int(graphed.calls.item()) == drawn               # (the warm-up pass is no call)
        seen.append(got)
    assert not torch.equal(seen[0], seen[1])                    # the counterfactual attributes were read
    assert torch.equal(graphed.add(xd, cd, None, eps), seen[0]) and len(graphed._graphs) == 4


def test_gan_stepper_with_some_draws_given_and_some_made_on_the_device():
    from ali_hip.gan import GanStepper
    draws = [[t.cuda() for t in d] for d in make_draws(2, 77, steps=3)]
    out = []
    for capture in (False, True):
        G, D = models(4, 1)
        st = GanStepper(G.cuda(), D.cuda(), lr=LR, betas=BETAS, loss_mode="wgan", capture=capture, seed=5)
        res = []
        for images, z_g, z_d, z_s, eps in draws[:2]:
            res.append({k: v.clone() for k, v in st.step(images, z_d=z_d, eps=eps).items()})
        res.append({k: v.clone() for k, v in st.step(*draws[2]).items()})
        assert int(st.opt_d.step_t.item()) == 3 and int(st.iter_t.item()) == 3
        out.append((st, res))
    (eager, res_e), (graphed, res_c) = out
    assert len(graphed._graphs) == 2
    for a, b in zip(res_e, res_c):
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert _same_state(eager, graphed)


def _n_graphs(gl):
    """the graphs one GriffinLim instance holds (its cache; counted over its per-shape states where those hold them)"""
    if hasattr(gl, "_graphs"):
        return len(gl._graphs)
    return sum(len(st["graphs"]) for st in gl._states.values())


def test_griffinlim_has_one_graph_per_entry_point_and_shape():
    shape = SHAPES[0]
    spec, a0 = inputs(shape)
    Gg, Ge = _gl(shape, n_iter=4), _gl(shape, n_iter=4, capture=False)
    n = 0
    for T in (shape[4], shape[4] - 2):
        s, a = spec[..., :T].float().contiguous().cuda(), a0[..., :T].to(torch.complex64).contiguous().cuda()
        log_spec = (s + 1e-6).log()
        mean, std = log_spec.mean(dim=(0, 1)), log_spec.std(dim=(0, 1))
        img = torch.clip((log_spec - mean) / (std + 1e-6), -3, 3) / 3
        calls = [lambda G: G(s, a), lambda G: G.from_log(log_spec, a), lambda G: G.from_image(img, mean, std, angles0=a)]
        for call in calls if T == shape[4] else calls[:1]:
            want = call(Ge)
            n += 1
            assert torch.equal(call(Gg), want) and _n_graphs(Gg) == n
            assert torch.equal(call(Gg), want) and _n_graphs(Gg) == n       # a replay
    assert n == 4 and Gg.counter.item() == 0                                # given phases: nothing drawn
