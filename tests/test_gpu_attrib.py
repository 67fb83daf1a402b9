"""The executor ``ali_hip.attrib.ExpectedGradients`` and the drop-in surface of ``explain/attribute_shap.py`` on the
device.

Reference: the torch statement of the estimator (``ali_hip.attrib.eg_statement``: autograd) on the CPU in fp64 on
copies of the same modules; yardstick: the same statement in CPU fp32 (``_check`` of test_gpu_xent.py).  The thirteen
attribute columns of a class are a handful of numbers, so the classes are pooled as test_gpu_explain.py pools small
tensors (``_check_pooled``: each class scaled by its own max|ref64|).  The cases are seeded (``TieWatch``) so that the
fp64 forward has no LeakyReLU input within fp32 noise of zero: no row is left out.  Everything else is compared bit for
bit: a run restricted to one class against the full run (saved state damaged by the repeated backward passes would show
there), captured against eager, one chunk against ``rows_per_launch=1``, the modules' parameters and buffers before
and after."""
import copy

import pytest
import torch

from test_gpu_explain import _check_pooled
from test_gpu_modules import TieWatch
from test_gpu_xent import _check

gpu = pytest.mark.gpu

SLICES = {"digit": (0, 10), "thickness": (10, 1), "intensity": (11, 1), "slant": (12, 1)}
R, S, ND, NB = 2, 4, 2, 5
_CASES = {}


def _rows(n, g):
    a = torch.zeros(n, 13)
    a[torch.arange(n), torch.randint(0, 10, (n,), generator=g)] = 1.0
    a[:, 10:] = torch.rand(n, 3, generator=g) * 2 - 1
    return a


def _case(kind="G"):
    """modules, inputs, draws and both statements of a tie-free draw (computed once, shared, left unchanged)"""
    if kind in _CASES:
        return _CASES[kind]
    import image_scms.mnist as pm
    from ali_hip.attrib import eg_statement, value_statement
    from classifiers.mnist import MNISTClassifier
    from deepscm_vae.mnist import VAEDecoder
    torch.manual_seed(0 if kind == "G" else 3)
    G, clf = (pm.Generator() if kind == "G" else VAEDecoder()).eval(), MNISTClassifier().eval()
    G64, clf64 = copy.deepcopy(G).double(), copy.deepcopy(clf).double()
    for v in range(24):
        g = torch.Generator().manual_seed(100 * v + 7)
        x, bg = _rows(R, g), _rows(NB, g)
        idx = torch.randint(0, NB, (R, S), generator=g)
        t = torch.rand(R, S, generator=g)
        z = torch.randn(R, S, ND, 512, generator=g)
        with TieWatch(G64.layers, clf64) as tw:
            ref = eg_statement(G64, clf64, x.double(), bg.double(), idx, t.double(), z.double(), SLICES)
            val = value_statement(G64, clf64, x.double(), z[:, 0].double(), SLICES)
        if tw.ties == 0:
            break
    else:
        pytest.fail("no tie-free case in 24 draws")
    assert tw.ties == 0                                       # the chosen seed has no tie: no row is left out
    f32 = eg_statement(G, clf, x, bg, idx, t, z, SLICES)
    val32 = value_statement(G, clf, x, z[:, 0], SLICES)
    _CASES[kind] = dict(G=G, clf=clf, x=x, bg=bg, draws={"idx": idx, "t": t, "z": z}, ref=ref, f32=f32, val=val,
                        val32=val32)
    return _CASES[kind]


def _executor(case, **kw):
    from ali_hip.attrib import ExpectedGradients
    G, clf = copy.deepcopy(case["G"]).cuda(), copy.deepcopy(case["clf"]).cuda()
    kw.setdefault("capture", False)
    return ExpectedGradients(G, clf, case["bg"].cuda(), n_draws=ND, nsamples=S, **kw), G, clf


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


@gpu
@pytest.mark.parametrize("kind", ["G", "VAEDecoder"])
def test_phi_against_the_fp64_statement_and_parameter_safety(kind):
    case = _case(kind)
    ex, G, clf = _executor(case)
    before = {(i, k): v.clone() for i, m in enumerate((G, clf)) for k, v in m.state_dict().items()}
    phi = ex.shap_values(case["x"].cuda(), draws=_cuda(case["draws"]))
    assert phi.shape == (R, 10, 13) and phi.dtype == torch.float32 and phi.is_cuda
    ref, f32 = case["ref"], case["f32"]
    assert ref.abs().max().item() > 0
    _check_pooled(f"attrib phi {kind}", [(phi[:, c], ref[:, c], f32[:, c]) for c in range(10)])
    # the attribute dict gives the same bits as the rows
    as_dict = ex.shap_values({k: case["x"][:, o:o + w].cuda() for k, (o, w) in SLICES.items()},
                             draws=_cuda(case["draws"]))
    assert torch.equal(as_dict, phi)
    # parameter safety: weights and buffers bit for bit, no .grad anywhere
    after = {(i, k): v for i, m in enumerate((G, clf)) for k, v in m.state_dict().items()}
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for m in (G, clf) for p in m.parameters())


@gpu
def test_a_class_on_its_own_equals_the_full_run_bit_for_bit():
    case = _case()
    ex, _, _ = _executor(case)
    x, draws = case["x"].cuda(), _cuda(case["draws"])
    full = ex.shap_values(x, draws=draws)
    for c in (0, 4, 9):
        one = ex.shap_values(x, draws=draws, classes=[c])
        assert torch.equal(one[:, c], full[:, c]), c
        assert not one[:, [k for k in range(10) if k != c]].any()
    assert torch.equal(ex.shap_values(x, draws=draws), full)            # and the full run repeats itself


@gpu
def test_captured_equals_eager_replays_one_graph_and_drops_it_with_a_weight():
    case = _case()
    x, draws = case["x"].cuda(), _cuda(case["draws"])
    eager, _, _ = _executor(case)
    cap, _, clf = _executor(case, capture=True)
    want = eager.shap_values(x, draws=draws)
    got = cap.shap_values(x, draws=draws)
    assert torch.equal(got, want)
    assert len(cap._graphs) == 1
    first = next(iter(cap._graphs.entries.values()))
    other = torch.flip(case["x"], dims=[0]).cuda()                     # new a of the same signature: the one graph again
    got2 = cap.shap_values(other, draws=draws)
    assert len(cap._graphs) == 1 and next(iter(cap._graphs.entries.values())) is first
    assert torch.equal(got2, eager.shap_values(other, draws=draws)) and not torch.equal(got2, got)
    with torch.no_grad():                                              # a changed classifier weight drops the graph
        clf[0].weight.mul_(1.5)
        eager.classifier[0].weight.mul_(1.5)
    got3 = cap.shap_values(other, draws=draws)
    assert len(cap._graphs) == 1 and next(iter(cap._graphs.entries.values())) is not first
    assert torch.equal(got3, eager.shap_values(other, draws=draws)) and not torch.equal(got3, got2)


@gpu
@pytest.mark.parametrize("capture", [False, True])
def test_rows_per_launch_does_not_change_a_bit(capture):
    case = _case()
    x, draws = case["x"].cuda(), _cuda(case["draws"])
    whole, _, _ = _executor(case, capture=capture, seed=5)
    split, _, _ = _executor(case, capture=capture, seed=5, rows_per_launch=1)
    assert whole.default_rows_per_launch(whole._device_layout(x.device)) >= R          # one chunk
    assert torch.equal(split.shap_values(x, draws=draws), whole.shap_values(x, draws=draws))
    # ... nor what is drawn on the device: a chunk draws under its rows' own offsets
    a, b = whole.shap_values(x), split.shap_values(x)
    assert torch.equal(a, b)
    a2, b2 = whole.shap_values(x), split.shap_values(x)                                # the next call draws anew
    assert torch.equal(a2, b2) and not torch.equal(a2, a)


@gpu
def test_value_at_fixed_z():
    case = _case()
    z = case["draws"]["z"][:, 0].cuda()                                # [R, n_draws, 512]
    for capture in (False, True):
        ex, _, _ = _executor(case, capture=capture)
        val = ex.value(case["x"].cuda(), z)
        assert val.shape == (R, 10)
        _check(f"attrib value capture={capture}", val, case["val"], case["val32"])
        fresh = ex.value(case["x"].cuda())
        assert fresh.shape == (R, 10) and not torch.equal(fresh, val)
        assert torch.allclose(fresh.sum(dim=1).cpu(), torch.ones(R), atol=1e-5)


@gpu
def test_explain_all_in_batches_with_one_host_read(monkeypatch):
    from explain.attribute_shap import AttributeModel, GradientExplainer
    case = _case()
    G, clf = copy.deepcopy(case["G"]).cuda(), copy.deepcopy(case["clf"]).cuda()
    a_test = _rows(5, torch.Generator().manual_seed(3)).reshape(5, 1, 13).cuda()
    bg = case["bg"].reshape(NB, 1, 13).cuda()
    ex = GradientExplainer(AttributeModel(G, clf, ND), bg, seed=9)
    twin = GradientExplainer(AttributeModel(G, clf, ND), bg, seed=9).executor(S)
    per_batch = torch.cat([twin.shap_values(a_test[lo:lo + 2]) for lo in range(0, 5, 2)]).cpu().numpy()
    reads = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *args, _orig=orig, _name=name, **kw):
            if self.is_cuda:
                reads.append((_name, tuple(self.shape)))
            return _orig(self, *args, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    every = ex.explain_all(a_test, batch=2, nsamples=S)
    monkeypatch.undo()
    assert reads == [("cpu", (5, 10, 13))], reads                      # one host read, of the result, at the end
    assert every.shape == (5, 10, 13) and (every == per_batch).all()
    # the script's own line on one row
    import numpy as np
    vals = ex.shap_values(a_test[:1], nsamples=S)
    assert len(vals) == 10 and vals[0].shape == (1, 1, 13)
    assert np.array(vals).reshape((10, 13))[:, [10, 11, 12]].shape == (10, 3)
