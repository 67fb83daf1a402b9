"""The bits of the four explainer executors (``ali_hip.explain.HingeCFStepper`` / ``MixtureSweep``,
``ali_hip.attrib.ExpectedGradients``, ``ali_hip.contrast.ContrastiveSearch``) through their public surfaces.  The other
tests of these executors compare with fp64 within a tolerance and captured with eager runs of the same code; a change
of a launch, of its order or of one of its arguments between the decoder's input rows and the data gradient can pass
both.  This one compares the raw bits of every output with ``tests/golden/explainer_bits.npz``.

The golden file is recorded on an MI355X at the commit it names (``commit`` inside it, next to ``torch``, the
``torch.__version__`` of the recording), with ``python tests/test_gpu_explainer_bits.py --record [--commit NAME] [--out
PATH]``, in the manner of test_gpu_reduce_bits.py (whose ``bits`` and ``entry`` it uses: outputs of up to 64 elements
whole, larger ones as a 64-bit blake2b checksum).  Recording it again is legitimate where a kernel or a launch of these
paths changes on purpose, or after a ROCm upgrade that changes the device's ``exp`` / ``tanh``; a change of the Python
that schedules the same launches must reproduce it.

Module weights come from ``torch.manual_seed`` on the CPU generator, as in test_gpu_explain.py; inputs are closed forms
or draws of a seeded CPU generator, and nothing on the host reduces (no encoder pass: the codes are draws).  Every case
runs eager and captured, twice each -- the second time on the same executor (the captured one then replays the graph
it holds) except where a call moves the executor's RNG counter, which get a fresh executor.  The four runs must give
equal bits, and those bits must be the recorded ones.  The cases are the smallest that reach each branch; they are
listed at the case functions.

The contrastive cases' ``learning_rate``, ``kappa`` and ``c0`` (``CT_HYPER``) were chosen so that over the four cases at
least one row ends found and one does not; the recorder refuses to write the file otherwise and the last test asserts
it of what it computed."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_reduce_bits import WHOLE, bits, entry

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explainer_bits.npz")
LR = 0.1
# the fp32 statement on the CPU: "ce" finds every row, "pn" rows 1 and 2 but not row 0, the same for c0 from 70 to 100
CT_HYPER = dict(num_iterations=3, binary_search_steps=2, learning_rate=0.1, kappa=0.0, c0=85.0)

_MODELS = {}


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _models(kind):
    """seeded CPU modules in eval mode, built once; the executors get copies on the device"""
    if kind not in _MODELS:
        if kind == "mnist":
            import image_scms.mnist as pm
            from classifiers.mnist import MNISTClassifier
            torch.manual_seed(0)
            _MODELS[kind] = (pm.Generator().eval(), MNISTClassifier().eval())
        else:
            import image_scms.audio_mnist as pm
            from classifiers.audio_mnist import AudioMNISTClassifier
            torch.manual_seed(3)
            _MODELS[kind] = (pm.Generator(8).eval(), AudioMNISTClassifier(10).eval())
    return tuple(copy.deepcopy(m).cuda() for m in _MODELS[kind])


# ------------------------------------------------------------------------------------------------------- the cases
# Each is (make(capture) -> executor, body(executor) -> {name: tensor}, fresh): ``fresh`` cases get a new executor for
# every run.
def _mnist_batch(B, seed, ignored):
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(B, 1, 28, 28, generator=g))
    digit = torch.zeros(B, 10)
    digit[torch.arange(B), torch.randint(0, 10, (B,), generator=g)] = 1.0
    attrs = {"digit": digit}
    for k in ("thickness", "intensity", "slant"):
        attrs[k] = torch.rand(B, 1, generator=g) * 2 - 1
    init = {k: 0.3 * torch.randn(B, attrs[k].shape[1], generator=g) for k in attrs if k not in ignored}
    init["z"] = torch.randn(B, 512, 1, 1, generator=g)
    codes = torch.randn(B, 512, 1, 1, generator=g)
    target = torch.randint(0, 10, (B,), generator=g)
    return x, attrs, init, codes, target


def _hinge_outputs(stepper, attrs, B, update_z, result):
    x_cf, attrs_cf, out3 = result
    out = {"x_cf": x_cf, "out3": out3}
    out.update({"attr_" + k: v for k, v in attrs_cf.items()})
    var = stepper.variables(attrs, True, update_z, B=B)
    out["step"] = var["step"].clone()
    for k, views in var.items():
        if k not in ("step", "probe"):
            out.update({f"{n}_{k}": t.clone() for n, t in views.items()})
    return out


def hinge_mnist(which):
    """"fixed_z": B = 3, 3 steps, slant ignored, targets, tanh(init z) given; "trained_z": the same with z a variable;
    "no_given": B = 2, 2 steps, nothing ignored and z trained (no given column), no target (the rows are compared with
    the classifier's softmax of x), x one image for all rows"""
    from ali_hip.explain import HingeCFStepper
    B, steps, ignored = (2, 2, []) if which == "no_given" else (3, 3, ["slant"])
    update_z = which != "fixed_z"
    x, attrs, init, codes, target = _mnist_batch(B, 40 + B, ignored)
    if which == "no_given":
        x, target = x[:1], None

    def make(capture):
        G, clf = _models("mnist")
        return HingeCFStepper(G, clf, "digit", ["digit"], ignored, c=10.0, capture=capture)

    def body(stepper):
        a = _cuda(attrs)
        r = stepper.run(x.cuda(), a, codes.cuda(), None if target is None else target.cuda(), _cuda(init), steps, LR,
                        True, update_z=update_z)
        return _hinge_outputs(stepper, a, B, update_z, r)
    return make, body, False


def hinge_spect():
    """the spectrogram stacks (SpectGenerator with six tables, the AudioMNIST classifier), B = 2, one step"""
    import image_scms.audio_mnist as pm
    from ali_hip.explain import HingeCFStepper
    B = 2
    g = torch.Generator().manual_seed(6)
    x = torch.clip(torch.randn(B, 1, 128, 128, generator=g), -3, 3) / 3
    attrs = {k: torch.eye(n)[torch.randint(0, n, (B,), generator=g)] for k, n in pm.ATTRIBUTE_DIMS.items()}
    codes = torch.randn(B, 512, 1, 1, generator=g)
    keys = list(attrs)
    ignored = [keys[1]]
    init = {k: 0.3 * torch.randn(B, attrs[k].shape[1], generator=g) for k in keys if k not in ignored}
    init["z"] = torch.randn(B, 512, 1, 1, generator=g)
    target = torch.tensor([4, 7])

    def make(capture):
        G, clf = _models("spect")
        return HingeCFStepper(G, clf, "digit", keys, ignored, c=10.0, capture=capture)

    def body(stepper):
        a = _cuda(attrs)
        r = stepper.run(x.cuda(), a, codes.cuda(), target.cuda(), _cuda(init), 1, LR, True, update_z=True)
        return _hinge_outputs(stepper, a, B, True, r)
    return make, body, False


def sweep(metric, orig):
    """S = 8 mixture rows towards class 3; ``orig`` None (the classifier's pass over x is part of the graph) or given"""
    from ali_hip.explain import MixtureSweep
    x, attrs, _, codes, _ = _mnist_batch(1, 2, [])

    def make(capture):
        G, clf = _models("mnist")
        return MixtureSweep(G, clf, "digit", capture=capture)

    def body(sw):
        o = None if orig is None else torch.tensor([orig], dtype=torch.int32, device="cuda")
        return dict(sw.run(x.cuda(), codes.cuda(), _cuda(attrs), 3, 8, metric, orig=o))
    return make, body, False


EG_R, EG_S, EG_ND, EG_NB = 3, 3, 2, 4


def _eg_inputs():
    def rows(n, g):
        a = torch.zeros(n, 13)
        a[torch.arange(n), torch.randint(0, 10, (n,), generator=g)] = 1.0
        a[:, 10:] = torch.rand(n, 3, generator=g) * 2 - 1
        return a
    g = torch.Generator().manual_seed(7)
    x, bg = rows(EG_R, g), rows(EG_NB, g)
    draws = {"idx": torch.randint(0, EG_NB, (EG_R, EG_S), generator=g), "t": torch.rand(EG_R, EG_S, generator=g),
             "z": torch.randn(EG_R, EG_S, EG_ND, 512, generator=g)}
    return x, bg, draws


def _eg_make(bg, **kw):
    from ali_hip.attrib import ExpectedGradients

    def make(capture):
        G, clf = _models("mnist")
        return ExpectedGradients(G, clf, bg.cuda(), n_draws=EG_ND, nsamples=EG_S, capture=capture, **kw)
    return make


def eg(which):
    """R = 3 rows, 3 samples, 2 draws of z, 4 background rows.  "explicit": given draws, all classes, one chunk;
    "chunked": the same with rows_per_launch=2 (chunks of 2 + 1 rows); "drawn": two calls that draw on the device at
    seed 5 (the second under the advanced counter)"""
    x, bg, draws = _eg_inputs()
    if which == "drawn":
        def body(ex):
            return {"phi_first": ex.shap_values(x.cuda()), "phi_second": ex.shap_values(x.cuda())}
        return _eg_make(bg, seed=5), body, True

    def body(ex):
        return {"phi": ex.shap_values(x.cuda(), draws=_cuda(draws))}
    return _eg_make(bg, **({"rows_per_launch": 2} if which == "chunked" else {})), body, False


def eg_value():
    """f(a) at the given z and at z drawn on the device (seed 5)"""
    x, bg, draws = _eg_inputs()

    def body(ex):
        return {"given_z": ex.value(x.cuda(), draws["z"][:, 0].cuda()), "drawn_z": ex.value(x.cuda())}
    return _eg_make(bg, seed=5), body, True


def contrastive(mode, bounded):
    """B = 3 searches on the MNIST classifier, 3 iterations, 2 rounds: 8 replays; the rows' own bounds or (-1, 1)"""
    from ali_hip.contrast import ContrastiveSearch
    x = torch.rand(3, 1, 28, 28, generator=torch.Generator().manual_seed(1)) * 2 - 1

    def make(capture):
        return ContrastiveSearch(_models("mnist")[1], mode, capture=capture,
                                 bounds=(-1.0, 1.0) if bounded else None, **CT_HYPER)

    def body(search):
        st = search.start(x.cuda())
        search.advance(search.replays_per_search)
        out = dict(search.result())
        out.update({k: st[k].clone() for k in ("it", "rnd", "ctab")})
        return out
    return make, body, False


CASES = {}
for _fn, _params in ((hinge_mnist, [("fixed_z",), ("trained_z",), ("no_given",)]), (hinge_spect, [()]),
                     (sweep, [("mixture", None), ("mse", None), ("ssim", None), ("mse", 5)]),
                     (eg, [("explicit",), ("chunked",), ("drawn",)]), (eg_value, [()]),
                     (contrastive, [("pn", False), ("pn", True), ("ce", False), ("ce", True)])):
    for _p in _params:
        CASES["-".join([_fn.__name__] + [str(v) for v in _p])] = (_fn, _p)
CONTRASTIVE = [n for n in CASES if n.startswith("contrastive-")]

_RESULTS = {}


def run_case(name):
    """the case's outputs as {name/output: bits}: eager and captured, twice each, equal bits asked for (computed once)"""
    if name in _RESULTS:
        return _RESULTS[name]
    fn, params = CASES[name]
    make, body, fresh = fn(*params)
    runs = []
    for capture in (False, True):
        ex = make(capture)
        for again in range(2):
            if fresh and again:
                ex = make(capture)
            runs.append({k: bits(t) for k, t in body(ex).items()})
    for what, other in zip(("a second eager run", "the captured run", "a second captured run"), runs[1:]):
        assert sorted(other) == sorted(runs[0]), name
        for k in runs[0]:
            assert np.array_equal(runs[0][k], other[k]), f"{name}/{k}: {what} gives other bits than the first eager run"
    _RESULTS[name] = {f"{name}/{k}": a for k, a in runs[0].items()}
    return _RESULTS[name]


def found_and_not_found(results):
    """(rows that ended found, rows that did not) over the contrastive cases of {name/output: bits}"""
    found = np.concatenate([results[n + "/found"] for n in CONTRASTIVE])
    return int((found != 0).sum()), int((found == 0).sum())


_GOLD = {}


def golden():
    if not _GOLD:
        with np.load(GOLDEN) as z:
            _GOLD.update({k: z[k] for k in z.files})
    return _GOLD


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bits_are_the_recorded_ones(name):
    gold = golden()
    got = run_case(name)
    assert sorted(k for k in gold if k.startswith(name + "/")) == sorted(got), name
    for k, a in got.items():
        e, want = entry(a), gold[k]
        what = "bits" if a.size <= WHOLE else f"checksum of {a.size} elements"
        assert e.dtype == want.dtype and np.array_equal(e, want), \
            f"{k}: {what} {e.tolist()} differ from the recorded {want.tolist()} (commit {gold['commit']}, " \
            f"torch {gold['torch']}; this is torch {torch.__version__})"


@gpu
def test_contrastive_cases_end_found_and_not_found():
    results = {}
    for name in CONTRASTIVE:
        results.update(run_case(name))
    n_found, n_not = found_and_not_found(results)
    assert n_found >= 1 and n_not >= 1, (n_found, n_not)


def record(path, commit):
    out = {"commit": np.array(commit), "torch": np.array(torch.__version__),
           "device": np.array(torch.cuda.get_device_name(0))}
    results = {}
    for name in CASES:
        results.update(run_case(name))
    for k, a in results.items():
        out[k] = entry(a)
        print(f"{k}: {a.size} elements -> {out[k].tolist() if a.size <= WHOLE else '(checksum)'}")
    n_found, n_not = found_and_not_found(results)
    assert n_found >= 1 and n_not >= 1, \
        f"the contrastive cases end with {n_found} rows found and {n_not} not found: choose other CT_HYPER"
    np.savez_compressed(path, **out)
    print(f"recorded {len(results)} outputs of {len(CASES)} cases at {commit} (torch {torch.__version__}) into {path} "
          f"({os.path.getsize(path)} bytes); contrastive rows found {n_found}, not found {n_not}")


if __name__ == "__main__":
    import argparse
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "imagecfgen-pytorch_amd"))
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", default=None, help="default: git rev-parse --short HEAD")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    if a.commit is None:
        import subprocess
        a.commit = subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], text=True).strip()
    assert torch.cuda.is_available(), "recording needs the GPU"
    record(a.out, a.commit)
