"""Counterfactual explainers: the drop-in surface of the reference's ``explain/cf_example.py`` (same names, constructor
and ``explain`` signatures, defaults and return values), used by ``morphomnist_cf_metrics.py``, ``mnist_oracle_scores.py``,
``make_mnist_cf_matrix.py``, ``cf_automatic_mix.py`` and ``mnist_cf_comparisons.py``.

CUDA tensors with this package's generator stacks and a ``ClassifierStack`` run on the executors of
``ali_hip.explain`` (hand-scheduled steps on the HIP kernels, replayed from HIP graphs); CPU tensors, and models the
executors do not recognise, run the torch statement of the same loops.  The encoder is only ever called.

Corners of the reference that are kept, because callers and published numbers depend on them:

* ``HingeLossCFExplainer.explain`` draws ``0.01 * randn((1, n_k))`` per attribute that is not ignored, in ``attrs``
  order, on x's device, then -- with ``train_z`` -- ``randn(codes.shape)`` on the default device, moved to x's.
* That z is created after the other variables were marked trainable, so Adam never moves it: with ``train_z`` the
  generator's latent is ``tanh`` of the random draw, fixed over the loop.  ``explain_batch(update_z=True)`` optimises
  z as well.
* Without a target class the loss compares the classifier's logits of the counterfactual with its softmax of x.
* ``DeepCounterfactualExplainer.explain(metric='mixture')`` sorts a [n, 1] metric along its last axis, which yields
  zeros: it returns the first hit n times, ``samples`` [n, 1, ...] and the metric as [n, 1, 1].  With 'mse' / 'ssim'
  the metric is 1-D and the hits really come back sorted.  When nothing hits, all samples and the whole metric come
  back unsorted.

Beyond the reference: ``explain_batch`` of both classes (B independent explanations in one run).
"""
from typing import Dict, List, Optional, Tuple

import torch

from ali_hip.ssim import ssim


def progress(it):
    try:
        from tqdm import tqdm
    except ImportError:
        return it
    return tqdm(it)


def hinge(true, pred):
    return torch.relu(1 - true * pred)


def mse(a: torch.Tensor, b: torch.Tensor):
    d = a - b
    return d.square().mean(dim=list(range(1, d.dim())))


def max_excluding(y: torch.Tensor, c: int):
    """largest column of the one-row ``y`` other than column ``c`` (the first one on ties), as a [1] tensor"""
    best = float('-inf')
    for i in range(y.shape[1]):
        if i != c and y[:, i].item() > best:
            best = y[:, i]
    return best


def _executor(make):
    """the executor ``make()`` builds, or None for models it does not recognise"""
    try:
        return make()
    except TypeError:
        return None


def _on_device(x, *modules):
    return x.is_cuda and all(isinstance(m, torch.nn.Module) for m in modules)


class DeepCounterfactualExplainer:
    def __init__(self,
                 encoder: torch.nn.Module,
                 decoder: torch.nn.Module,
                 classifier: torch.nn.Module,
                 target_feature: str):
        self.encoder = encoder
        self.decoder = decoder
        self.classifier = classifier
        self.target_feature = target_feature
        self._sweep = None

    def _device_sweep(self, x):
        if not _on_device(x, self.decoder, self.classifier):
            return None
        if self._sweep is None:
            from ali_hip.explain import MixtureSweep
            self._sweep = _executor(lambda: MixtureSweep(self.decoder, self.classifier, self.target_feature)) or False
        return self._sweep or None

    def explain(self, x: torch.Tensor,
                attrs: Dict[str, torch.Tensor],
                target_class: int,
                sample_points=100,
                metric='mixture') -> Tuple[torch.Tensor, torch.Tensor]:
        sweep = self._device_sweep(x)
        if sweep is not None:
            return self._explain_device(sweep, x, attrs, target_class, sample_points, metric)
        return self._explain_torch(x, attrs, target_class, sample_points, metric)

    def explain_batch(self, x, attrs, target_class, sample_points=100, metric='mixture'):
        """``explain`` for every row of x / attrs: a list of its results.  ``target_class``: an int, or one per row.
        On the device every row replays the one recorded graph."""
        B = x.shape[0]
        targets = [int(t) for t in target_class] if hasattr(target_class, '__len__') else [int(target_class)] * B
        return [self.explain(x[b:b + 1], {k: v[b:b + 1] for k, v in attrs.items()}, targets[b], sample_points, metric)
                for b in range(B)]

    # ---- the torch statement of the sweep
    def _explain_torch(self, x, attrs, target_class, sample_points, metric):
        S = sample_points

        def tile(t):
            return t.repeat(S, *[1] * (t.dim() - 1))

        codes = tile(self.encoder(x, attrs))
        with torch.no_grad():
            original_class = self.classifier(x).argmax(1).cpu().item()
        cf_attrs = {k: tile(v) for k, v in attrs.items() if k != self.target_feature}
        eye = torch.eye(attrs[self.target_feature].shape[1]).to(x.device)
        e_orig = eye[original_class].reshape((1, eye.shape[1])).repeat(S, 1)
        e_target = eye[target_class].reshape((1, eye.shape[1])).repeat(S, 1)
        probs = torch.linspace(0, 1, S).reshape((S, 1)).to(x.device)
        cf_attrs[self.target_feature] = (1 - probs) * e_orig + probs * e_target
        with torch.no_grad():
            samples = self.decoder(codes, cf_attrs)
            preds = self.classifier(samples).argmax(1)
            if metric == 'mixture':
                metric_val = probs
            elif metric == 'mse':
                metric_val = mse(x, samples)
            elif metric == 'ssim':
                metric_val = 1 - ssim((tile(x) + 1) / 2, (samples + 1) / 2, data_range=1.0, size_average=False)
            else:
                raise ValueError(metric)
            hit = preds == target_class
            if not bool(hit.any()):
                return samples, metric_val
            metric_val, samples = metric_val[hit], samples[hit]
            inds = metric_val.argsort()
            return samples[inds], metric_val[inds]

    # ---- the same results from the device executor's order / n_hit
    def _explain_device(self, sweep, x, attrs, target_class, sample_points, metric):
        with torch.no_grad():
            codes = self.encoder(x, attrs)
        r = sweep.run(x, codes, attrs, int(target_class), sample_points, metric)
        n = int(r["n_hit"].item())              # the one host read: the result's length depends on it
        samples, mval = r["samples"], r["metric"]
        if metric == 'mixture':
            if n == 0:
                return samples.clone(), mval.reshape(-1, 1).clone()
            first = r["order"][:1].long()
            return (samples[first].unsqueeze(0).repeat(n, *[1] * samples.dim()),
                    mval[first].reshape(1, 1, 1).repeat(n, 1, 1))
        if n == 0:
            return samples.clone(), mval.clone()
        inds = r["order"][:n].long()
        return samples[inds], mval[inds]


class HingeLossCFExplainer:
    def __init__(self,
                 encoder: torch.nn.Module,
                 decoder: torch.nn.Module,
                 classifier: torch.nn.Module,
                 target_feature: str,
                 latent_dim: int,
                 categorical_features: List[str] = None,
                 features_to_ignore: List[str] = None,
                 c=10.0):
        self.encoder = encoder
        self.decoder = decoder
        self.classifier = classifier
        self.categorical_features = categorical_features or []
        self.features_to_ignore = features_to_ignore or []
        self.c = c
        self.target_feature = target_feature
        self.latent_dim = latent_dim
        self._stepper = None

    def _device_stepper(self, x):
        if not _on_device(x, self.decoder, self.classifier):
            return None
        if self._stepper is None:
            from ali_hip.explain import HingeCFStepper
            self._stepper = _executor(lambda: HingeCFStepper(
                self.decoder, self.classifier, self.target_feature, self.categorical_features,
                self.features_to_ignore, c=self.c)) or False
        return self._stepper or None

    def _draw(self, x, attrs, codes, train_z, rows=1):
        """the initial raw variables, drawn in the reference's order and on the devices it draws them on"""
        init = {k: 0.01 * torch.randn((rows, attrs[k].shape[1]), device=x.device)
                for k in attrs if k not in self.features_to_ignore}
        if train_z:
            init["z"] = torch.randn(codes.shape).to(x.device)
        return init

    def explain(self, x: torch.Tensor,
                attrs: Dict[str, torch.Tensor],
                target_class=None,
                train_z=True,
                steps=30,
                lr=0.1):
        codes = self.encoder(x, attrs).detach()
        stepper = self._device_stepper(x)
        if stepper is None:
            with torch.no_grad():
                original_pred = self.classifier(x).softmax(1)
                original_pred.argmax(1).item()            # (one row only, as in the reference)
            init = self._draw(x, attrs, codes, train_z)
            return self._loop_torch(x, attrs, codes, original_pred, target_class, init, train_z, steps, lr, False)
        if x.shape[0] != 1:
            raise ValueError("HingeLossCFExplainer.explain: one image per call (explain_batch takes a batch)")
        init = self._draw(x, attrs, codes, train_z)
        target = None if target_class is None else torch.tensor([int(target_class)], dtype=torch.int32, device=x.device)
        x_cf, _, _ = stepper.run(x, attrs, codes, target, init, steps, lr, train_z, update_z=False)
        return x_cf

    def explain_batch(self, x, attrs, target_class: Optional[torch.Tensor] = None, train_z=True, steps=30, lr=0.1,
                      init=None, update_z=False):
        """B independent explanations in one run: row b is what ``explain`` computes for ``x[b:b+1]`` from the raw
        variables ``init`` ({key: [B, n_k]} for every attribute that is not ignored, "z": [B, latent, 1, 1] with
        ``train_z``; drawn here when None).  ``target_class``: an int tensor [B] or None.  ``update_z=True`` optimises
        z as well (see the module docstring).  Returns x_cf [B, 1, H, W]."""
        B = x.shape[0]
        codes = self.encoder(x, attrs).detach()
        if init is None:
            init = self._draw(x, attrs, codes, train_z, rows=B)
        stepper = self._device_stepper(x)
        if stepper is not None:
            x_cf, _, _ = stepper.run(x, attrs, codes, target_class, init, steps, lr, train_z, update_z=update_z)
            return x_cf
        out = []
        for b in range(B):
            xb, ab = x[b:b + 1], {k: v[b:b + 1] for k, v in attrs.items()}
            with torch.no_grad():
                original_pred = self.classifier(xb).softmax(1)
            tb = None if target_class is None else int(target_class[b])
            ib = {k: v[b:b + 1].clone() for k, v in init.items()}
            out.append(self._loop_torch(xb, ab, codes[b:b + 1], original_pred, tb, ib, train_z, steps, lr, update_z))
        return torch.cat(out, dim=0)

    # ---- the torch statement of the loop (one row)
    def _loop_torch(self, x, attrs, codes, original_pred, target_class, init, train_z, steps, lr, update_z):
        trained = {k: v for k, v in init.items() if k != "z"}
        for v in trained.values():
            v.requires_grad = True
        variables = dict(trained)
        if train_z:
            variables["z"] = init["z"]
            if update_z:
                variables["z"].requires_grad = True

        def generate():
            a = {}
            for k in attrs:
                if k in self.features_to_ignore:
                    a[k] = attrs[k]
                elif k in self.categorical_features:
                    a[k] = trained[k].softmax(1)
                else:
                    a[k] = trained[k].tanh()
            z = variables["z"].tanh() if train_z else codes
            return self.decoder(z, a)

        def class_term(x_):
            pred = self.classifier(x_)
            if target_class is not None:
                return (max_excluding(pred, target_class) - pred[:, target_class]).mean()
            return (pred - original_pred).square().mean()

        opt = torch.optim.Adam(list(variables.values()), lr=lr)
        for _ in progress(list(range(steps))):
            opt.zero_grad()
            x_cf = generate()
            h = class_term(x_cf)
            m = (x - x_cf).abs().mean()
            loss = self.c * h + m
            loss.backward()
            opt.step()
        return generate()
