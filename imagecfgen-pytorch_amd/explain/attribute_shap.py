"""Attribute attributions: the drop-in surface of ``morphomnist_attribute_shap.py`` -- its two model classes
(``VaeShapClf`` / ``BiganShapClf``: one ``AttributeModel``), the explainer it takes from the ``shap`` package
(``GradientExplainer``: expected gradients, Erion et al.) and its loop over the test rows (``explain_all``).

The script's lines and their replacement::

    vae_explainer = shap.GradientExplainer(VaeShapClf(), cat_at(background_a))
    vae_shap_values = np.array(vae_explainer.shap_values(a_expl)).reshape((10, 13))[:, [10, 11, 12]]

    vae_explainer = GradientExplainer(AttributeModel(vae.decoder, clf, n_samples), cat_at(background_a))
    vae_shap_values = np.array(vae_explainer.shap_values(a_expl)).reshape((10, 13))[:, [10, 11, 12]]     # unchanged
    vae_shap = vae_explainer.explain_all(cat_at(a_test_scaled))[:, :, [10, 11, 12]]                      # the whole loop

CUDA tensors run on ``ali_hip.attrib.ExpectedGradients`` (HIP kernels, HIP graphs); CPU tensors run the torch statement
of the same estimator.  The models must be in eval mode (``ali_hip.attrib``).  What is computed is the published
estimator with this package's own draws; agreement with the ``shap`` package's sampling stream, or with any
post-processing it applies, has not been checked (the package is not a dependency).
"""
import numpy as np
import torch

from ali_hip.attrib import MNIST_SLICES, ExpectedGradients, attr_dict


class AttributeModel(torch.nn.Module):
    """``forward(a [N, 1, A])``: the script's ``VaeShapClf.forward`` / ``BiganShapClf.forward`` as executed -- the
    attribute rows repeated ``n_samples`` times sample-major, one z per repeated row, and the softmax rows averaged in
    groups of ``n_samples`` CONSECUTIVE rows (so a group mixes different inputs unless N == 1; the gradient shap takes
    of it is the one of the per-input mean all the same).  ``z`` (optional, [N * n_samples, latent, 1, 1])
    replaces the ``torch.randn`` draw."""

    def __init__(self, decoder, clf, n_samples, attr_slices=None):
        super().__init__()
        self.decoder, self.clf, self.n_samples = decoder, clf, int(n_samples)
        self.slices = dict(attr_slices or MNIST_SLICES)

    def forward(self, a, z=None):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(a)
        n = self.n_samples
        device = next(self.clf.parameters()).device
        a = a.to(device)
        attrs = {k: a[:, :, o:o + w].float().repeat(n, 1, 1).reshape((-1, w)) for k, (o, w) in self.slices.items()}
        if z is None:
            z = torch.randn((a.shape[0] * n, 512, 1, 1)).to(device)
        img = self.decoder(z, attrs)
        pred = self.clf(img).softmax(1)
        return pred.reshape((-1, n, pred.shape[1])).mean(dim=1)


class GradientExplainer:
    """``shap.GradientExplainer(model, data)`` for an ``AttributeModel``: ``shap_values(X, nsamples=200)`` returns a
    list of C numpy arrays [n, 1, A], as the package does for a multi-output model."""

    def __init__(self, model, background, seed=0, capture=True, rows_per_launch=None):
        if not isinstance(model, AttributeModel):
            raise TypeError(f"GradientExplainer: {type(model).__name__} is not an AttributeModel")
        self.model = model
        if isinstance(background, np.ndarray):
            background = torch.from_numpy(background)
        self.background = background
        self._kw = dict(seed=seed, capture=capture, rows_per_launch=rows_per_launch)
        self._executors = {}

    def executor(self, nsamples=200):
        ex = self._executors.get(nsamples)
        if ex is None:
            m = self.model
            ex = self._executors[nsamples] = ExpectedGradients(m.decoder, m.clf, self.background, n_draws=m.n_samples,
                                                               nsamples=nsamples, attr_slices=m.slices, **self._kw)
        return ex

    def _device_rows(self, X):
        if isinstance(X, dict):
            return X
        if isinstance(X, np.ndarray):
            X = torch.from_numpy(X)
        return X.to(next(self.model.clf.parameters()).device)

    def shap_values(self, X, nsamples=200):
        phi = self.executor(nsamples).shap_values(self._device_rows(X)).cpu().numpy()      # [n, C, A]
        return [phi[:, c].reshape(phi.shape[0], 1, phi.shape[2]) for c in range(phi.shape[1])]

    def explain_all(self, a_test, batch=64, nsamples=200):
        """The script's loop over the test rows: ``batch`` rows per ``shap_values`` call on the executor, the results
        kept on the device, one host read at the end.  Returns a numpy array [n, C, A]."""
        ex = self.executor(nsamples)
        a_test = self._device_rows(a_test)
        rows = a_test if not isinstance(a_test, dict) else None
        n = rows.shape[0] if rows is not None else next(iter(a_test.values())).shape[0]
        out = []
        for lo in range(0, n, batch):
            part = rows[lo:lo + batch] if rows is not None else {k: v[lo:lo + batch] for k, v in a_test.items()}
            out.append(ex.shap_values(part))
        return torch.cat(out, dim=0).cpu().numpy()


__all__ = ["AttributeModel", "GradientExplainer", "attr_dict"]
