"""Contrastive and counterfactual baselines: the drop-in surface of what ``morphomnist_cf_metrics.py`` and
``mnist_oracle_scores.py`` take from the omnixai package -- ``Image``, ``ContrastiveExplainer`` (its pertinent negative,
``'pn'``) and ``CounterfactualExplainer`` (``'cf'``) -- and their loop over the test rows (``explain_all``).

The scripts' lines and their replacement::

    from omnixai.explainers.vision import ContrastiveExplainer, CounterfactualExplainer
    from omnixai.data.image import Image

    from explain.contrastive import ContrastiveExplainer, CounterfactualExplainer
    from explain.contrastive import Image

    clf.eval()                                     # added: the device search is defined in eval mode only
    contrastive_explainer = ContrastiveExplainer(clf, preprocess_function=lambda x_: x_.data.reshape((-1, 1, 28, 28)))
    contrastive = contrastive_explainer.explain(Image(x.cpu().numpy().reshape((1, 28, 28, 1)), batched=True)) \\
        .explanations[0]['pn'].reshape((1, 1, 28, 28))                                                 # unchanged
    pn = contrastive_explainer.explain_all(x_test.reshape((-1, 28, 28, 1)))['pn']                      # the whole loop

A CUDA model that is a ``ClassifierStack`` runs ``ali_hip.contrast.ContrastiveSearch`` (HIP kernels, one HIP graph for
every iteration of every round); CPU models and wrappers run the torch statement of the same search.  On the device
path the model must be in eval mode: the scripts load ``clf`` and never call ``clf.eval()``, so that one line is added
next to the two imports (no ``ClassifierStack`` classifier has a layer that depends on the mode: nothing else
changes); a model in training mode is refused where the explainer is built.  The hyper-parameters are keyword
arguments of the constructor under the names ``ali_hip.contrast`` gives them -- omnixai's ``c`` is ``c0`` here -- and
an unknown name is a ``TypeError``; ``explain`` takes the images and nothing else.  What is computed is the published algorithm (Dhurandhar et al. 2018, pertinent
negatives; Wachter et al. 2017, as omnixai's "ce") with omnixai's default hyper-parameters -- pn: c0 = 10, beta = 0.1,
kappa = 10, binary_search_steps = 5, learning_rate = 1e-2, num_iterations = 1000, grad_clip = 1e3; cf: c0 = 10,
kappa = 10, gamma = 1, binary_search_steps = 5, learning_rate = 1e-2, num_iterations = 100, grad_clip = 1e3 -- as
``ali_hip.contrast`` states it.  Agreement with the omnixai package itself has not been checked (the package is not a
dependency).

Pertinent positives (``'pp'``, what ``uncertainty_evolution.py`` reads) come with ``positives=True``: each row also
gets ``cem_pp_statement``'s search (pn's hyper-parameters) around a "no information" pixel value ``background``, in
the units the model takes.  That script feeds ``[0, 1]`` images through a ``ScaledClf`` wrapper (``clf(2 x - 1)``),
which is no ``ClassifierStack`` and runs the statement with ``background=0.0``; on the device the classifier itself
takes ``2 x - 1`` with ``background=-1.0`` and ``(pp + 1) / 2`` maps the images back -- a search in ``[-1, 1]`` units,
whose iterates and distances are not the same numbers as the one in ``[0, 1]`` units.
"""
import numpy as np
import torch

from ali_hip.contrast import (ContrastiveSearch, as_fp32, ce_statement, cem_pn_statement, cem_pp_statement,
                              hyper_parameters)


class Image:
    """``Image(array, batched=True)``: a batch of images [B, H, W, C] (one image [H, W, C] without ``batched``);
    ``.data`` is what a ``preprocess_function`` reads."""

    def __init__(self, data, batched=False):
        if torch.is_tensor(data):
            data = data.detach().cpu().numpy()
        data = np.asarray(data)
        self.data = data if batched else data[None]

    @property
    def shape(self):
        return self.data.shape

    def __len__(self):
        return self.data.shape[0]

    def to_numpy(self):
        return self.data


class Explanations:
    """what ``explain`` returns: ``.explanations[i]`` is the dict of row i"""

    def __init__(self, rows):
        self.explanations = rows

    def get_explanations(self, index=None):
        return self.explanations if index is None else self.explanations[index]


class _SearchExplainer:
    MODE, KEY = None, None

    def __init__(self, model, preprocess_function=None, capture=True, bounds=None, **hyper):
        self.model, self.preprocess, self.capture, self.bounds, self.hyper = model, preprocess_function, capture, bounds, hyper
        params = list(model.parameters()) if isinstance(model, torch.nn.Module) else []
        self.device = params[0].device if params else torch.device("cpu")
        from classifiers._stack import ClassifierStack
        self.on_device = self.device.type == "cuda" and isinstance(model, ClassifierStack)
        if self.on_device and model.training:
            raise ValueError(f"{type(self).__name__}: the model is in training mode; the device search is defined in "
                             f"eval mode only -- call model.eval() before building the explainer")
        self._executors = {}
        self._shapes = {}
        hyper_parameters(self.MODE, hyper)           # (an unknown name is refused here, on either route)

    def _searches(self):
        """(mode, image key, found key, keyword arguments) of every search a row gets"""
        return [(self.MODE, self.KEY, "found", dict(bounds=self.bounds))]

    # ---- the model's input shape, learnt from the preprocess function on one probe
    def _input_shape(self, shape):
        """the per-row shape the model takes for image batches [B, *shape]"""
        shape = tuple(shape)
        got = self._shapes.get(shape)
        if got is None:
            if self.preprocess is None:
                got = shape
            else:
                n = int(np.prod(shape))
                probe = np.arange(2 * n, dtype=np.float32).reshape((2,) + shape)
                out = self.preprocess(Image(probe, batched=True))
                out = out.detach().cpu().numpy() if torch.is_tensor(out) else np.asarray(out)
                if out.size != probe.size or out.shape[0] != 2 or not np.array_equal(out.reshape(-1), probe.reshape(-1)):
                    raise ValueError(f"{type(self).__name__}: the preprocess_function must keep the images' element "
                                     f"count and order (a reshape); it turned {probe.shape} into {out.shape}")
                got = tuple(out.shape[1:])
            self._shapes[shape] = got
        return got

    def _search(self, x, mode, kw):
        """x [B, *model input shape] on the model's device -> the result dict of search ``mode`` there"""
        if self.on_device and x.dim() == 4 and x.shape[1] == 1:
            ex = self._executors.get(mode)
            if ex is None:
                ex = self._executors[mode] = ContrastiveSearch(self.model, mode, capture=self.capture, **kw,
                                                               **self.hyper)
            return ex.run(x)
        statement = {"pn": cem_pn_statement, "ce": ce_statement, "pp": cem_pp_statement}[mode]
        return statement(self.model, x, **kw, **self.hyper)

    def _tensor(self, X):
        data = X.data if isinstance(X, Image) else X
        if not torch.is_tensor(data):
            data = torch.from_numpy(np.ascontiguousarray(data))
        return data

    def _run(self, data):
        """data [B, ...] tensor in the caller's layout -> [(key, found key, images [B, n] in that layout's order, label,
        found)] for every search"""
        B = data.shape[0]
        x = data.to(self.device).float().reshape((B,) + self._input_shape(data.shape[1:]))
        out = []
        for mode, key, fkey, kw in self._searches():
            res = self._search(x, mode, kw)
            out.append((key, fkey, res["image"].reshape(B, -1), res["label"], res["found"]))
        return out

    def explain(self, X):
        data = self._tensor(X)
        rows = [{} for _ in range(data.shape[0])]
        for key, fkey, img, label, found in self._run(data):
            img = img.reshape(data.shape).cpu().numpy()
            label, found = label.cpu().numpy(), found.cpu().numpy()
            for i, row in enumerate(rows):
                row.update({key: img[i], key + "_label": int(label[i]), fkey: int(found[i])})
        return Explanations(rows)

    def explain_all(self, images, batch=64):
        """The scripts' loop over the test rows: ``batch`` rows per search, the results kept on the model's device, one
        host read at the end.  Returns {key: images in the input's layout, key_label: int64 [n], "found": int64 [n]}
        (and, with positives, "pp", "pp_label", "pp_found") as numpy arrays, rows in the input's order."""
        data = self._tensor(images)
        n = data.shape[0]
        parts, names = [], []
        for lo in range(0, n, batch):
            res = self._run(data[lo:lo + batch])
            names = [(key, fkey) for key, fkey, _, _, _ in res]
            parts.append(torch.cat([torch.cat([img, label.to(img.dtype).unsqueeze(1), found.to(img.dtype).unsqueeze(1)],
                                              dim=1) for _, _, img, label, found in res], dim=1))
        every = torch.cat(parts, dim=0).cpu().numpy()                # (labels and flags are small integers: exact)
        width = every.shape[1] // len(names)
        out = {}
        for j, (key, fkey) in enumerate(names):
            blk = every[:, j * width:(j + 1) * width]
            out.update({key: blk[:, :-2].reshape(tuple(data.shape)), key + "_label": blk[:, -2].astype(np.int64),
                        fkey: blk[:, -1].astype(np.int64)})
        return out


class ContrastiveExplainer(_SearchExplainer):
    """``ContrastiveExplainer(model, preprocess_function=None, positives=False, background=0.0, **hyper)``:
    ``explain(Image(...))`` returns an object whose ``.explanations[i]`` is {"pn": image in the input's layout,
    "pn_label": int, "found": 0 / 1}; a row without a pertinent negative gets its own image and label back (``found`` =
    0).  With ``positives`` each row also gets the pertinent positive around the "no information" value ``background``
    (in the model's input units): "pp", "pp_label", "pp_found" (a row without one: its own image, its label, 0).  The
    hyper-parameters serve both searches; ``bounds`` is the pertinent negative's alone."""
    MODE, KEY = "pn", "pn"

    def __init__(self, model, preprocess_function=None, capture=True, bounds=None, positives=False, background=0.0,
                 **hyper):
        super().__init__(model, preprocess_function=preprocess_function, capture=capture, bounds=bounds, **hyper)
        self.positives, self.background = bool(positives), as_fp32(background)

    def _searches(self):
        pp = [("pp", "pp", "pp_found", dict(background=self.background))] if self.positives else []
        return super()._searches() + pp


class CounterfactualExplainer(_SearchExplainer):
    """``CounterfactualExplainer(model, preprocess_function=None, **hyper)``: as ``ContrastiveExplainer`` with the keys
    "cf", "cf_label" and "found"."""
    MODE, KEY = "ce", "cf"


__all__ = ["Image", "ContrastiveExplainer", "CounterfactualExplainer"]
