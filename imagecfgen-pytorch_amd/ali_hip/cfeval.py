"""Executors of the counterfactual-identity family: the evaluation loops that ask whether a counterfactual keeps the
identity of the recording it came from (``audiomnist_cf_eval.py``, ``audiomnist_cf_classifier_metric.py``) and the
counterfactual-score loops ``whale_cf_score.py``, ``mnist_bigan_score.py`` and ``audiomnist_bigan_score.py``.

  ManifoldBank        the real recordings, grouped by (owner, class) -- (subject, digit) in the AudioMNIST scripts.
                      ``errors(cf, owner, cls)`` is audiomnist_cf_eval.py:93-131 per row: the mean squared distance to
                      the cell's recordings (same), to the recordings of every other owner of that class (other), and
                      their ratio.  On the device the bank is two fp64 moment arrays built once (csrc/cfeval.hip:
                      ``ali_group_moments``) and a row costs one pass over its own columns (``ali_manifold_err``).
  CounterfactualEval  the scripts' loop body for one batch and several models: codes, counterfactual, intervention,
                      the bank's errors and every classifier's hit for both images -- one HIP graph per input signature,
                      columns kept on the device until ``table()``, hits in device counters until ``accuracy()``.

CPU tensors run the torch statement of the same loops in the dtype of the tensors (fp64 capable): the tests' reference.
"""
import numpy as np
import torch

from . import ops
from .graphs import GraphCache

_MAX_ROWS = 65535                # rows of one ali_manifold_err launch


def _index(t: torch.Tensor) -> torch.Tensor:
    """labels as an int64 vector: one-hot (or soft) rows [B, n > 1] by their first maximum, int tensors as they are"""
    if t.dim() >= 2 and t.shape[-1] > 1:
        return t.reshape(-1, t.shape[-1]).argmax(1)
    return t.reshape(-1).long()


class ManifoldBank:
    """The real rows a counterfactual is measured against, grouped into ``n_owners * n_classes`` cells.

    ``rows`` [N, ...] are flattened to [N, D]; ``owner`` and ``cls`` are int tensors [N] or one-hot rows.  Bank rows
    whose owner or class is negative or out of range are left out.

    CUDA ``rows``: the cells' CSR is built with torch ops on the device (``n_owners`` and ``n_classes`` are given, so
    nothing is read back), ``ali_group_moments`` runs once and ``rows`` is not kept.  What stays is the column sums and
    column sums of squares of every cell and class in float64: 16 bytes * (O * C + C) * D -- 157 MB for the 600 cells
    of AudioMNIST's 60 subjects, 10 digits and 16384 columns (plus 2.6 MB of class totals).

    CPU ``rows``: the rows are kept, and ``errors`` evaluates the pairwise statement of the script literally."""

    def __init__(self, rows, owner, cls, n_owners, n_classes):
        self.O, self.C = int(n_owners), int(n_classes)
        if self.O < 1 or self.C < 1:
            raise ValueError("ManifoldBank: n_owners and n_classes must be >= 1")
        N = rows.shape[0]
        rows = rows.reshape(N, -1)
        self.D = rows.shape[1]
        owner, cls = _index(owner).to(rows.device), _index(cls).to(rows.device)
        if N < 1 or self.D < 1 or owner.numel() != N or cls.numel() != N:
            raise ValueError(f"ManifoldBank: need N >= 1 rows of D >= 1 columns and one owner and class per row, got "
                             f"{tuple(rows.shape)}, {owner.numel()} owners, {cls.numel()} classes")
        valid = (owner >= 0) & (owner < self.O) & (cls >= 0) & (cls < self.C)
        self.on_device = rows.is_cuda
        if not self.on_device:
            self.rows, self.owner, self.cls = rows[valid], owner[valid], cls[valid]
            return
        cells = self.O * self.C
        cell = torch.where(valid, owner * self.C + cls, torch.full_like(owner, cells))     # left-out rows sort last
        order = torch.argsort(cell, stable=True).to(torch.int32)
        counts = torch.bincount(cell, minlength=cells + 1)[:cells]
        start = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
        self.cnt = counts.to(torch.int32)
        self.tcnt = counts.reshape(self.O, self.C).sum(0).to(torch.int32)
        if rows.dtype != torch.float32 or rows.stride(1) != 1:
            rows = rows.float().contiguous()
        self.S, self.Q, self.TS, self.TQ = ops.group_moments(rows, order, start, self.O, self.C)

    def errors(self, cf, owner, cls):
        """{"same", "other", "ratio"} as [M] tensors on ``cf``'s device for cf [M, ...] and one (owner, class) per row;
        no host read on the device.  An empty cell gives same = NaN, an empty rest of the class other = NaN (the
        script's 0 / 0); an owner outside [0, O) is a subject the bank has never seen: same = NaN and other over the
        whole class; a class outside [0, C) gives three NaNs."""
        M = cf.shape[0]
        cf = cf.reshape(M, -1)
        if cf.shape[1] != self.D:
            raise ValueError(f"ManifoldBank.errors: rows of {cf.shape[1]} columns against a bank of {self.D}")
        if cf.is_cuda != self.on_device:
            raise ValueError("ManifoldBank.errors: the rows and the bank live on different devices")
        owner, cls = _index(owner), _index(cls)
        if owner.numel() != M or cls.numel() != M:
            raise ValueError("ManifoldBank.errors: one owner and one class per row")
        if not self.on_device:
            return self._errors_torch(cf, owner, cls)
        if cf.dtype != torch.float32 or (cf.shape[1] > 1 and cf.stride(1) != 1):
            cf = cf.float().contiguous()
        owner, cls = owner.to(torch.int32), cls.to(torch.int32)
        out = torch.empty(M, 3, dtype=torch.float32, device=cf.device)
        for lo in range(0, M, _MAX_ROWS):
            hi = min(lo + _MAX_ROWS, M)
            ops.manifold_err(cf[lo:hi], owner[lo:hi].contiguous(), cls[lo:hi].contiguous(), self.S, self.Q, self.TS,
                             self.TQ, self.cnt, self.tcnt, out=out[lo:hi])
        return {"same": out[:, 0], "other": out[:, 1], "ratio": out[:, 2]}

    def _errors_torch(self, cf, owner, cls):
        """audiomnist_cf_eval.py:93-131 for every (owner, class) pair among the rows, in the rows' dtype"""
        M = cf.shape[0]
        same, other = cf.new_empty(M), cf.new_empty(M)
        bank = self.rows.to(cf.dtype)
        pairs = torch.stack([owner, cls], dim=1)
        for o, c in torch.unique(pairs, dim=0).tolist():
            at = (owner == o) & (cls == c)
            a = cf[at]
            same_x = bank[(self.owner == o) & (self.cls == c)]
            other_x = bank[(self.owner != o) & (self.cls == c)]
            same[at] = (a.unsqueeze(1) - same_x).square().sum(dim=(1, 2)) / len(same_x)
            other[at] = (a.unsqueeze(1) - other_x).square().sum(dim=(1, 2)) / len(other_x)
        return {"same": same, "other": other, "ratio": same / other}


def _is_vae(m):
    return hasattr(m, "encoder") and hasattr(m, "decoder")


class CounterfactualEval:
    """The body of the counterfactual evaluation loops for one batch and every model:

        codes = E(x, attrs);  cf = G(codes, cf_attrs);  int = G(z, cf_attrs)
        same, other, ratio = bank.errors(img, owner, cls)          hit = clf(img).argmax(1) == label

    for img in (cf, int).  ``models`` maps a column name to ``(E, G)`` or to a VAE (codes = ``vae.encoder(x, a)[0]``,
    decoder = ``vae.decoder``, as the scripts use them); ``classifiers`` maps a name to a classifier; ``bank`` is a
    ``ManifoldBank``.  Each statement is ONE module call at B rows -- nothing is batched across models or across cf /
    int -- so the images and hits are those of the module calls the scripts make, bit for bit.  On the device all of it
    is one HIP graph per input signature (``capture``), dropped when a weight changes; ``add`` makes no host read.

    ``add`` returns the batch's columns as device tensors of the caller's own -- ``{model}_{cf|int}_{same|other|
    ratio}``, ``{model}_{cf|int}_hit_{clf}`` and the images ``{model}_{cf|int}_image`` --, appends the columns to
    device buffers and adds the hits into int64 device counters.  ``table()`` is the one host read of the columns,
    ``accuracy()`` of the counters; ``reset()`` clears both.  CPU tensors and modules run the torch statement."""

    def __init__(self, models, bank=None, classifiers=None, capture=True, latent_dim=512):
        self.models = {}
        mods = []
        for name, m in models.items():
            if _is_vae(m):
                self.models[name] = (m.encoder, m.decoder, True)
                mods.append(m)
            else:
                E, G = m
                self.models[name] = (E, G, False)
                mods += [E, G]
        self.bank = bank
        self.classifiers = dict(classifiers or {})
        mods += list(self.classifiers.values())
        self.capture = capture
        self.latent_dim = latent_dim
        self._modules = mods
        self._graphs = GraphCache(modules=mods)
        self._hit_cols = [f"{name}_{kind}_hit_{c}" for name in self.models for kind in ("cf", "int")
                          for c in self.classifiers]
        self._blocks = []                  # (column names, [B, columns] block) in the order they were added
        self.counters = None               # int64 hits per hit column, on the device of the batches
        self.seen = [0] * len(self._hit_cols)

    # ------------------------------------------------------------------ names
    def _columns(self, with_int):
        cols = []
        for name in self.models:
            for kind in ("cf", "int") if with_int else ("cf",):
                if self.bank is not None:
                    cols += [f"{name}_{kind}_{k}" for k in ("same", "other", "ratio")]
                cols += [f"{name}_{kind}_hit_{c}" for c in self.classifiers]
        return cols

    def _ensure_counters(self, device):
        if self.counters is None or self.counters.device != device:
            self.counters = torch.zeros(max(len(self._hit_cols), 1), dtype=torch.int64, device=device)

    # ------------------------------------------------------------------ one batch
    def _run(self, x, attrs, cf_attrs, owner, cls, labels, z):
        out, cols, hits = {}, [], {}
        want = {c: _index(labels[c] if labels is not None and c in labels else cf_attrs[c]) for c in self.classifiers}
        for i, (name, (E, G, vae)) in enumerate(self.models.items()):
            codes = E(x, attrs)[0] if vae else E(x, attrs)
            imgs = [("cf", G(codes, cf_attrs))]
            if z is not None:
                imgs.append(("int", G(z[i], cf_attrs)))
            for kind, img in imgs:
                out[f"{name}_{kind}_image"] = img
                if self.bank is not None:
                    e = self.bank.errors(img, owner, cls)
                    for k in ("same", "other", "ratio"):
                        out[f"{name}_{kind}_{k}"] = e[k]
                        cols.append(e[k].reshape(-1, 1).to(img.dtype))
                for c, clf in self.classifiers.items():
                    hit = clf(img).argmax(1) == want[c]
                    out[f"{name}_{kind}_hit_{c}"] = hits[f"{name}_{kind}_hit_{c}"] = hit
                    cols.append(hit.reshape(-1, 1).to(img.dtype))
        if hits:            # one sum for every counter; a column this batch does not have (z=False) adds zeros
            none = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
            self.counters.add_(torch.stack([hits.get(c, none) for c in self._hit_cols], dim=1).sum(0))
        if cols:
            out["row"] = torch.cat(cols, dim=1)              # [B, columns]: what ``table`` reads (0 / 1 are exact)
        return out

    @torch.no_grad()
    def add(self, x, attrs, cf_attrs, owner=None, cls=None, labels=None, z=None):
        """x [B, ...] images, attrs / cf_attrs the attribute dicts of the observation and of the counterfactual; owner,
        cls: the bank cell every row is measured against (needed with a bank) -- [B] int tensors, one-hot rows, or one
        int for the whole batch; labels {classifier: int tensor or one-hot rows} (default: ``cf_attrs[classifier]``);
        z [n_models, B, latent, 1, 1]: the intervention's latents in the models' order, drawn with ``torch.randn``
        outside the graph when None; ``z=False`` skips the intervention columns."""
        B, dev = x.shape[0], x.device
        attrs = {k: v for k, v in attrs.items() if torch.is_tensor(v)}
        cf_attrs = {k: v for k, v in cf_attrs.items() if torch.is_tensor(v)}
        if self.bank is None:
            owner = cls = None
        elif owner is None or cls is None:
            raise ValueError("CounterfactualEval.add: a bank needs owner and cls of every row")
        else:
            owner, cls = (t if torch.is_tensor(t) else torch.full((B,), int(t), dtype=torch.int32, device=dev)
                          for t in (owner, cls))
        if z is False:
            z = None
        elif z is None:
            z = torch.randn(len(self.models), B, self.latent_dim, 1, 1, device=dev, dtype=x.dtype)
        elif z.shape[0] != len(self.models):
            raise ValueError(f"CounterfactualEval.add: z holds {z.shape[0]} draws for {len(self.models)} models")
        self._ensure_counters(dev)
        args = (x, attrs, cf_attrs, owner, cls, labels, z)
        if self.capture and x.is_cuda:
            out = self._graphs(self._run, args, tuple(m.training for m in self._modules), [self.counters])
        else:
            out = self._run(*args)
        # (a replay writes the tensors the recording returned: the caller gets copies of its own)
        out = {k: v.clone() for k, v in out.items()}
        for i, col in enumerate(self._hit_cols):
            if col in out:
                self.seen[i] += B
        row = out.pop("row", None)
        if row is not None:
            self._blocks.append((tuple(self._columns(z is not None)), row))
        return out

    # ------------------------------------------------------------------ results
    def table(self):
        """{column: numpy array} of every row added so far, in the order the rows were added; hit columns are int64.
        One host read per set of columns (one, unless some calls passed ``z=False`` and others did not: a column then
        holds the rows of the calls that produced it)."""
        groups = {}
        for names, row in self._blocks:
            groups.setdefault(names, []).append(row)
        host = {names: torch.cat(rows).cpu().numpy() for names, rows in groups.items()}
        at = dict.fromkeys(host, 0)
        parts = {c: [] for c in self._columns(True)}
        for names, row in self._blocks:
            lo = at[names]
            at[names] = lo + row.shape[0]
            for j, c in enumerate(names):
                parts[c].append(host[names][lo:lo + row.shape[0], j])
        out = {}
        for c, p in parts.items():
            v = np.concatenate(p) if p else np.zeros(0, dtype=np.float32)
            out[c] = v.astype(np.int64) if c in self._hit_cols else v
        return out

    def accuracy(self):
        """{hit column: hits / rows that column has seen} (one host read)"""
        if not self._hit_cols:
            return {}
        hits = self.counters.tolist() if self.counters is not None else [0] * len(self._hit_cols)
        return {c: h / max(n, 1) for c, h, n in zip(self._hit_cols, hits, self.seen)}

    def reset(self):
        self._blocks = []
        self.seen = [0] * len(self._hit_cols)
        if self.counters is not None:
            self.counters.zero_()
