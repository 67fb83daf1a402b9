"""Executor of the attribute_shap family (``morphomnist_attribute_shap.py``): expected-gradients attributions (Erion et
al.) of

    f(a) = mean over n_draws z ~ N(0, I) of softmax(clf(decoder(z, a)))

with respect to the attribute row ``a``, hand scheduled on the HIP kernels and replayed from HIP graphs.

The statement.  Explained rows x [R, A], background bg [Nb, A], S = ``nsamples`` samples per row, draws
idx[r,k] in [0, Nb), t[r,k] in [0, 1), z[r,k,s,:] ~ N(0, I):

    a[r,k]     = t[r,k] * x[r] + (1 - t[r,k]) * bg[idx[r,k]]
    delta[r,k] = x[r] - bg[idx[r,k]]
    p[r,k,s,:] = softmax(clf(decoder(z[r,k,s], a[r,k])))
    phi[r,c,:] = 1/S * sum_k delta[r,k] * d/da[r,k] ( 1/n_draws * sum_s p[r,k,s,c] )

``eg_statement`` is that formula in torch (autograd); CPU tensors run it, and the tests compare the device with it.

One ``shap_values`` call on the device, per chunk of ``rows_per_launch`` explained rows: ``ali_eg_input`` (one launch),
then per explained row the generator's and the classifier's forward chains once over its S * n_draws input rows, and
per class ``ali_eg_seed``, both chains' data-gradient passes over the same saved state (``chain_backward`` reads it and
writes none of it; no parameter gradient is computed or touched) and ``ali_eg_reduce``.  The chains always see one
explained row, whatever the chunk: a row's bits do not depend on ``rows_per_launch`` or on R.  No host read inside.

Eval mode only: with BatchNorm in training mode the reference's result depends on shap's internal batches of 50.  The
decoder must be ``image_scms.mnist.Generator`` or derive from it (``deepscm_vae.mnist.VAEDecoder``) and the classifier a
``ClassifierStack``; anything else is a ``TypeError`` at construction.
"""
import torch

from . import ops, rng
from .graphs import GraphCache
from .pipeline import DecodeClassify, LayoutCache, require_eval

MNIST_SLICES = {"digit": (0, 10), "thickness": (10, 1), "intensity": (11, 1), "slant": (12, 1)}
SAVED_BYTES_BUDGET = 8 << 30        # device memory one launch may hold: what the default ``rows_per_launch`` is sized by
MAX_ROWS_PER_LAUNCH = 16            # ... and its cap: bounds the length of a recorded graph (unmeasured)


def attr_dict(rows, slices):
    """{key: columns} of attribute rows [N, A] under ``slices`` {key: (offset, width)}"""
    return {k: rows[:, o:o + w] for k, (o, w) in slices.items()}


def mixed_rows(x, bg, idx, t):
    """(a [R, S, A], delta [R, S, A]) of x [R, A], bg [Nb, A], idx [R, S] (integers), t [R, S], in the dtype of x"""
    b = bg[idx.long()]
    tt = t.to(x.dtype).unsqueeze(-1)
    return tt * x.unsqueeze(1) + (1 - tt) * b, x.unsqueeze(1) - b


def expected_gradients(f, x, bg, idx, t, classes=None):
    """The estimator in torch for any differentiable ``f``: a [R, S, A] -> [R, S, C].  phi [R, C, A]; classes not in
    ``classes`` stay 0."""
    a, delta = mixed_rows(x, bg, idx, t)
    a = a.detach().requires_grad_(True)
    with torch.enable_grad():
        p = f(a)
        phi = torch.zeros(x.shape[0], p.shape[-1], x.shape[1], dtype=x.dtype, device=x.device)
        for c in (range(p.shape[-1]) if classes is None else classes):
            g, = torch.autograd.grad(p[..., c].sum(), a, retain_graph=True)
            phi[:, c] = (delta * g).sum(dim=1) / idx.shape[1]
    return phi


def eg_statement(decoder, classifier, x, bg, idx, t, z, slices, classes=None):
    """The statement in torch: phi [R, C, A] for x [R, A], bg [Nb, A], idx [R, S] (integers), t [R, S], z [R, S, n_draws,
    latent]; in the dtype of ``x`` (the modules must match it)."""
    R, A = x.shape
    S, n_draws = idx.shape[1], z.shape[2]

    def f(a):
        rep = a.unsqueeze(2).expand(R, S, n_draws, A).reshape(-1, A)
        img = decoder(z.to(x.dtype).reshape(R * S * n_draws, -1, 1, 1), attr_dict(rep, slices))
        return classifier(img).softmax(1).reshape(R, S, n_draws, -1).mean(dim=2)
    return expected_gradients(f, x, bg, idx, t, classes)


def input_rows_statement(decoder, x, bg, idx, t, z, slices):
    """What ``ali_eg_input`` writes, in torch: (rows [R*S*n_draws, n_log] = [z | digit @ table | continuous in the
    decoder's order], row ((r*S + k)*n_draws + s), delta [R, S, A])"""
    from image_scms.mnist import _cont_keys
    R, A = x.shape
    S, n_draws = idx.shape[1], z.shape[2]
    a, delta = mixed_rows(x, bg, idx, t)
    rep = attr_dict(a.unsqueeze(2).expand(R, S, n_draws, A).reshape(-1, A), slices)
    parts = [z.to(x.dtype).reshape(R * S * n_draws, -1), rep["digit"].matmul(decoder.digit_embedding.weight.to(x.dtype))]
    return torch.cat(parts + [rep[k] for k in _cont_keys(slices)], dim=1), delta


def value_statement(decoder, classifier, x, z, slices):
    """f(x) [R, C] at z [R, n_draws, latent], in torch"""
    R, A = x.shape
    n_draws = z.shape[1]
    rep = x.unsqueeze(1).expand(R, n_draws, A).reshape(-1, A)
    with torch.no_grad():
        img = decoder(z.to(x.dtype).reshape(R * n_draws, -1, 1, 1), attr_dict(rep, slices))
        return classifier(img).softmax(1).reshape(R, n_draws, -1).mean(dim=1)


class ExpectedGradients:
    """``shap_values(a, draws=None)``: a {key: [R, n]} or a [R, A] tensor (the script's [R, 1, A] as well); ``draws`` an
    optional dict of explicit "idx" [R, S] (integers), "t" [R, S], "z" [R, S, n_draws, latent] -- what is missing is
    drawn from the counter RNG under (``seed``, the number of calls that drew before, the row).  Returns phi [R, C, A]
    fp32 on a's device, without a host read; ``classes`` restricts the backward passes to those classes (the others stay
    0: each class is computed on its own from the one saved forward state).  ``value(a, z=None)`` is f(a) [R, C] at fresh (or the given [R, n_draws,
    latent]) z.  ``background``: {key: [Nb, n]} or [Nb, A]; ``attr_slices`` {key: (offset, width)} names the columns
    of tensor inputs (default: the keys of a background dict in order, else digit | thickness | intensity | slant)."""

    def __init__(self, decoder, classifier, background, n_draws=4, nsamples=200, seed=0, capture=True,
                 rows_per_launch=None, attr_slices=None):
        self.pipe = DecodeClassify(classifier, decoder)
        self.dec = self.pipe.dec
        if self.dec.spect:
            raise TypeError("ExpectedGradients: SpectGenerator decoders are not supported")
        self.decoder, self.classifier = decoder, classifier
        self._check_eval()
        if attr_slices is None:
            if isinstance(background, dict):
                attr_slices, off = {}, 0
                for k, v in background.items():
                    attr_slices[k] = (off, v.shape[1])
                    off += v.shape[1]
            else:
                attr_slices = dict(MNIST_SLICES)
        self.slices = {k: (int(o), int(w)) for k, (o, w) in attr_slices.items()}
        self.cat, self.cont = self.dec.keys(self.slices)
        n_log, want = self.dec.row_width(self.cat, self.cont)[0], self.dec.layers[0].in_channels
        if n_log != want:
            raise ValueError(f"ExpectedGradients: the decoder takes the attributes of a {want}-column input row, "
                             f"{list(self.slices)} make {n_log}")
        for k in self.cont:
            if self.slices[k][1] != 1:
                raise ValueError(f"ExpectedGradients: the continuous attribute {k!r} must be one column")
        self.A = max(o + w for o, w in self.slices.values())
        self.bg = self._rows(background)
        self.n_draws, self.nsamples, self.seed = int(n_draws), int(nsamples), int(seed)
        if self.n_draws < 1 or self.nsamples < 1 or self.bg.shape[0] < 1:
            raise ValueError("ExpectedGradients: n_draws, nsamples and the background must be at least 1")
        self.capture, self.rows_per_launch = capture, rows_per_launch
        self._graphs = GraphCache(modules=[decoder, classifier])
        self._value_graphs = GraphCache(modules=[decoder, classifier])
        self._layouts = LayoutCache(self.dec, self._forget)
        self._calls = 0             # calls that drew: the counter of the RNG key (on the device: ``_ctr``)
        self._ctr = None
        self._shape = None

    # ---- checks and input forms
    def _check_eval(self):
        require_eval("ExpectedGradients", decoder=self.decoder, classifier=self.classifier)

    def _rows(self, a):
        if isinstance(a, dict):
            if set(a) != set(self.slices):
                raise ValueError(f"ExpectedGradients: the decoder takes the attributes {list(self.slices)}, got {list(a)}")
            some = next(iter(a.values()))
            rows = torch.zeros(some.shape[0], self.A, dtype=torch.float32, device=some.device)
            for k, (o, w) in self.slices.items():
                rows[:, o:o + w] = a[k].reshape(-1, w).float()
            return rows
        if a.shape[-1] != self.A:
            raise ValueError(f"ExpectedGradients: attribute rows have {self.A} columns, got {tuple(a.shape)}")
        return a.detach().reshape(-1, self.A).float().contiguous()

    def _draws(self, draws, R, device):
        S, nd, L = self.nsamples, self.n_draws, self.dec.latent()
        draws = dict(draws or {})
        idx, t, z = draws.pop("idx", None), draws.pop("t", None), draws.pop("z", None)
        if draws:
            raise ValueError(f"ExpectedGradients: draws has the unknown entries {list(draws)}")
        if idx is not None:
            idx = idx.to(device=device, dtype=torch.int32).reshape(R, S).contiguous()
        if t is not None:
            t = t.to(device=device, dtype=torch.float32).reshape(R, S).contiguous()
        if z is not None:
            z = z.to(device=device, dtype=torch.float32).reshape(R, S, nd, L).contiguous()
        return idx, t, z

    # ---- the torch statement (CPU tensors), with the draws of the device's streams
    def _host_draws(self, idx, t, z, R):
        S, nd, L = self.nsamples, self.n_draws, self.dec.latent()
        if idx is None:
            idx = torch.from_numpy(rng.eg_index_reference(self.seed, self._calls, R * S, self.bg.shape[0])).reshape(R, S)
        if t is None:
            t = rng.eg_t_reference(self.seed, self._calls, R * S).reshape(R, S)
        if z is None:
            z = rng.normal_reference(self.seed, self._calls, R * S * nd * L).float().reshape(R, S, nd, L)
        return idx, t, z

    # ---- the device path
    def _forget(self):
        """the embedding table moved: the recorded launches name the old layout's"""
        self._graphs.clear()
        self._value_graphs.clear()

    def _device_layout(self, device):
        return self._layouts.get(None, self._build_layout)

    def _build_layout(self):
        L = self.dec.latent()
        segs = []
        for k, (o, w) in self.slices.items():
            if k in self.cat:
                segs.append((ops.CF_COPY, w, o, L + ops.CF_EMB * self.cat.index(k), self.cat.index(k), o))
            else:
                segs.append((ops.CF_COPY, w, o, L + ops.CF_EMB * len(self.cat) + self.cont.index(k), -1, o))
        lay = ops.CfLayout(segs, self.dec.tables(self.cat), *self.dec.row_width(self.cat, self.cont))
        lay.cat = self.cat
        return lay

    def _shapes(self, lay):
        """(classes C, bytes of saved activations per generator-input row): from the two plans, no launch"""
        if self._shape is None:
            self._shape = self.pipe.shapes(lay.n_log, lay.ld)
        return self._shape

    def default_rows_per_launch(self, lay):
        """Explained rows per ``ali_eg_input`` launch (and recorded graph).  The chains run one explained row at a
        time, so one row's saved activations are alive at once; every row of the launch keeps its input rows and
        delta.  As many rows as fit the budget next to that, at most ``MAX_ROWS_PER_LAUNCH``."""
        per = self.nsamples * self.n_draws
        saved = per * self._shapes(lay)[1]
        each = 4 * (per * lay.ld + self.nsamples * self.A)
        return max(1, min(MAX_ROWS_PER_LAUNCH, (SAVED_BYTES_BUDGET - saved) // each))

    def _chunk(self, lay, classes, r0, x, idx, t, z):
        S, nd = self.nsamples, self.n_draws
        R, N = x.shape[0], S * nd
        C = self._shapes(lay)[0]
        rows, delta, _, _ = ops.eg_input(lay, self.dec.latent(), x, self.bg, S, nd, idx, t, z, self.seed, self._ctr, r0)
        phi = torch.zeros(R, C, self.A, dtype=torch.float32, device=x.device)
        # The chains take one explained row (its S * n_draws input rows) per pass: the GEMMs pick their tiles and their
        # split by the batch, so a row's bits would otherwise depend on the rows it shares a launch with
        for r in range(R):
            x_cf, logits, saved = self.pipe.forward(rows[r * N:(r + 1) * N], lay.n_log, True)
            for c in classes:                   # (each from the one saved state; no distance term in the row gradient)
                glogit, _ = ops.eg_seed(logits, c, 1.0 / N)
                ops.eg_reduce(lay, self.pipe.row_grad(saved, glogit, x_cf), delta[r:r + 1], nd, phi[r:r + 1], c)
        return phi

    def _advance(self):
        self._calls += 1
        if self._ctr is not None:
            ops.add_i64_multi([self._ctr], [1])

    @torch.no_grad()
    def shap_values(self, a, draws=None, classes=None):
        self._check_eval()
        x = self._rows(a)
        R = x.shape[0]
        idx, t, z = self._draws(draws, R, x.device)
        drew = idx is None or t is None or z is None
        if not x.is_cuda:
            idx, t, z = self._host_draws(idx, t, z, R)
            phi = eg_statement(self.decoder, self.classifier, x, self.bg.to(x.device), idx, t, z, self.slices, classes)
            self._calls += int(drew)
            return phi
        if self.bg.device != x.device:
            self.bg = self.bg.to(x.device)
        if self._ctr is None:
            self._ctr = torch.full((1,), self._calls, dtype=torch.int64, device=x.device)
        lay = self._device_layout(x.device)
        C = self._shapes(lay)[0]
        classes = tuple(range(C)) if classes is None else tuple(int(c) for c in classes)
        step = int(self.rows_per_launch or self.default_rows_per_launch(lay))
        out = torch.empty(R, C, self.A, dtype=torch.float32, device=x.device)
        for r0 in range(0, R, step):
            r1 = min(R, r0 + step)
            args = tuple(None if v is None else v[r0:r1].contiguous() for v in (x, idx, t, z))
            off = r0 if drew else 0                          # (explicit draws: the offset is not read)
            if self.capture:
                phi = self._graphs(lambda *v: self._chunk(lay, classes, off, *v), args,
                                   (id(lay), classes, off, self.nsamples, self.n_draws, str(x.device)))
            else:
                phi = self._chunk(lay, classes, off, *args)
            out[r0:r1].copy_(phi)
        if drew:
            self._advance()
        return out

    def _value(self, lay, x, z):
        R, nd = x.shape[0], self.n_draws
        rows_idx = torch.arange(R, dtype=torch.int32, device=x.device).reshape(R, 1)
        ones = torch.ones(R, 1, dtype=torch.float32, device=x.device)
        # t = 1 against the rows themselves as background: the attribute part is x, bit for bit
        rows, _, _, _ = ops.eg_input(lay, self.dec.latent(), x, x, 1, nd, rows_idx, ones, z, self.seed, self._ctr, 0)
        _, logits, _ = self.pipe.forward(rows, lay.n_log)
        _, p = ops.eg_seed(logits, 0, 1.0, want_p=True)
        return p.reshape(R, nd, -1).mean(dim=1)

    @torch.no_grad()
    def value(self, a, z=None):
        self._check_eval()
        x = self._rows(a)
        R, nd, L = x.shape[0], self.n_draws, self.dec.latent()
        if z is not None:
            z = z.to(device=x.device, dtype=torch.float32).reshape(R, nd, L).contiguous()
        if not x.is_cuda:
            if z is None:
                z = rng.normal_reference(self.seed, self._calls, R * nd * L).float().reshape(R, nd, L)
                self._calls += 1
            return value_statement(self.decoder, self.classifier, x, z, self.slices)
        if self._ctr is None:
            self._ctr = torch.full((1,), self._calls, dtype=torch.int64, device=x.device)
        lay = self._device_layout(x.device)
        if self.capture:
            out = self._value_graphs(lambda *v: self._value(lay, *v), (x, z), (id(lay), nd, str(x.device))).clone()
        else:
            out = self._value(lay, x, z)
        if z is None:
            self._advance()
        return out
