"""Executors of the explain family (``explain/cf_example.py``): the two counterfactual explainers' loops, hand
scheduled on the HIP kernels and replayed from HIP graphs.

  HingeCFStepper   the optimisation loop of ``HingeLossCFExplainer.explain``: per step one launch that turns the raw
                   variables into the generator's input rows, the generator's and the classifier's forward chains, the
                   L1 distance, the hinge loss, both chains' data-gradient passes (no parameter gradient is computed or
                   touched) and one launch for the variables' gradient and Adam update.  Any batch size: B rows are B
                   independent explanations.  No host read inside.
  MixtureSweep     ``DeepCounterfactualExplainer.explain``: the mixture rows, the generator and the classifier on all
                   ``sample_points`` rows, the metric, and arg-max / filter / sort as ``ali_cf_select`` -- one graph.

The decoder must be one of this package's generator stacks (``image_scms.mnist.Generator``,
``image_scms._spect.SpectGenerator`` and what derives from them) and the classifier a ``ClassifierStack``: the
executors read their tables and layer stacks instead of calling them.  Anything else is a ``TypeError`` at
construction (``explain/cf_example.py`` then runs the torch statement of the loop).
"""
import torch

from . import ops, ssim as _ssim
from .graphs import GraphCache
from .pipeline import DecodeClassify, LayoutCache


class HingeCFStepper:
    """The loop of ``HingeLossCFExplainer.explain`` on the device (see the module docstring).

    ``run(x, attrs, codes, target, init, steps, lr, train_z)``: x [B,1,H,W] (or one image for all rows), attrs {key:
    [B, n]}, codes the encoder's [B, latent, 1, 1], target an int32 / int64 [B] device tensor or None (None: every row
    keeps its class, the loss compares the logits with the classifier's softmax of x, as the reference does), init
    {key: raw variable [B, n] for every attribute that is not ignored, "z": codes-shaped when ``train_z``}.  Returns
    (x_cf [B,1,H,W], {key: transformed attribute}, last [B, 3] = (loss, h, m) per row), all on the device.

    ``update_z=False`` (the default here and in the drop-in class: one default for one flag) keeps ``tanh(init["z"])``
    fixed instead of optimising z: the reference creates its z after it has marked the variables as trainable, so its
    Adam never moves z.  ``update_z=True`` optimises z as well."""

    def __init__(self, decoder, classifier, target_feature, categorical_features=None, features_to_ignore=None, c=10.0,
                 capture=True, betas=(0.9, 0.999), eps=1e-8):
        self.pipe = DecodeClassify(classifier, decoder)
        self.dec = self.pipe.dec
        self.decoder, self.classifier = decoder, classifier
        self.target_feature = target_feature
        self.categorical = list(categorical_features or [])
        self.ignored = list(features_to_ignore or [])
        self.c, self.capture, self.betas, self.eps = float(c), capture, betas, eps
        self._graphs = GraphCache(modules=[decoder, classifier])           # the step: one graph per input signature
        self._final_graphs = GraphCache(modules=[decoder, classifier])     # the closing forward
        self._state = {}
        self._layouts = LayoutCache(self.dec, self._forget)

    def _forget(self):
        """the embedding tables moved: nothing recorded or keyed under a layout's id is valid any more"""
        self._graphs.clear()
        self._final_graphs.clear()
        self._state.clear()

    # ---- the segment table of one attribute signature
    def layout(self, attrs, trained_z):
        key = (tuple((k, v.shape[1]) for k, v in attrs.items()), trained_z)
        return self._layouts.get(key, lambda: self._build_layout(attrs, trained_z))

    def _build_layout(self, attrs, trained_z):
        dec = self.dec
        cat, cont = dec.keys(attrs)
        L = dec.latent()
        segs, raw_off, given_off, attr_off = [], 0, 0, 0
        where = {"raw": {}, "given": {}, "attr": {}}
        for k, v in attrs.items():
            w = v.shape[1]
            if k in cat:
                table, dst = cat.index(k), L + ops.CF_EMB * cat.index(k)
            else:
                if w != 1:
                    raise ValueError(f"explain: the continuous attribute {k!r} must be [B, 1], got {tuple(v.shape)}")
                table, dst = -1, L + ops.CF_EMB * len(cat) + cont.index(k)
            if k in self.ignored:
                segs.append((ops.CF_COPY, w, given_off, dst, table, attr_off))
                where["given"][k] = (given_off, w)
                given_off += w
            else:
                kind = ops.CF_SOFTMAX if k in self.categorical else ops.CF_TANH
                segs.append((kind, w, raw_off, dst, table, attr_off))
                where["raw"][k] = (raw_off, w)
                raw_off += w
            where["attr"][k] = (attr_off, w)
            attr_off += w
        if trained_z:
            segs.append((ops.CF_TANH, L, raw_off, 0, -1, -1))
            where["raw"]["z"] = (raw_off, L)
        else:
            segs.append((ops.CF_COPY, L, given_off, 0, -1, -1))
            where["given"]["z"] = (given_off, L)
        lay = ops.CfLayout(segs, dec.tables(cat), *dec.row_width(cat, cont))
        lay.cat, lay.where = cat, where
        if lay.raw_ld == 0:
            raise ValueError("explain: nothing to optimise (every attribute is ignored and z is not trained)")
        return lay

    def _buffers(self, lay, B, device):
        key = (id(lay), B, device)
        st = self._state.get(key)
        if st is None:
            f = dict(dtype=torch.float32, device=device)
            st = self._state[key] = dict(
                raw=torch.zeros(B, lay.raw_ld, **f), m=torch.zeros(B, lay.raw_ld, **f), v=torch.zeros(B, lay.raw_ld, **f),
                step=torch.zeros(B, dtype=torch.int32, device=device), graw=torch.zeros(B, lay.raw_ld, **f))
        return st

    # ---- one step and the closing forward: what the graphs record
    def _step(self, lay, st, lr, x, given, target, orig_pred):
        rows, attrs = ops.cf_input_fwd(lay, st["raw"], given)
        x_cf, logits, saved = self.pipe.forward(rows, lay.n_log, True)
        m = ops.row_dist(x, x_cf.reshape(rows.shape[0], -1), ops.DIST_L1)
        out3, glogit = ops.cf_hinge(logits, target, m, self.c, orig_pred=orig_pred)
        g_rows = self.pipe.row_grad(saved, glogit, x_cf, x)
        ops.cf_input_step(lay, g_rows, rows, attrs, st["raw"], st["m"], st["v"], st["step"], lr, self.betas, self.eps,
                          graw=st["graw"])
        st["probe"] = {"logits": logits, "glogit": glogit, "x_cf": x_cf, "m": m}                  # (tests, inspection)
        return out3

    def _final(self, lay, st, given):
        rows, attrs = ops.cf_input_fwd(lay, st["raw"], given)
        return self.pipe.generate(rows, lay.n_log)[0], attrs

    @torch.no_grad()
    def run(self, x, attrs, codes, target=None, init=None, steps=30, lr=0.1, train_z=True, update_z=False):
        if not x.is_cuda:
            raise ValueError("HingeCFStepper.run: needs CUDA tensors")
        B = codes.shape[0]
        dev = x.device
        trained_z = bool(train_z and update_z)
        lay = self.layout(attrs, trained_z)
        st = self._buffers(lay, B, dev)
        init = init or {}
        for k, (off, w) in lay.where["raw"].items():
            if k not in init:
                raise ValueError(f"HingeCFStepper.run: init has no entry for {k!r}")
            st["raw"][:, off:off + w] = init[k].reshape(-1, w).float().expand(B, w)
        zrow = codes.reshape(B, -1).float()
        if train_z and not update_z:
            zrow = torch.tanh(init["z"].reshape(B, -1).float())
        parts = [(zrow if k == "z" else attrs[k].reshape(B, -1).float()) for k in lay.where["given"]]
        given = torch.cat(parts, dim=1).contiguous() if parts else None
        for k in ("m", "v", "step", "graw"):
            st[k].zero_()
        xf = x.reshape(x.shape[0], -1).float().contiguous()
        if xf.shape[0] not in (1, B):
            raise ValueError(f"HingeCFStepper.run: x has {xf.shape[0]} rows, the batch {B}")
        orig_pred = None
        if target is None:
            target = torch.full((B,), -1, dtype=torch.int32, device=dev)
            ximg = x.float().expand((B,) + tuple(x.shape[1:])) if x.shape[0] != B else x.float()
            orig_pred = torch.softmax(self.classifier(ximg), dim=1).contiguous()
        target = target.to(device=dev, dtype=torch.int32).reshape(B).contiguous()

        out3 = None
        state = [st["raw"], st["m"], st["v"], st["step"], st["graw"]]
        if not self.capture:
            for _ in range(steps):
                out3 = self._step(lay, st, lr, xf, given, target, orig_pred)
            x_cf, attrs_cf = self._final(lay, st, given)
        else:
            modes = (self.decoder.training, self.classifier.training)
            # the recorded calls close over this batch's buffers: B and the device belong to the key (``given`` may be
            # None, and then no argument carries them)
            where = (id(lay), B, str(dev), modes)
            args, extra = (xf, given, target, orig_pred), where + (float(lr),)
            if steps > 0:
                out3 = self._graphs(lambda *a: self._step(lay, st, lr, *a), args, extra, state)
                self._graphs.replay(args, extra, steps - 1)               # the inputs are in place: replay only
            x_cf, attrs_cf = self._final_graphs(lambda g_: self._final(lay, st, g_), (given,), where)
        if out3 is None:
            out3 = torch.full((B, 3), float("nan"), device=dev)
        named = {k: attrs_cf[:, off:off + w].clone() for k, (off, w) in lay.where["attr"].items()}
        return x_cf.clone(), named, out3.clone()

    def variables(self, attrs, train_z=True, update_z=False, B=None, device=None):
        """{name: view} of the raw variables, their gradient of the last step, both Adam moments, the step counters and
        the last step's logits / logit gradient / image / distance ("probe") of the batch that ran last under this
        signature (tests, inspection)."""
        lay = self.layout(attrs, bool(train_z and update_z))
        some = next(iter(attrs.values()))
        st = self._buffers(lay, B or some.shape[0], device or some.device)
        out = {"step": st["step"], "probe": st.get("probe")}
        for k, (off, w) in lay.where["raw"].items():
            out[k] = {n: st[n][:, off:off + w] for n in ("raw", "graw", "m", "v")}
        return out


class MixtureSweep:
    """``DeepCounterfactualExplainer.explain`` on the device (see the module docstring).

    ``run(x, codes, attrs, target, sample_points, metric, orig=None)``: x [1,1,H,W], codes [1, latent, 1, 1], attrs
    {key: [1, n]}, target an int or a one-element int32 device tensor, orig the class the classifier gives x (a
    one-element int32 device tensor, as ``ops.softmax_xent(want_pred=True)`` returns it; None: computed here, inside the
    graph).  Returns {"samples" [S,1,H,W], "metric" [S], "pred" [S] int32, "order" [S] int32, "n_hit" [1] int32,
    "logits" [S, C]} on the device: tensors of the graph, overwritten by the next call of the same signature."""

    METRICS = ("mixture", "mse", "ssim")

    def __init__(self, decoder, classifier, target_feature, capture=True):
        self.pipe = DecodeClassify(classifier, decoder)
        self.dec = self.pipe.dec
        self.decoder, self.classifier = decoder, classifier
        self.target_feature = target_feature
        self.capture = capture
        self._graphs = GraphCache(modules=[decoder, classifier])
        self._const = {}

    def _constants(self, S, n, device):
        key = (S, n, device)
        c = self._const.get(key)
        if c is None:
            p = torch.linspace(0, 1, S).reshape(S, 1).to(device)
            c = self._const[key] = (p, torch.eye(n).to(device))
        return c

    def _sweep(self, S, metric, x, codes, attrs, target, orig):
        dec = self.dec
        cat, cont = dec.keys(attrs)
        n_log, ld = dec.row_width(cat, cont)
        if orig is None:
            lx, _ = self.pipe.classify(x)
            _, _, orig = ops.softmax_xent(lx, lx, want_grad=False, want_pred=True)
        p, eye = self._constants(S, attrs[self.target_feature].shape[1], x.device)
        e_orig = eye.index_select(0, orig.long())
        e_target = eye.index_select(0, target.long())
        mix = (1 - p) * e_orig + p * e_target
        rep = {k: (mix if k == self.target_feature else v.float().expand(S, v.shape[1]).contiguous())
               for k, v in attrs.items()}
        z = codes.reshape(1, -1).float().expand(S, -1).contiguous()
        cvals = torch.cat([rep[k] for k in cont], dim=1).contiguous() if cont else None
        rows = ops.g_input(z, [rep[k].contiguous() for k in cat], dec.tables(cat), cvals, ld)
        samples, logits, _ = self.pipe.forward(rows, n_log)
        if metric == "mixture":
            mval = p.reshape(S).clone()
        elif metric == "mse":
            mval = ops.row_dist(x.reshape(1, -1).float().contiguous(), samples.reshape(S, -1), ops.DIST_L2)
        else:
            xv = x.float().expand(samples.shape).contiguous()
            mval = (1 - _ssim.ssim((xv + 1) / 2, (samples + 1) / 2, data_range=1.0, size_average=False)).contiguous()
        pred, order, n_hit = ops.cf_select(logits, mval, target)
        return {"samples": samples, "metric": mval, "pred": pred, "order": order, "n_hit": n_hit, "logits": logits,
                "orig": orig}

    @torch.no_grad()
    def run(self, x, codes, attrs, target, sample_points=100, metric="mixture", orig=None):
        S = int(sample_points)
        if S > 1024:
            raise ValueError(f"MixtureSweep: sample_points = {S} > 1024 (ali_cf_select sorts one block's worth of rows)")
        if S < 1:
            raise ValueError(f"MixtureSweep: sample_points = {S}")
        if metric not in self.METRICS:
            raise ValueError(metric)
        if not x.is_cuda:
            raise ValueError("MixtureSweep.run: needs CUDA tensors")
        if not torch.is_tensor(target):
            target = torch.tensor([int(target)], dtype=torch.int32, device=x.device)
        target = target.to(device=x.device, dtype=torch.int32).reshape(1)
        if orig is not None:
            orig = orig.to(device=x.device, dtype=torch.int32).reshape(1)
        x = x.float().contiguous()
        codes = codes.detach().float().contiguous()
        attrs = {k: v.detach().float().contiguous() for k, v in attrs.items()}
        self._constants(S, attrs[self.target_feature].shape[1], x.device)      # (made outside capture)
        if not self.capture:
            return self._sweep(S, metric, x, codes, attrs, target, orig)
        modes = (self.decoder.training, self.classifier.training)
        return self._graphs(lambda *a: self._sweep(S, metric, *a), (x, codes, attrs, target, orig), (S, metric, modes))
