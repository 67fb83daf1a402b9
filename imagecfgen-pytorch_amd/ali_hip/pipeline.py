"""The pass the explainer executors (``explain.py``, ``attrib.py``, ``contrast.py``) share between their own kernels:
generator input rows through the generator's chain, the image through the classifier's chain, and the data gradient
of the logits back to the rows.  ``DecodeClassify`` is the one place that knows the conventions of that
pass: the rows enter as a [R,1,1,ld] map of ``n_log`` real channels, the image is [R,1,H,W] and enters the classifier
NHWC, padded to four channels of which one is real, the backward passes compute no parameter gradient
(``need_params=False``: no parameter and no ``.grad`` is touched), the classifier's input gradient is made contiguous
and its plane 0 goes on to the generator through ``ali_cf_join``.

``Decoder`` is what the executors need of a generator stack, ``LayoutCache`` keeps their segment tables
(``ops.CfLayout``) in step with the embedding tables they point into.
"""
from . import ops
from .chain import chain_backward, chain_forward, get_plan, saved_rows, trace
from .classify import nhwc_input


class Decoder:
    """What the executors need of a generator stack: its layers' plan, the embedding tables, and which attribute goes
    where in the input row ``[z | attribute @ table ... | continuous ... | 0]``."""

    def __init__(self, G):
        from image_scms._spect import SpectGenerator
        from image_scms.mnist import Generator
        self.G = G
        if isinstance(G, Generator):
            self.spect = False
        elif isinstance(G, SpectGenerator):
            self.spect = True
        else:
            raise TypeError(f"explain: {type(G).__name__} is not one of this package's generator stacks")
        self.layers = G.layers

    def keys(self, attrs):
        """(table keys, continuous keys) in the order of the input row"""
        if self.spect:
            cat = list(self.G.cat_keys)
            cont = [self.G.cont_key] if self.G.cont_key is not None else []
        else:
            from image_scms.mnist import _cont_keys
            cat, cont = ["digit"], list(_cont_keys(attrs))
        if set(cat + cont) != set(attrs):
            raise ValueError(f"explain: the decoder takes the attributes {cat + cont}, got {list(attrs)}")
        return cat, cont

    def tables(self, cat):
        if self.spect:
            return [self.G.table(k).weight.detach() for k in cat]
        return [self.G.digit_embedding.weight.detach()]

    def latent(self):
        if self.spect:
            from image_scms._spect import LATENT_DIM
        else:
            from image_scms.mnist import LATENT_DIM
        return LATENT_DIM

    def image_hw(self):
        if self.spect:
            return tuple(self.G.image_hw)
        return (28, 28)

    def row_width(self, cat, cont):
        """(n_log, ld): the logical width of the input row and its width padded to a multiple of 32"""
        n_log = self.latent() + ops.CF_EMB * len(cat) + len(cont)
        return n_log, n_log + (-n_log) % 32


def check_classifier(clf):
    from classifiers._stack import ClassifierStack
    if not isinstance(clf, ClassifierStack):
        raise TypeError(f"explain: {type(clf).__name__} is not a ClassifierStack")


def require_eval(who, **modules):
    """``ValueError`` if one of the named modules is in training mode"""
    for name, m in modules.items():
        if m.training:
            raise ValueError(f"{who}: the {name} is in training mode; {who} is defined in eval mode only "
                             "(call .eval())")


class DecodeClassify:
    """The pass over a generator stack (optional: ``ContrastiveSearch`` has none) and a ``ClassifierStack``.  Every
    method makes the chains' launches and nothing else; the modules' own ``training`` flags are the chains'."""

    def __init__(self, classifier, decoder=None):
        self.dec = None if decoder is None else Decoder(decoder)
        check_classifier(classifier)
        self.classifier = classifier

    def classify(self, images, save=False):
        """images [R,1,H,W] -> (logits [R, C], the classifier's saved state)"""
        logits, saved = chain_forward(get_plan(self.classifier), nhwc_input(images), self.classifier.training, 1, save)
        return logits.reshape(logits.shape[0], -1), saved

    def generate(self, rows, n_log, save=False):
        """input rows [R, ld] of ``n_log`` real columns -> (images [R,1,H,W], the generator's saved state)"""
        R, ld = rows.shape
        xg, saved = chain_forward(get_plan(self.dec.layers), rows.reshape(R, 1, 1, ld), self.dec.G.training, n_log, save)
        return xg.reshape((R, 1) + self.dec.image_hw()), saved

    def forward(self, rows, n_log, save=False):
        """both in sequence -> (images [R,1,H,W], logits [R, C], the saved state of both chains)"""
        x_cf, sG = self.generate(rows, n_log, save)
        logits, sC = self.classify(x_cf, save)
        return x_cf, logits, (sG, sC)

    def image_grad(self, saved, glogit, rows=None):
        """The classifier's NHWC input gradient [R,H,W,4], contiguous, of the logit gradient ``glogit`` [R, C] under
        its saved state.  ``rows`` = (lo, hi): the gradient of those rows of the forward batch alone (R = hi - lo; a
        stack without BatchNorm)."""
        if rows is not None:
            saved = saved_rows(saved, *rows)
        gx, _ = chain_backward(get_plan(self.classifier), saved, glogit.reshape(saved[-1].out_shape), 1, True,
                               need_params=False)
        return gx.contiguous()

    def row_grad(self, saved, glogit, x_cf, x_ref=None):
        """The gradient [R, ld] of the input rows under ``forward``'s saved state: the classifier's data gradient of
        ``glogit``, plane 0 of it joined with the gradient of mean |x_ref - x_cf| (``ali_cf_join``; x_ref [R or 1, N];
        None: no distance term -- x_cf against itself, sign(0) = 0), then the generator's data gradient."""
        sG, sC = saved
        xc = x_cf.reshape(x_cf.shape[0], -1)
        gy = ops.cf_join(self.image_grad(sC, glogit), xc, xc if x_ref is None else x_ref)
        g_rows, _ = chain_backward(get_plan(self.dec.layers), sG, gy.reshape(sG[-1].out_shape), sG[0].c_log, True,
                                   need_params=False)
        return g_rows.reshape(xc.shape[0], -1)

    def shapes(self, n_log, ld):
        """(classes C, bytes of saved activations per generator-input row): from the two plans, no launch"""
        H, W = self.dec.image_hw()
        tG = trace(get_plan(self.dec.layers), (1, 1, 1, ld), n_log)
        tC = trace(get_plan(self.classifier), (1, H, W, 4), 1)
        numel = lambda s: s[0] * s[1] * s[2] * s[3]  # noqa: E731
        # every stage keeps its input and its output; a stage's input is the output of the one before
        saved = sum(numel(t[0][0]) + sum(numel(o) for _, o, _ in t) for t in (tG, tC))
        return tC[-1][1][3], 4 * saved


class LayoutCache:
    """{key: ops.CfLayout} of one executor.  A layout holds the addresses of the decoder's embedding tables, and so do
    the launches recorded with it: when a table has moved (``.to()``, a loaded checkpoint), ``get`` builds the layout
    anew and calls ``dropped()``, in which the owner forgets its graphs and whatever else it keys by a layout's id --
    the old layout is released after that, and its id may be taken again."""

    def __init__(self, decoder: Decoder, dropped):
        self.dec, self.dropped = decoder, dropped
        self._layouts = {}

    def get(self, key, build):
        """the layout of ``key``; ``build()`` makes a missing or stale one: an ``ops.CfLayout`` over the decoder's
        current tables whose ``cat`` names their keys"""
        lay = self._layouts.get(key)
        if lay is not None and all(a.data_ptr() == b.data_ptr() for a, b in zip(lay.tables, self.dec.tables(lay.cat))):
            return lay
        new = self._layouts[key] = build()
        if lay is not None:
            self.dropped()
        return new
