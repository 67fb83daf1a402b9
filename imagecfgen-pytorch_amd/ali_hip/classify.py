"""Executors of the classifier family (``classifiers/``): the training step and the scoring loops.

The classifiers are ``nn.Sequential`` stacks of 3x3 unpadded convolutions that end in ``Flatten -> Linear`` (one more
``Linear`` in the spectrogram models); ``ali_hip.chain`` runs them as stages, ``ali_softmax_xent`` (csrc/xent.hip) is
their loss, gradient, arg-max and hit count in one launch.

  ClassifierStepper   classifiers/mnist.py:48-56 (and audio_mnist.py:257-266, whalecalls.py:296-305):
                      forward, cross-entropy, hand-scheduled backward, flat Adam, pack refresh; HIP graph per shape.
  ClassifierScorer    the ``(labels.argmax(1) == clf(x).argmax(1)).sum()`` of every scoring loop, hits kept in device
                      counters: one host read per ``result()``, none per batch.
  GeneratorScore      audiomnist_generator_score.py:83-98 (mnist_generator_score.py:69-74 and whale_generator_score.py
                      are its mc_rounds = 1 case): mc-round mean image, every classifier, the counters -- one graph.

CPU tensors run the stock torch statement of the same loop (plumbing tests, ``device='cpu'`` callers).
"""
import torch
import torch.nn.functional as F

from . import ops
from .chain import chain_backward, chain_forward, get_plan
from .graphs import GraphCache
from .step import GeneratorSampler
from .trainer import FlatGroup, Stepper


def nhwc_input(x: torch.Tensor) -> torch.Tensor:
    """[B,C,H,W] image batch -> the chain's NHWC input, channels zero-padded to a multiple of 4"""
    x = x.float().permute(0, 2, 3, 1)
    return F.pad(x, (0, (-x.shape[-1]) % 4)).contiguous()


class ClassifierStepper(Stepper):
    """One training step of a classifier stack, hand scheduled:

        opt.zero_grad(); pred = model(x); loss = CrossEntropyLoss()(pred, y); loss.backward(); opt.step()
        hits = (pred.argmax(1) == y.argmax(1)).sum()

    ``y``: float one-hot or soft rows [B, num_classes].  ``step`` returns {"loss", "hits"} as 0-d device tensors (no host
    sync).  The parameters move into one flat buffer (``FlatGroup``: one Adam launch); ``capture=True`` replays the step
    from a HIP graph per input shape."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, capture=False):
        self.model = model
        self.on_device = next(model.parameters()).is_cuda
        if self.on_device:
            self.plan = get_plan(model)
            self.opt = FlatGroup(list(model.parameters()), lr, betas, eps)
        else:
            self.opt = torch.optim.Adam(model.parameters(), lr=lr, betas=betas, eps=eps)
        self._adopt([(self.opt, [self.plan])] if self.on_device else [], capture)

    @torch.no_grad()
    def step(self, x, y):
        if x.is_cuda != self.on_device:
            raise ValueError("ClassifierStepper.step: the batch and the model live on different devices")
        if not self.on_device:
            return self._step_torch(x, y)
        return self._run(self._step, (x, y.float()), (self.model.training,))

    def _step(self, x, y):
        B = x.shape[0]
        c_log = x.shape[1]
        logits, saved = chain_forward(self.plan, nhwc_input(x), self.model.training, c_log, True)
        out2, glogit, _ = ops.softmax_xent(logits.reshape(B, -1), y.contiguous())
        chain_backward(self.plan, saved, glogit.reshape(logits.shape), c_log, False, True, self.opt.grad_views)
        self._update(self.opt)
        return {"loss": out2[0], "hits": out2[1]}

    def _step_torch(self, x, y):
        with torch.enable_grad():
            self.opt.zero_grad()
            pred = self.model(x)
            loss = F.cross_entropy(pred, y.float())
            loss.backward()
            self.opt.step()
        hits = (pred.argmax(1) == y.argmax(1)).sum().float()
        return {"loss": loss.detach(), "hits": hits}


class ClassifierScorer:
    """Accuracy of several classifiers over a stream of batches:

        for name, clf in models.items():  n_correct[name] += (labels[name].argmax(1) == clf(images).argmax(1)).sum()

    ``add(images, labels)`` runs every classifier on the batch and adds its hits into that classifier's int64 counter
    ON THE DEVICE (``ali_softmax_xent(hits_accum=...)``), all of it one HIP graph per input shape; ``result()`` is the
    one host read, {name: hits / seen}; ``reset()`` clears the counters.  Graphs captured for older weights are dropped
    when a parameter's version changes (``GraphCache(modules=...)``)."""

    def __init__(self, models, capture=True):
        self.models = dict(models)
        self.capture = capture
        self.seen = 0
        self.counters = None
        self._graphs = GraphCache(modules=self.models.values())

    def _ensure_counters(self, device):
        if self.counters is None or self.counters.device != device:
            self.counters = torch.zeros(len(self.models), dtype=torch.int64, device=device)

    def _score(self, images, labels):
        """every classifier on ``images``; hits into the counters (no host read)"""
        for i, (name, clf) in enumerate(self.models.items()):
            pred = clf(images)
            y = labels[name]
            if images.is_cuda:
                ops.softmax_xent(pred.contiguous(), y.float().contiguous(), want_grad=False,
                                 hits_accum=self.counters[i:i + 1])
            else:
                self.counters[i] += (pred.argmax(1) == y.argmax(1)).sum()

    @torch.no_grad()
    def add(self, images, labels):
        labels = {k: labels[k] for k in self.models}
        self._ensure_counters(images.device)
        self.seen += images.shape[0]
        if not (self.capture and images.is_cuda):
            return self._score(images, labels)
        # (state: the warm-up pass is no batch of the stream)
        self._graphs(self._score, (images, labels), tuple(m.training for m in self.models.values()), [self.counters])

    def result(self):
        hits = self.counters.tolist() if self.counters is not None else [0] * len(self.models)
        return {name: h / max(self.seen, 1) for name, h in zip(self.models, hits)}

    def reset(self):
        self.seen = 0
        if self.counters is not None:
            self.counters.zero_()


class GeneratorScore:
    """The body of the generator-score loops (audiomnist_generator_score.py:83-98):

        gen = mean over mc_rounds of G(randn(B, 512, 1, 1), attrs);  every classifier on gen;  hits += ...

    ``models`` maps an attribute name to the classifier that predicts it from the image.  ``add(attrs, zs=None)`` runs
    one batch -- ``GeneratorSampler``'s batched rounds, then ``ClassifierScorer``'s classifiers and counters -- as ONE
    HIP graph per input shape; ``zs`` [mc_rounds, B, latent, 1, 1] are the latent draws (drawn here when None)."""

    def __init__(self, G, models, mc_rounds=1, capture=True, latent_dim=512):
        self.G = G
        self.mc_rounds = int(mc_rounds)
        self.latent_dim = latent_dim
        self.capture = capture
        self.sampler = GeneratorSampler(G, capture=False)
        self.scorer = ClassifierScorer(models, capture=False)
        self._graphs = GraphCache(modules=[G, *self.scorer.models.values()])

    def _run(self, zs, attrs):
        gen = self.sampler._forward(zs, attrs)
        self.scorer._score(gen, attrs)
        return gen

    @torch.no_grad()
    def add(self, attrs, zs=None):
        some = next(iter(attrs.values()))
        B, device = some.shape[0], some.device
        if zs is None:
            zs = torch.randn(self.mc_rounds, B, self.latent_dim, 1, 1, device=device)
        if zs.dim() == 4:
            zs = zs.unsqueeze(0)
        sc = self.scorer
        sc._ensure_counters(device)
        sc.seen += B
        if not (self.capture and zs.is_cuda):
            return self._run(zs, attrs)
        return self._graphs(self._run, (zs, attrs), (self.G.training, tuple(m.training for m in sc.models.values())),
                            [sc.counters])

    def result(self):
        return self.scorer.result()

    def reset(self):
        self.scorer.reset()
