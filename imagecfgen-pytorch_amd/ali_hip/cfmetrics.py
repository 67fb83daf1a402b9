"""Executors of the counterfactual-metrics family (``train_morphomnist_ae.py`` and the two scripts that turn
counterfactuals into result tables, ``morphomnist_cf_metrics.py`` and ``mnist_oracle_scores.py``).

The autoencoders are two conv stacks ``ali_hip.chain`` runs as stages (``Conv2d -> ReLU`` twice and a ``Flatten ->
Linear`` on a 7 x 7 map; ``Linear + Unflatten`` and two stride-2 ``ConvTranspose2d``).  What sits between the stacks
is csrc/cfmetrics.hip: ``ali_mse`` (loss and the gradient of the tanh stage's pre-activation), ``ali_cf_recon`` (the
l1 / o_rec / t_rec / all_rec cells of B rows) and ``ali_oracle_scores`` (the os / lvs cells of B rows and J oracles).

  encode / decode   ``Encoder.forward`` / ``Decoder.forward`` on CUDA tensors: one autograd node each.
  AeStepper         train_morphomnist_ae.py:100-104: forward of both chains, ``ali_mse``, hand-scheduled backward
                    through G then E, one flat Adam over both parameter lists, pack refresh; HIP graph per shape.
  CfMetrics         what the scripts compute for one counterfactual after the explainers have run -- the classifier's
                    label, every autoencoder's reconstruction, the reconstruction cells, every oracle on the original
                    and the counterfactual, the oracle cells -- for B rows at once, one HIP graph per shape, columns
                    kept on the device until ``table()``.
  js_div            mnist_oracle_scores.py:19-28 as a torch statement (CPU callers, the tests' reference).

CPU tensors run the torch statement of the same loops, in the dtype of the modules (fp64 capable).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .chain import chain_backward, chain_forward, get_plan, run_chain
from .classify import nhwc_input
from .graphs import GraphCache
from .trainer import FlatGroup, Stepper


def _latent_rows(z: torch.Tensor, latent: int) -> torch.Tensor:
    """[B, latent] codes -> the Decoder chain's input rows [B, 1, 1, latent padded to a multiple of 4] (pad: zero)"""
    z = z.reshape(-1, latent).float()
    return F.pad(z, (0, (-latent) % 4)).reshape(z.shape[0], 1, 1, -1).contiguous()


def encode(E, x: torch.Tensor) -> torch.Tensor:
    """``Encoder.forward`` on a CUDA batch [B,1,28,28] -> [B, latent]"""
    x = x.reshape((-1, 1) + tuple(x.shape[-2:]))
    return run_chain(E.chain_view(), nhwc_input(x), 1).reshape(x.shape[0], -1)


def decode(G, z: torch.Tensor) -> torch.Tensor:
    """``Decoder.forward`` on CUDA codes [B, latent] -> [B,1,28,28]"""
    latent = G.fc.in_features
    y = run_chain(G.chain_view(), _latent_rows(z, latent), latent)      # NHWC [B,H,W,1]: the memory of [B,1,H,W]
    return y.reshape(y.shape[0], 1, y.shape[1], y.shape[2])


def _reconstruct(E, G, x_nhwc, out_rows=None):
    """G(E(x)) without autograd for an NHWC batch; the last stage writes into ``out_rows`` [B, H*W] when given.
    Returns the reconstruction as [B, H*W]."""
    pE, pG = get_plan(E.chain_view()), get_plan(G.chain_view())
    latent = G.fc.in_features
    z, _ = chain_forward(pE, x_nhwc, E.training, 1, False)
    last = len(pG.stages) - 1
    alloc = None
    if out_rows is not None:
        def alloc(tag, shape):
            if tag == ("y", last):
                return out_rows.view(shape)
            return torch.empty(shape, dtype=torch.float32, device=out_rows.device)
    y, _ = chain_forward(pG, _latent_rows(z, latent), G.training, latent, False, alloc=alloc)
    return y.reshape(y.shape[0], -1)


class AeStepper(Stepper):
    """One iteration of train_morphomnist_ae.py:100-104, hand scheduled (no autograd engine):

        opt.zero_grad(); loss = (x - G(E(x))).square().mean(); loss.backward(); opt.step()

    ``step(x)``, x [B,1,28,28] in [-1, 1], returns {"loss"} as a 0-d device tensor (no host sync).  ``ali_mse`` hands
    the Decoder chain the gradient of its tanh stage's pre-activation, so the backward pass starts at the last
    convolution.  E's and G's parameters move into ONE flat buffer (``FlatGroup``: one Adam launch);
    ``capture=True`` replays the iteration from a HIP graph per input shape; the ``loss`` it returns is then the
    graph's own output tensor, the SAME tensor on every step of that shape, overwritten by the next one: add it into an
    accumulator (as ``train`` does) or ``.clone()`` it to keep it.  CPU modules run the torch statement."""

    def __init__(self, E, G, lr=1e-4, betas=(0.5, 0.9), eps=1e-8, capture=False):
        self.E, self.G = E, G
        self.on_device = next(E.parameters()).is_cuda
        if self.on_device != next(G.parameters()).is_cuda:
            raise ValueError("AeStepper: E and G live on different devices")
        params = list(E.parameters()) + list(G.parameters())
        if self.on_device:
            self.pE, self.pG = get_plan(E.chain_view()), get_plan(G.chain_view())
            self.latent = G.fc.in_features
            self.opt = FlatGroup(params, lr, betas, eps)
        else:
            self.opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps)
        self._adopt([(self.opt, [self.pE, self.pG])] if self.on_device else [], capture)

    @torch.no_grad()
    def step(self, x):
        if x.is_cuda != self.on_device:
            raise ValueError("AeStepper.step: the batch and the models live on different devices")
        if not self.on_device:
            return self._step_torch(x)
        x = x.reshape((-1, 1) + tuple(x.shape[-2:])).float()
        return self._run(self._step, (x,), (self.E.training, self.G.training))

    def _step(self, x):
        B, latent = x.shape[0], self.latent
        x_in = nhwc_input(x)
        z, sE = chain_forward(self.pE, x_in, self.E.training, 1, True)                       # [B,1,1,latent]
        y, sG = chain_forward(self.pG, _latent_rows(z, latent), self.G.training, latent, True)   # [B,28,28,1]
        loss, g_pre = ops.mse(y.reshape(B, -1), x.reshape(B, -1).contiguous(), tanh_out=True)
        views = self.opt.grad_views
        gz, _ = chain_backward(self.pG, sG, g_pre.reshape(y.shape), latent, True, True, views, gy_pre=True)
        gz = gz.reshape(B, -1)[:, :latent].contiguous().reshape(z.shape)
        chain_backward(self.pE, sE, gz, 1, False, True, views)
        self._update(self.opt)
        return {"loss": loss}

    def _step_torch(self, x):
        with torch.enable_grad():
            self.opt.zero_grad()
            x = x.reshape((-1, 1) + tuple(x.shape[-2:]))
            loss = (x - self.G(self.E(x))).square().mean()
            loss.backward()
            self.opt.step()
        return {"loss": loss.detach()}


def js_div(p_logits: torch.Tensor, q_logits: torch.Tensor) -> torch.Tensor:
    """Jensen-Shannon divergence per row of two [B, C] logit batches, with the scripts' 1e-6 inside the logarithms"""
    p, q = p_logits.softmax(1), q_logits.softmax(1)
    m = 0.5 * (p + q)
    lm = (m + 1e-6).log()
    return 0.5 * ((p * ((p + 1e-6).log() - lm)).sum(1) + (q * ((q + 1e-6).log() - lm)).sum(1))


def _num_classes(clf) -> int:
    last = None
    for m in clf.modules():
        if isinstance(m, nn.Linear):
            last = m
    if last is None:
        raise ValueError("CfMetrics: the classifier has no Linear layer to read its class count from")
    return last.out_features


class CfMetrics:
    """The evaluation the two scripts run per counterfactual, for B rows at once:

        label   = clf(cf).argmax(1)                               target = label when none is given
        l1      = |cf|.sum()                                      o_rec = (cf - ae[orig](cf))^2.sum()
        t_rec   = (cf - ae[target](cf))^2.sum()                   all_rec = (ae[target](cf) - ae["all"](cf))^2.sum()
        os_j    = label == oracle_j(cf).argmax(1)                 lvs_j = js_div(oracle_j(x), oracle_j(cf))

    ``aes`` maps every class index of ``clf`` and "all" to an (Encoder, Decoder) pair.  EVERY autoencoder runs on every
    row (A times the minimum work: picking rows by label would need a host read or a device sort per batch) into one
    [A, B, N] buffer that ``ali_cf_recon`` indexes by the device labels; every oracle runs once on the 2B rows of
    ``x`` and ``cf``.  ``add`` makes no host read and replays one HIP graph per input shape (``capture``); graphs are
    dropped when a weight changes.  It returns the batch's columns as device tensors and appends them to device-side
    buffers; ``table(prefix)`` is the one host read, ``reset()`` clears the buffers."""

    def __init__(self, clf, aes, oracles=(), capture=True):
        self.clf, self.oracles, self.capture = clf, list(oracles), capture
        self.n_cls = _num_classes(clf)
        missing = [k for k in list(range(self.n_cls)) + ["all"] if k not in aes]
        if missing:
            raise ValueError(f"CfMetrics: no autoencoder for {missing} (the classifier has {self.n_cls} classes; 'all' "
                             f"is the autoencoder of every class)")
        self.aes = [tuple(aes[k]) for k in list(range(self.n_cls)) + ["all"]]
        mods = [clf] + [m for pair in self.aes for m in pair] + self.oracles
        self._graphs = GraphCache(modules=mods)
        self._modules = mods
        self._rows = []

    # ------------------------------------------------------------------ one batch
    def _run_device(self, x, cf, orig, target):
        B, J, A = cf.shape[0], len(self.oracles), len(self.aes)
        dev = cf.device
        cf = cf.reshape((B, 1) + tuple(cf.shape[-2:])).float().contiguous()
        N = cf.shape[-2] * cf.shape[-1]
        label = self.clf(cf).argmax(1).to(torch.int32)
        orig = orig.reshape(B).to(torch.int32)
        target = label if target is None else target.reshape(B).to(torch.int32)
        cf_in = nhwc_input(cf)
        recon = torch.empty(A, B, N, dtype=torch.float32, device=dev)
        for a, (E, G) in enumerate(self.aes):
            _reconstruct(E, G, cf_in, recon[a])
        rec = ops.cf_recon(cf.reshape(B, N), recon, orig, target)
        out = {"label": label, "l1": rec[:, 0], "o_rec": rec[:, 1], "t_rec": rec[:, 2], "all_rec": rec[:, 3]}
        cols = [label.float().reshape(B, 1), rec]
        if J:
            both = torch.cat([x.reshape(cf.shape).float(), cf])
            logits = [o(both).reshape(2, B, -1).contiguous() for o in self.oracles]
            pair = torch.empty((J, 2) + tuple(logits[0].shape[1:]), dtype=torch.float32, device=dev)
            ops.copy_multi([(pair[j], lg) for j, lg in enumerate(logits)])
            out["os"], out["lvs"] = ops.oracle_scores(label, pair[:, 0], pair[:, 1])
            cols += [out["os"].float(), out["lvs"]]
        else:
            out["os"] = torch.empty(B, 0, dtype=torch.int32, device=dev)
            out["lvs"] = torch.empty(B, 0, dtype=torch.float32, device=dev)
        out["row"] = torch.cat(cols, dim=1)           # [B, 5 + 2J]: what ``table`` reads (small integers are exact)
        return out

    def _run_torch(self, x, cf, orig, target):
        B = cf.shape[0]
        cf = cf.reshape((B, 1) + tuple(cf.shape[-2:]))
        label = self.clf(cf).argmax(1)
        target = label if target is None else target.reshape(B).long()
        orig = orig.reshape(B).long()
        flat = cf.reshape(B, -1)
        recon = torch.stack([G(E(cf)).reshape(B, -1) for E, G in self.aes])          # [A, B, N]
        rows = torch.arange(B)
        r_o, r_t = recon[orig, rows], recon[target, rows]
        out = {"label": label, "l1": flat.abs().sum(1), "o_rec": (flat - r_o).square().sum(1),
               "t_rec": (flat - r_t).square().sum(1), "all_rec": (r_t - recon[-1]).square().sum(1)}
        os_, lvs = [], []
        for o in self.oracles:
            lx, lc = o(x.reshape(cf.shape)), o(cf)
            os_.append((label == lc.argmax(1)).to(torch.int32))
            lvs.append(js_div(lx, lc))
        out["os"] = torch.stack(os_, 1) if os_ else torch.empty(B, 0, dtype=torch.int32)
        out["lvs"] = torch.stack(lvs, 1) if lvs else flat.new_empty(B, 0)
        dt = flat.dtype
        out["row"] = torch.cat([label.to(dt).reshape(B, 1)] + [out[k].reshape(B, 1) for k in ("l1", "o_rec", "t_rec",
                                                                                             "all_rec")]
                               + [out["os"].to(dt), out["lvs"]], dim=1)
        return out

    @torch.no_grad()
    def add(self, x, cf, orig, target=None):
        """x, cf [B,1,28,28]; orig, target int tensors [B] (``target=None``: the predicted label, as the scripts' cf / pn
        columns; the explainer columns pass the class that was asked for).  Returns {"label", "l1", "o_rec", "t_rec",
        "all_rec", "os" [B,J], "lvs" [B,J]} on the batch's device: tensors of the caller's own, which later calls leave
        alone (the outputs of a replayed graph are copied out)."""
        if not cf.is_cuda:
            out = self._run_torch(x, cf, orig, target)
        elif not self.capture:
            out = self._run_device(x, cf, orig, target)
        else:       # (a replay writes the tensors the recording returned: the caller gets copies of its own)
            out = self._graphs(self._run_device, (x, cf, orig, target), tuple(m.training for m in self._modules))
            out = {k: v.clone() for k, v in out.items()}
            self._rows.append(out["row"])
            return {k: v for k, v in out.items() if k != "row"}
        self._rows.append(out["row"].clone())
        return {k: v for k, v in out.items() if k != "row"}

    def table(self, prefix):
        """The columns of every row added so far under the scripts' names, as numpy arrays (the one host read)."""
        J = len(self.oracles)
        if self._rows:
            rows = torch.cat(self._rows).cpu().numpy()
        else:
            rows = np.zeros((0, 5 + 2 * J), dtype=np.float32)
        out = {f"{prefix}_label": rows[:, 0].astype(np.int64)}
        for i, name in enumerate(("l1", "o_rec", "t_rec", "all_rec")):
            out[f"{name}_{prefix}"] = rows[:, 1 + i]
        for j in range(J):
            out[f"{prefix}_os_{j}"] = rows[:, 5 + j].astype(np.int64)
            out[f"{prefix}_lvs_{j}"] = rows[:, 5 + J + j]
        return out

    def reset(self):
        self._rows = []
