"""Executors of the DeepSCM conditional-VAE family (``deepscm_vae/``): the ELBO, its training step and the
reconstruction loops.

The conv stacks are the ones ``ali_hip.chain`` already runs (``image_scms`` Encoder / Generator shapes without
BatchNorm or Dropout); what sits between them is csrc/vae.hip: ``ali_vae_latent_fwd`` (reparameterisation of all
``num_samples`` draws into the decoder's input rows, conditioning columns and the KL sum in one launch),
``ali_vae_loglik`` (Gaussian log-likelihood, loss and its gradient) and ``ali_vae_latent_bwd`` (head gradient).  The S
decoder passes share weights and the stacks hold no BatchNorm / Dropout, so they are ONE pass over S*B rows, forward and
backward.

  elbo               ``MorphoMNISTVAE.elbo`` / ``VAE.elbo`` / ``WhaleCallVAE.elbo`` on CUDA tensors: one
                     ``torch.autograd.Function`` around the schedule below, so ``(-vae.elbo(...)).backward()`` works.
  VaeStepper         deepscm_vae/mnist.py:179-185 (audio_mnist.py:377-383): zero_grad, -elbo, backward, Adam -- hand
                     scheduled, parameter gradients straight into the flat Adam group, HIP graph per shape.
  VaeReconstructor   mnist.py:213-217, mnist_vae_measured_cf.py:224-233: mean over ``rounds`` of
                     decoder(encoder.sample(x, c), c_cf or c), the rounds as one batched decoder pass.

CPU tensors run the stock torch statement of the same modules (plumbing tests, ``device='cpu'`` callers).
"""
import torch
import torch.nn as nn

from . import ops
from . import source as _source
from .chain import chain_backward, chain_forward, get_plan
from .graphs import GraphCache
from .step import MnistFamily, SpectFamily, _e_plane_grads, _e_planes, mean_of_rounds
from .trainer import FlatGroup, Stepper

DECODER_LOG_VAR = -5.0          # log-variance of p(x | z) (mnist.py:95, audio_mnist.py:282, whalecalls.py:332)


def head_chains(enc):
    """The two 1x1 heads of a ``VAEEncoder`` as one-stage chains.  The wrappers live in the instance ``__dict__``, not
    in the module registry: ``state_dict`` keys and ``parameters()`` stay the reference's."""
    seqs = enc.__dict__.get("_ali_head_seqs")
    convs = (enc.mean_head, enc.log_var_head)
    if seqs is None or any(s[0] is not m for s, m in zip(seqs, convs)):
        seqs = tuple(nn.Sequential(m) for m in convs)
        enc.__dict__["_ali_head_seqs"] = seqs
    return seqs


class _Family:
    """Input assembly of a VAE: the conditioning of ``ali_hip.step``'s families on the VAE's own tables."""

    def __init__(self, vae):
        E, G = vae.encoder, vae.decoder
        if hasattr(E, "cat_keys"):
            self.base = SpectFamily(E, G, E)
            self.hw, self.e_tables, self.g_tables = self.base.hw, self.base.e_tables, self.base.g_tables
        else:
            self.base = MnistFamily
            self.hw = (28, 28)
            self.e_tables, self.g_tables = [E.digit_embedding[0].weight], [G.digit_embedding.weight]
        self.latent = E.mean_head.out_channels

    def conditioning(self, c):
        return self.base.conditioning(c)

    def used(self, c):
        return self.base.used(c)


class _State:
    __slots__ = ("B", "S", "x0", "n_log", "idx", "onehots", "sE", "sM", "sV", "sG", "mean", "lv", "eps", "g_log",
                 "gxhat", "out3", "xhat")


class VaeCore:
    """The hand schedule shared by ``elbo`` (autograd) and ``VaeStepper``: plans of the four chains (encoder stack, two
    heads, decoder stack) and the launches between them."""

    def __init__(self, vae):
        self.vae = vae
        self.fam = _Family(vae)
        hm, hv = head_chains(vae.encoder)
        self.pE, self.pM, self.pV, self.pG = (get_plan(vae.encoder.layers), get_plan(hm), get_plan(hv),
                                              get_plan(vae.decoder.layers))

    def plans(self):
        return (self.pE, self.pM, self.pV, self.pG)

    # ---- forward
    def encode(self, x, cond, save, st=None):
        """(mean, log_var) as [B, L] tensors; ``cond`` = fam.conditioning(c)"""
        fam = self.fam
        idx, cont, onehots = cond
        B = x.shape[0]
        x0, n_log = _e_planes(fam, x, idx, cont)
        training = self.vae.training
        feat, sE = chain_forward(self.pE, x0, training, n_log, save)
        L = fam.latent
        mean, sM = chain_forward(self.pM, feat, training, feat.shape[-1], save)
        lv, sV = chain_forward(self.pV, feat, training, feat.shape[-1], save)
        if st is not None:
            st.x0, st.n_log, st.idx, st.sE, st.sM, st.sV = x0, n_log, idx, sE, sM, sV
        return mean.reshape(B, L), lv.reshape(B, L)

    def decode_rows(self, mean, lv, S, cond, k, eps, rng, save, want_kl):
        """the S*B decoder rows of S draws and the decoder pass over them.  ``rng`` = (seed, device counter) for draws
        made in the kernel (``eps`` None).  Returns (xhat [S*B, P], saved, kl_sum, eps, logical input width)"""
        fam = self.fam
        _, cont, onehots = cond
        B, L = mean.shape
        g_log = L + 256 * len(fam.g_tables) + (0 if cont is None else cont.shape[1])
        ld = g_log + (-g_log) % 32        # channel stride % 32 == 0 -> uniform-tap fast path of the GEMM kernel
        gin = torch.empty(S * B, ld, dtype=torch.float32, device=mean.device)
        seed, ctr = rng if rng is not None else (0, None)
        kl, eps = ops.vae_latent_fwd(mean, lv, S, gin, k=k, eps=eps, seed=seed, dev_counter=ctr, want_eps=save,
                                     onehots=onehots, tables=[t.detach() for t in fam.g_tables], cont=cont,
                                     want_kl=want_kl)
        xhat, sG = chain_forward(self.pG, gin.reshape(S * B, 1, 1, ld), self.vae.training, g_log, save)
        return xhat.reshape(S * B, -1), sG, kl, eps, g_log

    def forward(self, x, c, S, kl_weight, eps=None, rng=None, save=True):
        """-> _State; ``out3`` = [logp, loss = -(logp - kl_weight * mean dkl), mean dkl]"""
        st = _State()
        B = x.shape[0]
        cond = self.fam.conditioning(self.fam.used(c))
        st.B, st.S, st.onehots = B, S, cond[2]
        st.mean, st.lv = self.encode(x, cond, save, st)
        if eps is not None:
            eps = eps.reshape(S, B, -1).float().contiguous()
        st.xhat, st.sG, kl, st.eps, st.g_log = self.decode_rows(st.mean, st.lv, S, cond, 0.5, eps, rng, save, True)
        st.out3, st.gxhat = ops.vae_loglik(x.reshape(B, -1).float().contiguous(), st.xhat, S, DECODER_LOG_VAR, kl,
                                           kl_weight, 1.0, want_grad=save)
        return st

    # ---- backward
    def backward(self, st, kl_weight, grad_dst=None, gxhat=None, kl_scale=None):
        """Gradients of ``loss`` (times ``kl_scale`` when given; ``gxhat`` then already carries it) for every parameter:
        written into ``grad_dst`` {id(param): view} where it names one, returned as {id(param): tensor} otherwise."""
        fam = self.fam
        B, S, L = st.B, st.S, fam.latent
        dst = grad_dst or {}
        grads = {}

        def out_for(p):
            t = dst.get(id(p))
            if t is None:
                t = grads[id(p)] = torch.empty_like(p)
            return t

        gx = st.gxhat if gxhat is None else gxhat
        g_gin, gr = chain_backward(self.pG, st.sG, gx.reshape(st.sG[-1].y.shape), st.g_log, True, True, grad_dst)
        grads.update(gr)
        g_gin = g_gin.reshape(S * B, -1)
        gmean = torch.empty(B, L, dtype=torch.float32, device=g_gin.device)
        glv = torch.empty_like(gmean)
        ncond = 256 * len(fam.g_tables)
        gcond = ops.vae_latent_bwd(g_gin, st.eps, st.mean, st.lv, S, gmean, glv, 0.5, kl_weight, kl_scale, ncond)
        for j, t in enumerate(fam.g_tables):
            ops.g_input_table_grad(st.onehots[j], gcond, 256 * j, out_for(t))
        c_feat = st.sM[0].x_in.shape[-1]
        gfa, gr = chain_backward(self.pM, st.sM, gmean.reshape(B, 1, 1, L), c_feat, True, True, grad_dst)
        grads.update(gr)
        gfb, gr = chain_backward(self.pV, st.sV, glv.reshape(B, 1, 1, L), c_feat, True, True, grad_dst)
        grads.update(gr)
        gfeat = gfa + gfb
        emb = tuple(range(1, 1 + len(fam.e_tables)))       # only these planes of the input gradient are consumed
        g_x0, gr = chain_backward(self.pE, st.sE, gfeat.reshape(st.sE[-1].y.shape), st.n_log, bool(emb), True, grad_dst,
                                  gx_planes=emb or None)
        grads.update(gr)
        _e_plane_grads(fam, g_x0, st.x0, st.idx, out_for)
        return grads


_CORES = {}


def core_of(vae):
    """the (cached) schedule of a VAE instance; keyed by id with the instance kept alive by the entry's weak check"""
    import weakref
    ent = _CORES.get(id(vae))
    if ent is None or ent[0]() is not vae:
        core = VaeCore(vae)
        ent = _CORES[id(vae)] = (weakref.ref(vae, lambda _r, k=id(vae): _CORES.pop(k, None)), core)
        core.vae = weakref.proxy(vae)
    return ent[1]


class ElboFn(torch.autograd.Function):
    """elbo(x, c) of a VAE on the HIP path as one autograd node: forward runs the whole schedule, backward the hand
    schedule; the parameters are its differentiable inputs (``x`` gets no gradient: no caller asks for one)."""

    @staticmethod
    def forward(ctx, core, x, c, S, kl_weight, eps, params, *flat_params):
        need = any(ctx.needs_input_grad[7:])
        st = core.forward(x, c, S, kl_weight, eps=eps, save=need)
        ctx.core, ctx.st, ctx.kl_weight, ctx.params = core, st, kl_weight, params
        return -st.out3[1]

    @staticmethod
    def backward(ctx, g):
        core, st = ctx.core, ctx.st
        scale = (-g).reshape(1).float().contiguous()           # d elbo = -d loss
        grads = core.backward(st, ctx.kl_weight, gxhat=st.gxhat * scale, kl_scale=scale)
        ctx.st = None
        out = []
        for p, need in zip(ctx.params, ctx.needs_input_grad[7:]):
            gp = grads.get(id(p)) if need else None
            out.append(torch.zeros_like(p) if (need and gp is None) else gp)   # (a parameter no path reaches)
        return (None,) * 7 + tuple(out)


def elbo(vae, x, c, num_samples=4, kl_weight=1.0, eps=None):
    """``vae.elbo`` for CUDA tensors; ``eps`` [S, B, L] (optional) replaces the host draws ``torch.randn(...)``."""
    core = core_of(vae)
    B, L = x.shape[0], core.fam.latent
    if eps is None:        # the reference's order of host draws (mnist.py:127), one per sample
        eps = torch.stack([torch.randn(B, L, 1, 1) for _ in range(num_samples)]).to(x.device)
    params = list(vae.parameters())
    return ElboFn.apply(core, x, c, int(num_samples), float(kl_weight), eps, params, *params)


def elbo_torch(vae, x, c, eps, kl_weight):
    """the stock torch statement with given draws ``eps`` [S, B, L]: (elbo, logp, mean dkl)"""
    from deepscm_vae._vae import gaussian_log_prob
    z_mean, z_log_var = vae.encoder(x, c)
    z_std = torch.exp(z_log_var * .5)
    xf = x.reshape(x.shape[0], -1)
    lp = 0
    for e in eps:
        z = z_mean + e.reshape(z_mean.shape).to(z_mean.dtype) * z_std
        lp = lp + gaussian_log_prob(xf, vae.decoder(z, c).reshape(xf.shape), vae.decoder_log_var)
    lp = (lp / len(eps)).mean()
    dkl = (.5 * (torch.square(z_std) + torch.square(z_mean) - 1 - z_log_var).reshape(x.shape[0], -1).sum(dim=1)).mean()
    return lp - kl_weight * dkl, lp, dkl


class VaeStepper(Stepper):
    """One training step of a conditional VAE, hand scheduled:

        opt.zero_grad(); loss = -vae.elbo(x, c, num_samples, kl_weight=kl_weight); loss.backward(); opt.step()

    encoder forward, latent forward, ONE decoder pass over num_samples*B rows, log-likelihood, decoder backward, latent
    backward, head and encoder backward, one flat Adam, pack refresh.  ``step(x, c, eps=None)`` returns {"loss", "logp",
    "kl"} as 0-d device tensors (no host sync).  ``eps`` [S, B, L]: the draws; None: drawn in the latent kernel from the
    counter stream ``ali_hip.source.normal_reference(seed, step number, S*B*L)`` (``seed`` None:
    ``source.DEFAULT_Z_SEED``) -- torch's host generator is left alone.  ``capture=True`` replays the step from a HIP
    graph per input shape."""

    def __init__(self, vae, lr=1e-4, betas=(0.9, 0.999), kl_weight=10, num_samples=4, capture=False, seed=None,
                 eps=1e-8):
        self.vae = vae
        self.kl_weight, self.num_samples = float(kl_weight), int(num_samples)
        self.seed = _source.DEFAULT_Z_SEED if seed is None else int(seed)
        self.on_device = next(vae.parameters()).is_cuda
        if self.on_device:
            self.core = core_of(vae)
            self.opt = FlatGroup(list(vae.parameters()), lr, betas, eps)
        else:
            self.opt = torch.optim.Adam(vae.parameters(), lr=lr, betas=betas, eps=eps)
        self._adopt([(self.opt, self.core.plans())] if self.on_device else [], capture)
        # steps that drew in the kernel
        self.draws = torch.zeros(1, dtype=torch.int64, device=self.opt.flat.device) if self.on_device else 0

    @torch.no_grad()
    def step(self, x, c, eps=None):
        if x.is_cuda != self.on_device:
            raise ValueError("VaeStepper.step: the batch and the model live on different devices")
        if not self.on_device:
            return self._step_torch(x, c, eps)
        c = self.core.fam.used(c)
        return self._run(self._step, (x, c, eps), (self.vae.training,), [self.draws])

    def _step(self, x, c, eps=None):
        core = self.core
        st = core.forward(x, c, self.num_samples, self.kl_weight, eps=eps, rng=(self.seed, self.draws), save=True)
        if eps is None:
            ops.add_i64_multi([self.draws], [1])
        core.backward(st, self.kl_weight, grad_dst=self.opt.grad_views)
        self._update(self.opt)
        return {"loss": st.out3[1], "logp": st.out3[0], "kl": st.out3[2]}

    def _step_torch(self, x, c, eps):
        S = self.num_samples
        if eps is None:
            n = x.shape[0] * self.vae.encoder.mean_head.out_channels
            eps = _source.normal_reference(self.seed, self.draws, S * n).float().reshape(S, x.shape[0], -1)
            self.draws += 1
        eps = eps.reshape(S, x.shape[0], -1)
        _, lp, dkl = elbo_torch(self.vae, x, c, eps, self.kl_weight)         # (the two terms, for the report only)
        with torch.enable_grad():
            self.opt.zero_grad()
            e = self.vae.elbo(x, c, num_samples=S, kl_weight=self.kl_weight, eps=eps)   # the module's own statement
            (-e).backward()
            self.opt.step()
        return {"loss": -e.detach(), "logp": lp, "kl": dkl}


class VaeReconstructor:
    """The reconstruction / counterfactual loops (mnist.py:213-217, mnist_vae_measured_cf.py:224-233):

        recon = 0;  for _ in range(rounds): recon = recon + decoder(encoder.sample(x, c), c_cf or c);  recon / rounds

    ``add(x, c, c_cf=None, eps=None)`` returns that mean image batch: the encoder once (its output does not depend on
    the round), the rounds' latents in one ``ali_vae_latent_fwd`` launch (k = 1: ``sample`` multiplies by
    ``exp(log_var)``), ONE decoder pass over rounds*B rows, the rounds added in the loop's order.  ``eps``
    [rounds, B, L]: the draws; None: drawn in the kernel from the counter stream keyed (seed, call number).  One HIP
    graph per input shape; graphs of older parameter versions are dropped (``GraphCache(modules=...)``)."""

    def __init__(self, vae, rounds=32, capture=True, seed=None):
        self.vae = vae
        self.rounds = int(rounds)
        self.capture = capture
        self.seed = _source.DEFAULT_Z_SEED + 1 if seed is None else int(seed)
        self.calls = None
        self._graphs = GraphCache(modules=[vae])

    def _run(self, x, c, c_cf=None, eps=None):
        core = core_of(self.vae)
        fam = core.fam
        R, B = self.rounds, x.shape[0]
        cond = fam.conditioning(c)
        mean, lv = core.encode(x, cond, False)
        cond_cf = cond if c_cf is None else fam.conditioning(c_cf)
        if eps is not None:
            eps = eps.reshape(R, B, -1).float().contiguous()
        xhat, _, _, _, _ = core.decode_rows(mean, lv, R, cond_cf, 1.0, eps, (self.seed, self.calls), False, False)
        if eps is None:
            ops.add_i64_multi([self.calls], [1])
        return mean_of_rounds(xhat.reshape((R, B, 1) + tuple(fam.hw)))

    def _run_torch(self, x, c, c_cf, eps):
        enc, dec = self.vae.encoder, self.vae.decoder
        mean, log_var = enc(x, c)
        rec = 0
        for r in range(self.rounds):
            e = torch.randn(mean.shape) if eps is None else eps[r].reshape(mean.shape)
            rec = rec + dec(mean + e * torch.exp(log_var), c_cf if c_cf is not None else c)
        return rec / self.rounds

    @torch.no_grad()
    def add(self, x, c, c_cf=None, eps=None):
        if not x.is_cuda:
            return self._run_torch(x, c, c_cf, eps)
        fam = core_of(self.vae).fam
        c = fam.used(c)
        c_cf = None if c_cf is None else fam.used(c_cf)
        if self.calls is None or self.calls.device != x.device:
            self.calls = torch.zeros(1, dtype=torch.int64, device=x.device)
        if not self.capture:
            return self._run(x, c, c_cf, eps)
        # (state: the warm-up pass is no call of the counter stream)
        return self._graphs(self._run, (x, c, c_cf, eps), (self.vae.training,), [self.calls])
