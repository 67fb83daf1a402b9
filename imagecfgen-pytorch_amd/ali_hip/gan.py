"""Executors of the unconditional GAN family (``gans/``): the WGAN-GP gradient penalty and the training iteration.

The Generator is ``Linear + Unflatten`` and five stride-2 ``ConvTranspose2d``, the Discriminator five unpadded stride-2
``Conv2d`` with LeakyReLU and a ``Flatten + Linear`` head: stage kinds ``ali_hip.chain`` already runs.  What sits between
them is csrc/gan.hip: ``ali_gp_mix`` (the interpolates), ``ali_gp_penalty`` (per-image gradient norm, penalty, tangent)
and ``ali_wgan_critic`` (the critic loss and its constant gradients).

The Discriminator has no BatchNorm and no Dropout, so it is piecewise linear in its input and the penalty needs no
general double backward (``ali_hip.chain``: "gradient of a gradient norm"): a backward pass from gy = 1 that keeps the
pre-activation gradients h_l gives g0 = d sum_b D(xhat_b) / d xhat; ``ali_gp_penalty`` turns it into the penalty and the
tangent v = d(weight * penalty) / d g0; one more FORWARD pass u_l = act'(a_l) * conv(W_l, u_{l-1}) from u_0 = v and one
ordinary weight-gradient launch per layer, dW_l = bwd_weight(u_{l-1}, h_l), give the penalty's parameter gradients.
Biases and the interpolates get exactly zero -- stock autograd agrees: ``leaky_relu``'s double backward is zero.

  GradientPenaltyFn   ``compute_gradient_penalty(disc, interpolates)`` on CUDA tensors as one autograd node, so that
                      ``wgan_loss_it(D, x, G(z)).mean().backward()`` works unchanged.
  GanStepper          gans/audio_mnist.py:287-337: generator step, discriminator step (BCE or critic + penalty), the
                      two scores -- hand scheduled, flat Adam groups, HIP graph per shape.
"""
import torch
import torch.nn.functional as F

from . import ops
from . import source as _source
from .chain import (chain_backward, chain_backward_keep, chain_forward, chain_param_grads, chain_tangent, get_plan,
                    saved_rows, tangent_param_grads)
from .trainer import FlatGroup, Stepper, load_module_state_, module_state_cpu

LATENT_DIM = 100
LATENT_LD = 128          # channel stride of the Generator's input rows: % 32 == 0 -> the GEMM's uniform-tap loop


def d_input(x: torch.Tensor) -> torch.Tensor:
    """[B, 1, H, W] (or [B, H, W, 1]: the same memory) image batch -> the Discriminator chain's NHWC input, the one
    channel zero-padded to four"""
    if x.dim() == 4:
        x = x[:, 0] if x.shape[1] == 1 else x[..., 0]
    return F.pad(x.float().unsqueeze(-1), (0, 3))


def g_input(z: torch.Tensor) -> torch.Tensor:
    """latents [B, 100(, 1, 1)] -> the Generator chain's input rows [B, 1, 1, 128] (columns >= 100 zero)"""
    z = z.float().reshape(-1, LATENT_DIM)
    return F.pad(z, (0, LATENT_LD - LATENT_DIM)).reshape(z.shape[0], 1, 1, LATENT_LD)


def _one_plane(gx):
    """the first stage's data gradient as [B, H, W, 1] (``gx_planes=(0,)`` gives it directly where the route has a
    plane form; the full padded gradient otherwise)"""
    return gx if gx.shape[-1] == 1 else gx[..., :1].contiguous()


class GradientPenaltyFn(torch.autograd.Function):
    """mean_b (||d sum D(xhat) / d xhat_b||_2 - 1)^2 of a plain conv stack ``plan`` at ``xhat`` [B, 1, H, W]
    (UNWEIGHTED: ``wgan_loss_it`` applies the weight).  Differentiable inputs: the stack's parameters
    (``plan.params()`` order).  Backward returns the tangent-pass weight gradients times the incoming gradient, zero
    for every bias and zero for ``xhat``."""

    @staticmethod
    def forward(ctx, plan, xhat, *params):
        B = xhat.shape[0]
        y, saved = chain_forward(plan, d_input(xhat), plan.seq().training, 1, True)
        g0, hs = chain_backward_keep(plan, saved, torch.ones_like(y), 1, True, gx_planes=(0,))
        g0 = _one_plane(g0)
        need = any(ctx.needs_input_grad[2:])
        out2, v = ops.gp_penalty(g0.reshape(B, -1), 1.0, want_v=need, out=g0.reshape(B, -1) if need else None)
        ctx.plan, ctx.state, ctx.norm = plan, (saved, hs, v) if need else None, out2[1]
        ctx.param_ids = [id(p) for p in plan.params()]
        ctx.weight_ids = {id(st.mod.weight) for st in plan.stages}
        return out2[0].clone()

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        saved, hs, v = ctx.state
        u0 = F.pad(v.reshape(saved[0].in_shape[:3] + (1,)), (0, saved[0].in_shape[3] - 1))
        us = chain_tangent(plan, saved, u0)
        grads = tangent_param_grads(plan, saved, us, hs, head_ones=True)
        out = []
        for p, pid, need in zip(plan.params(), ctx.param_ids, ctx.needs_input_grad[2:]):
            if not need:
                out.append(None)
            elif pid in ctx.weight_ids:
                out.append(grads[pid] * g)
            else:
                out.append(torch.zeros_like(p))
        gx = torch.zeros(saved[0].in_shape[:3], device=g.device).unsqueeze(1) if ctx.needs_input_grad[1] else None
        return (None, gx) + tuple(out)


def gradient_penalty(disc, interpolates):
    """``compute_gradient_penalty`` for a CUDA batch and a Discriminator whose ``layers`` the chain runs"""
    plan = get_plan(disc.layers)
    x = interpolates.reshape((-1, 1) + tuple(interpolates.shape[-2:]))
    return GradientPenaltyFn.apply(plan, x, *plan.params())


class GanStepper(Stepper):
    """One iteration of gans/audio_mnist.py:287-337, hand scheduled (no autograd engine):

        if ctr % d_updates_per_g_update == 0:  z ~ N;  loss_G = BCE(D(G(z)), 1) | -D(G(z)).mean();  Adam(G)
        ctr += 1
        z ~ N;  loss_D = (BCE(D(x), 1) + BCE(D(G(z)), 0)) / 2 | wgan_loss_it(D, x, G(z)).mean();  Adam(D)
        z ~ N;  DG = D(G(z));  DE = D(x)   (sigmoid means in "gan" mode, raw means in "wgan" mode)

    G step    G and D forward, loss kernel, D's data gradients only (no Discriminator weight gradients: the reference
              zeroes them before use), G's parameter gradients straight into its flat Adam group.
    D step    G forward only -- G(z) is a constant of the D step, the reference discards the gradients it lets run
              into G.  "gan": real and fake rows as ONE 2B-row pass, ``ali_bce_logits_pair``.  "wgan": fake, real and
              interpolated rows as ONE 3B-row pass (no batch statistics couple them); backward from
              [1/B, -1/B, 1] keeps every h_l; the first layer's data gradient runs on the interpolated rows only;
              ``ali_gp_penalty``; tangent pass on the interpolated rows; critic weight / bias gradients over the first
              2B rows into the flat gradient, the penalty's weight gradients into a second flat buffer, one add.
    scores    fresh z, forward only, one 2B-row D pass.

    ``step(images, z_g=None, z_d=None, z_s=None, eps=None)`` returns {"loss_G", "loss_D", "DG", "DE"} as 0-d device
    tensors (no host sync); "loss_G" is absent -- and G untouched -- on iterations whose counter is no multiple of
    ``d_updates_per_g_update``.  Draws not given are made on the device from the counter streams keyed by (seed,
    iteration): z_g / z_d / z_s are elements [0, 100B) / [100B, 200B) / [200B, 300B) of
    ``source.normal_reference(seed, iteration, .)``, eps is ``source.uniform_reference(seed, iteration, B)``; torch's
    host generator is left alone.  ``capture=True`` replays the iteration from a HIP graph per input signature, every
    launch on one stream."""

    def __init__(self, G, D, lr=1e-4, betas=(0.5, 0.9), loss_mode="gan", penalty_weight=10.0, d_updates_per_g_update=1,
                 capture=False, eps=1e-8, seed=None, discriminator_weight_decay=0.0):
        if loss_mode not in ("gan", "wgan"):
            raise NotImplementedError(loss_mode)
        if discriminator_weight_decay != 0:
            raise NotImplementedError("GanStepper: discriminator_weight_decay != 0 (ali_adam has no decay term; the "
                                      "reference default is 0)")
        if not (next(G.parameters()).is_cuda and next(D.parameters()).is_cuda):
            raise RuntimeError("GanStepper runs the HIP kernels: G and D must live on a CUDA device (on the CPU use the "
                               "modules under autograd, as gans.audio_mnist.train does)")
        self.G, self.D = G, D
        self.loss_mode, self.penalty_weight = loss_mode, float(penalty_weight)
        self.k = int(d_updates_per_g_update)
        self.seed = _source.DEFAULT_Z_SEED if seed is None else int(seed)
        self.pG, self.pD = get_plan(G.layers), get_plan(D.layers)
        self.opt_g = FlatGroup(list(G.parameters()), lr, betas, eps)
        self.opt_d = FlatGroup(list(D.parameters()), lr, betas, eps)
        dev = self.opt_d.flat.device
        # the penalty's weight gradients (bias segments stay zero): second buffer, added to the critic's
        self.gp_grad = torch.zeros_like(self.opt_d.grad)
        self.gp_views, off = {}, 0
        for p in self.opt_d.params:
            self.gp_views[id(p)] = self.gp_grad[off:off + p.numel()].view(p.shape)
            off += p.numel()
        self.gp_weight_views = {id(st.mod.weight): self.gp_views[id(st.mod.weight)] for st in self.pD.stages}
        self._adopt([(self.opt_g, [self.pG]), (self.opt_d, [self.pD])], capture)
        self.iter_t = torch.zeros(1, dtype=torch.int64, device=dev)     # iterations done: keys the draws
        self.ctr = 0                                                    # host mirror: decides the G step

    # ------------------------------------------------------------------ draws
    def _z(self, given, B, slot, dev):
        if given is not None:
            return g_input(given)
        z = torch.empty(B, LATENT_DIM, dtype=torch.float32, device=dev)
        ops.normal_fill(self.seed, z, dev_counter=self.iter_t, offset=slot * B * LATENT_DIM)
        return g_input(z)

    # ------------------------------------------------------------------ the iteration
    def _g_step(self, B, zin):
        G, D = self.G, self.D
        gen, sG = chain_forward(self.pG, zin, G.training, LATENT_DIM, True)          # [B, H, W, 1]
        logit, sD = chain_forward(self.pD, d_input(gen), D.training, 1, True)
        if self.loss_mode == "gan":
            out, gl = ops.bce_logits(logit.reshape(B), 1.0)
        else:       # -mean D(G(z)): the logits in the critic's "real" slot, out[0] = -mean, gradient -1/B
            out, _, gl = ops.wgan_critic(None, logit.reshape(B), 1.0)
        gx, _ = chain_backward(self.pD, sD, gl.reshape(logit.shape), 1, True, need_params=False, gx_planes=(0,))
        chain_backward(self.pG, sG, _one_plane(gx).reshape(gen.shape), LATENT_DIM, False, True, self.opt_g.grad_views)
        self._update(self.opt_g)
        return out[0]

    def _d_step_gan(self, B, x_real, x_fake):
        X = d_input(torch.cat([x_real, x_fake]).reshape((2 * B,) + self.hw + (1,)))
        logit, sD = chain_forward(self.pD, X, self.D.training, 1, True)
        out3, gl = ops.bce_logits_pair(logit.reshape(2 * B), B, 1.0, 0.0, gscale=0.5)      # (loss_a + loss_b) / 2
        chain_backward(self.pD, sD, gl.reshape(logit.shape), 1, False, True, self.opt_d.grad_views)
        return out3[0]

    def _d_step_wgan(self, B, x_real, x_fake, eps):
        pD, lam = self.pD, self.penalty_weight
        xhat, _ = ops.gp_mix(x_real, x_fake, eps=eps, seed=self.seed, dev_counter=self.iter_t)
        X = d_input(torch.cat([x_fake, x_real, xhat]).reshape((3 * B,) + self.hw + (1,)))
        logit, sD = chain_forward(pD, X, self.D.training, 1, True)
        flat = logit.reshape(3 * B)
        gy = torch.ones(3 * B, dtype=torch.float32, device=flat.device)
        out3, _, _ = ops.wgan_critic(flat[:B], flat[B:2 * B], 1.0, g_fake=gy[:B], g_real=gy[B:2 * B])
        g0, hs = chain_backward_keep(pD, sD, gy.reshape(logit.shape), 1, True, gx_planes=(0,), first_rows=(2 * B, 3 * B))
        g0 = _one_plane(g0).reshape(B, -1)
        out2, v = ops.gp_penalty(g0, lam, out=g0)
        s_hat = saved_rows(sD, 2 * B, 3 * B)
        us = chain_tangent(pD, s_hat, d_input(v.reshape((B,) + self.hw + (1,))))
        chain_param_grads(pD, saved_rows(sD, 0, 2 * B), [h[:2 * B] for h in hs], self.opt_d.grad_views)
        tangent_param_grads(pD, s_hat, us, [h[2 * B:] for h in hs], self.gp_weight_views, head_ones=True)
        self.opt_d.grad.add_(self.gp_grad)
        return out3[0] + lam * out2[0]

    def _scores(self, B, x_real, zin):
        gz, _ = chain_forward(self.pG, zin, self.G.training, LATENT_DIM, False)
        X = d_input(torch.cat([gz.reshape(B, -1), x_real]).reshape((2 * B,) + self.hw + (1,)))
        logit, _ = chain_forward(self.pD, X, self.D.training, 1, False)
        flat = logit.reshape(2 * B)
        if self.loss_mode == "gan":
            out3, _ = ops.bce_logits_pair(flat, B, 0.0, 0.0, want_grad=False)
        else:
            out3, _, _ = ops.wgan_critic(flat[:B], flat[B:], want_grad=False)
        return out3[1], out3[2]

    def _iteration(self, do_g, images, z_g, z_d, z_s, eps):
        B, dev = images.shape[0], images.device
        self.hw = tuple(images.shape[-2:])
        x_real = images.reshape(B, -1).float().contiguous()
        res = {}
        if do_g:
            res["loss_G"] = self._g_step(B, self._z(z_g, B, 0, dev))
        fake, _ = chain_forward(self.pG, self._z(z_d, B, 1, dev), self.G.training, LATENT_DIM, False)
        x_fake = fake.reshape(B, -1)
        if self.loss_mode == "gan":
            res["loss_D"] = self._d_step_gan(B, x_real, x_fake)
        else:
            res["loss_D"] = self._d_step_wgan(B, x_real, x_fake, None if eps is None else eps.reshape(B).float().contiguous())
        self._update(self.opt_d)
        res["DG"], res["DE"] = self._scores(B, x_real, self._z(z_s, B, 2, dev))
        ops.add_i64_multi([self.iter_t], [1])
        return res

    # ------------------------------------------------------------------ capture, state
    @torch.no_grad()
    def step(self, images, z_g=None, z_d=None, z_s=None, eps=None):
        if not images.is_cuda:
            raise ValueError("GanStepper.step: the batch must live on the model's CUDA device")
        do_g = self.ctr % self.k == 0
        self.ctr += 1
        return self._run(lambda *a: self._iteration(do_g, *a), (images, z_g, z_d, z_s, eps),
                         (do_g, self.G.training, self.D.training), [self.iter_t])

    def state_dict(self):
        """Resumable checkpoint: the two module state dicts, both Adam states in ``torch.optim.Adam.state_dict()``
        format, the iteration counter and the seed that key the draws.  Tensors are cloned to the CPU."""
        sd = {f"{n}_state_dict": module_state_cpu(m) for n, m in (("G", self.G), ("D", self.D))}
        sd.update(optimizer_G=self.opt_g.torch_state_dict(), optimizer_D=self.opt_d.torch_state_dict(),
                  iteration=int(self.iter_t.item()), z_seed=self.seed)
        return sd

    def load_state_dict(self, sd):
        """Inverse of ``state_dict``; everything is copied in place, so captured HIP graphs stay valid (a different
        seed is a launch argument: the graphs are dropped)."""
        with torch.no_grad():
            for n, m in (("G", self.G), ("D", self.D)):
                load_module_state_(m, sd[f"{n}_state_dict"])
            self.opt_g.load_torch_state_dict(sd["optimizer_G"])
            self.opt_d.load_torch_state_dict(sd["optimizer_D"])
            self.ctr = int(sd.get("iteration", 0))
            self.iter_t.fill_(self.ctr)
            if int(sd.get("z_seed", self.seed)) != self.seed:
                self.seed = int(sd["z_seed"])
                self._graphs.clear()
            for plan in (self.pG, self.pD):
                plan.cache.refresh()
