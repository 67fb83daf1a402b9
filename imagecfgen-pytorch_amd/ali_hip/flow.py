"""The device path of ``attribute_scms``: the MorphoMNIST attribute SCM on the kernels of csrc/flow.hip.

``bind(graph)`` moves the trainable state of an ``MNISTCausalGraph`` into ONE flat fp32 buffer -- theta [75] in the
layout of include/ali_hip.h, then BatchNorm's moving mean and variance -- and makes the modules' parameters and buffers
views of it, so that one ``ops.adam`` call steps everything and a kernel reads what the modules hold.

  FlowLogProb    ``graph.log_prob`` under autograd: one launch forward, one backward (the incoming gradient is the
                 kernel's ``wgt``); in training mode one more for the batch statistics
  FlowStepper    a whole training step in three launches (statistics, densities + gradient, Adam), replayed from a HIP
                 graph per batch size
  sample / recover_noise / sample_cf    through ``ops.flow_map``: one launch for any number of rows

The graph must have the reference's structure (``FlowState.matches``); anything else runs the torch statement."""
import torch

from . import ops
from .graphs import GraphCache

NAMES = ("thickness", "intensity", "slant")
_ADAM_EPS = 1e-8


class FlowState:
    def __init__(self, graph):
        self.bn = graph.get_module("thickness").td.transforms[0]
        self.caa = graph.get_module("intensity").ctd.transforms[0]
        self.spline = graph.get_module("slant").td.transforms[0]
        lin1, lin2 = self.caa.nn[0], self.caa.nn[2]
        self.params = [self.bn.gamma, self.bn.beta, lin1.weight, lin1.bias, lin2.weight, lin2.bias,
                       self.spline.unnormalized_widths, self.spline.unnormalized_heights,
                       self.spline.unnormalized_derivatives, self.spline.unnormalized_lambdas]
        dev = self.params[0].device
        self.flat = torch.empty(ops.FLOW_THETA + 2, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in self.params:
                n = p.numel()
                self.flat[off:off + n].copy_(p.reshape(-1))
                p.data = self.flat[off:off + n].view(p.shape)
                off += n
            assert off == ops.FLOW_THETA
            for name in ("moving_mean", "moving_variance"):
                self.flat[off:off + 1].copy_(self.bn._buffers[name])
                self.bn._buffers[name] = self.flat[off:off + 1]
                off += 1
        self.theta, self.moving = self.flat[:ops.FLOW_THETA], self.flat[ops.FLOW_THETA:]
        self.cst = graph.consts.to(device=dev, dtype=torch.float32).contiguous()
        self.transforms = tuple(tuple(graph.get_module(k).td.transforms if k != "intensity"
                                      else graph.get_module(k).ctd.transforms) for k in NAMES)

    def matches(self, graph):
        """whether ``graph`` still is what was bound: the four modules, the one edge, the same transforms, and
        parameters that still live in the flat buffer"""
        if set(graph.modules) != set(NAMES) | {"digit"}:
            return False
        if {(u, v) for u, vs in graph.adj.items() for v in vs} != {("thickness", "intensity")}:
            return False
        for k, was in zip(NAMES, self.transforms):
            m = graph.get_module(k)
            now = getattr(m, "ctd", None) or getattr(m, "td", None)
            if now is None or len(now.transforms) != len(was) or any(a is not b for a, b in zip(now.transforms, was)):
                return False
        off, base = 0, self.flat.data_ptr()
        for p in self.params:
            if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                return False
            off += p.numel()
        return (self.bn.moving_mean.data_ptr() == base + 4 * off
                and self.bn.moving_variance.data_ptr() == base + 4 * off + 4)

    def density_stats(self, t, out=None):
        """the statistics BatchNorm's density direction uses for thickness column ``t``: in training the batch's (the
        moving buffers move, as the statement's do), otherwise the moving buffers"""
        if self.bn.training:
            return ops.flow_stats(t, moving=self.moving, momentum=self.bn.momentum, out=out)
        return self.moving


def bind(graph):
    return FlowState(graph)


def state_of(graph, *tensors):
    """the graph's FlowState when the device path applies to these tensors, else None (-> the statement)"""
    st = getattr(graph, "_flow", None)
    if st is None or not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return None
    return st if st.matches(graph) else None


class FlowLogProb(torch.autograd.Function):
    """lp [N, 3] of (t, i, s); the gradient reaches the ten parameter tensors behind theta"""

    @staticmethod
    def forward(ctx, state, t, i, s, stats, *params):
        lp, _, _ = ops.flow_nll(t, i, s, state.theta, state.cst, stats, want_lp=True, want_out4=False)
        ctx.state = state
        ctx.save_for_backward(t, i, s, stats)
        return lp

    @staticmethod
    def backward(ctx, g):
        st = ctx.state
        t, i, s, stats = ctx.saved_tensors
        _, _, gth = ops.flow_nll(t, i, s, st.theta, st.cst, stats, wgt=g.contiguous(), want_lp=False, want_out4=False,
                                 want_grad=True)
        grads, off = [], 0
        for p in st.params:
            grads.append(gth[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return (None,) * 5 + tuple(grads)


def log_prob(st, obs):
    t, i, s = (obs[k] for k in NAMES)
    lp = FlowLogProb.apply(st, t, i, s, st.density_stats(t), *st.params)
    return {k: lp[:, j:j + 1] for j, k in enumerate(NAMES)}


class FlowStepper:
    """One Adam step on -mean(lp_thickness + lp_intensity + lp_slant) per ``step(t, i, s)``: statistics -> densities
    and gradient -> Adam, three launches, replayed from a HIP graph per batch size (``capture``).  Returns device
    scalars {"loss", "lp_thickness", "lp_intensity", "lp_slant"}: views of one buffer that the next step overwrites."""

    def __init__(self, graph, lr=1e-2, betas=(0.9, 0.999), capture=True):
        st = getattr(graph, "_flow", None)
        if st is None or not st.matches(graph):
            raise ValueError("FlowStepper: needs an MNISTCausalGraph of the reference's structure on a CUDA device")
        self.state, self.lr, self.betas, self.capture = st, float(lr), (float(betas[0]), float(betas[1])), capture
        dev = st.flat.device
        self.m = torch.zeros(ops.FLOW_THETA, dtype=torch.float32, device=dev)
        self.v = torch.zeros_like(self.m)
        self.g = torch.zeros_like(self.m)
        self.stats = torch.zeros(2, dtype=torch.float32, device=dev)
        self.dev_step = torch.zeros(1, dtype=torch.int32, device=dev)      # completed steps
        self.arrive = torch.zeros(1, dtype=torch.int32, device=dev)
        self.graphs = GraphCache()

    def _run(self, t, i, s):
        st = self.state
        stats = st.density_stats(t, out=self.stats)
        _, out4, _ = ops.flow_nll(t, i, s, st.theta, st.cst, stats, gscale=-1.0, want_lp=False, gtheta=self.g)
        ops.adam(st.theta, self.g, self.m, self.v, self.lr, self.betas[0], self.betas[1], _ADAM_EPS, 0,
                 dev_step=self.dev_step, arrive=self.arrive)
        return out4

    def step(self, t, i, s):
        t, i, s = (x.reshape(-1).contiguous() for x in (t, i, s))
        if self.capture:
            out4 = self.graphs(self._run, [t, i, s], extra=(bool(self.state.bn.training),),
                               state=(self.state.flat, self.m, self.v, self.dev_step))
        else:
            out4 = self._run(t, i, s)
        return {"loss": out4[0], "lp_thickness": out4[1], "lp_intensity": out4[2], "lp_slant": out4[3]}


def _rows(cols, n, dev):
    """[n, 3] rows from {column index: [n] / [n, 1] tensor}; columns not given are zero"""
    rows = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    for j, c in cols.items():
        rows[:, j] = c.reshape(-1)
    return rows


def sample(st, held, n):
    """ancestral samples of the three attributes, [n, 1] each; ``held`` {name: values} stay as they are"""
    dev = st.flat.device
    rows = torch.randn(n, 3, dtype=torch.float32, device=dev)
    modes = [ops.FLOW_FORWARD] * 3
    for j, k in enumerate(NAMES):
        if k in held:
            rows[:, j] = held[k].reshape(-1)
            modes[j] = ops.FLOW_SKIP
    out, _ = ops.flow_map(rows, st.theta, st.cst, st.moving, st.moving, modes=modes, out=rows)
    return {k: held[k] if k in held else out[:, j:j + 1] for j, k in enumerate(NAMES)}


def recover_noise(st, obs):
    """{name: noise [N, 1]} of the observed attributes whose parents are observed too"""
    have = [k for k in NAMES if k in obs and (k != "intensity" or "thickness" in obs)]
    if not have:
        return {}
    n = obs[have[0]].shape[0]
    rows = _rows({j: obs[k] for j, k in enumerate(NAMES) if k in obs}, n, st.flat.device)
    modes = [ops.FLOW_INVERSE if k in have else ops.FLOW_SKIP for k in NAMES]
    stats = st.density_stats(obs["thickness"]) if "thickness" in have else st.moving
    out, _ = ops.flow_map(rows, st.theta, st.cst, stats, st.moving, modes=modes)
    return {k: out[:, j:j + 1] for j, k in enumerate(NAMES) if k in have}


def sample_cf(st, obs, obs_int):
    """abduction, action, prediction of fully observed rows in one launch: {name: [N, 1]}"""
    n = obs["thickness"].shape[0]
    dev = st.flat.device
    rows = _rows({j: obs[k] for j, k in enumerate(NAMES)}, n, dev)
    mask = sum(1 << j for j, k in enumerate(NAMES) if k in obs_int)
    val = _rows({j: obs_int[k] for j, k in enumerate(NAMES) if k in obs_int}, n, dev) if mask else None
    out, _ = ops.flow_map(rows, st.theta, st.cst, st.density_stats(obs["thickness"]), st.moving, cf_mask=mask, val=val)
    return {k: obs_int[k] if k in obs_int else out[:, j:j + 1] for j, k in enumerate(NAMES)}


_GUMBEL = {"offset": 0}


def gumbel_posterior(logits, y):
    """``ops.gumbel_posterior`` with draws of its own: the stream is keyed by torch's seed and advances per call"""
    logits = logits.float().contiguous()
    n = logits.numel()
    noise, _ = ops.gumbel_posterior(logits, y.reshape(-1).to(torch.int64).contiguous(), seed=torch.initial_seed(),
                                    offset=_GUMBEL["offset"])
    _GUMBEL["offset"] += n
    return noise
