"""The flat Adam group of every family (``FlatGroup``), the protocol around a hand-scheduled training step (``Stepper``)
and the two module-state loops of the checkpoints."""
import torch

from . import ops
from .graphs import GraphCache


class FlatGroup:
    """Parameters re-pointed into one flat buffer + flat grad / exp_avg / exp_avg_sq buffers.

    ``layouts`` (optional, {id(param): strides}): the element order a parameter takes inside its segment of the flat
    buffers -- a dense permutation given as the strides of the (logically unchanged) parameter tensor.  The stepper
    asks for the forward GEMM's weight layout (`[K][R*S][C]`: torch's channels_last for a Conv2d weight), so that the
    optimiser step itself leaves the weights in kernel layout and half of the re-pack disappears; Adam is elementwise
    and does not care.  Gradients, exp_avg and exp_avg_sq use the same order (``*_views``)."""

    def __init__(self, params, lr, betas, eps, layouts=None, twin16=False):
        """``twin16``: keep an fp16 twin of the whole flat parameter buffer, written by the Adam launch itself (fp16-MFMA
        path: a conv weight whose segment is laid out as the forward GEMM's pack needs no re-pack launch at all -- the
        fp32 segment IS the pack and ``flat16``'s segment its twin)."""
        self.params = list(params)
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.n = n
        self.flat = torch.empty(n, device=dev)
        self.flat16 = torch.empty(n, dtype=torch.float16, device=dev) if twin16 else None
        self.grad = torch.zeros(n, device=dev)
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        self.grad_views, self.m_views, self.v_views = {}, [], []
        layouts = layouts or {}
        off = 0
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                st = layouts.get(id(p))

                def view(buf):
                    seg = buf[off:off + k]
                    return seg.view(p.shape) if st is None else torch.as_strided(seg, p.shape, st)
                w = view(self.flat)
                w.copy_(p.detach())
                p.data = w
                if self.flat16 is not None:      # the segment's twin, found by chain.packed through the parameter
                    p._ali_flat16 = self.flat16[off:off + k]
                gv = view(self.grad)
                p.grad = gv
                self.grad_views[id(p)] = gv
                self.m_views.append(view(self.m))
                self.v_views.append(view(self.v))
                off += k
        self.sync16()
        self.lr, self.betas, self.eps = lr, betas, eps
        self.steps = 0
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)   # device-side count of completed steps (graph replays)
        self.arrive = torch.zeros(1, dtype=torch.int32, device=dev) if dev.type == "cuda" else None

    def sync16(self):
        """re-round the fp16 twin after the parameters were changed by anything but ``adam`` (load_state, restore)"""
        if self.flat16 is not None:
            self.flat16.copy_(self.flat)

    def state_tensors(self):
        """what a pass that must not count (a graph's warm-up) clones and puts back; then ``resync``"""
        return [self.flat, self.m, self.v, self.step_t]

    def resync(self):
        """the state tensors were rewritten on the device: the host's step count and the fp16 twin follow"""
        self.steps = int(self.step_t.item())
        self.sync16()

    @staticmethod
    def logical(views):
        """the buffer behind ``views`` as one flat tensor in the parameters' own (row-major) element order"""
        return torch.cat([v.reshape(-1) for v in views])

    def grad_logical(self):
        """the flat gradient in the parameters' own element order (tests, diagnostics)"""
        return self.logical(list(self.grad_views.values()))

    def load_logical(self, views, flat):
        off = 0
        for v in views:
            v.copy_(flat[off:off + v.numel()].view(v.shape))
            off += v.numel()

    def adam(self, grad_scale=1.0):
        self.steps += 1
        # the kernel runs step step_t + 1 and its last block advances step_t: no launch for the counter
        ops.adam(self.flat, self.grad, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps, self.steps,
                 dev_step=self.step_t, grad_scale=grad_scale, arrive=self.arrive, p16=self.flat16)

    # torch.optim-like surface for callers that keep the returned optimisers
    def zero_grad(self):
        self.grad.zero_()

    def step(self):
        self.adam()

    def state_dict(self):
        # the device-side count is the authoritative one: HIP-graph replays do not run the host-side increment
        self.steps = int(self.step_t.item())
        return {"step": self.steps, "exp_avg": self.logical(self.m_views), "exp_avg_sq": self.logical(self.v_views),
                "lr": self.lr, "betas": self.betas, "eps": self.eps}

    def torch_state_dict(self):
        """this group as a ``torch.optim.Adam.state_dict()`` (per-parameter moments in the parameters' own layout, CPU
        clones): ``torch.optim.Adam(params, ...).load_state_dict(...)`` takes it"""
        step = int(self.step_t.item())
        proto = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=tuple(self.betas), eps=self.eps).state_dict()
        pg = dict(proto["param_groups"][0], params=list(range(len(self.params))))
        state = {i: {"step": torch.tensor(float(step)), "exp_avg": m.detach().cpu().clone().contiguous(),
                     "exp_avg_sq": v.detach().cpu().clone().contiguous()}
                 for i, (m, v) in enumerate(zip(self.m_views, self.v_views))}
        return {"state": state, "param_groups": [pg]}

    def load_torch_state_dict(self, sd):
        """inverse of ``torch_state_dict`` (also takes the state dict of a ``torch.optim.Adam`` over the same parameters;
        parameters without state get zero moments); in place, so captured graphs stay valid"""
        with torch.no_grad():
            steps = 0
            for i, (m, v) in enumerate(zip(self.m_views, self.v_views)):
                st = sd["state"].get(i)
                if st is None:
                    m.zero_(), v.zero_()
                    continue
                m.copy_(st["exp_avg"].to(m.device))
                v.copy_(st["exp_avg_sq"].to(v.device))
                steps = int(st["step"])
            self.steps = steps
            self.step_t.fill_(steps)


class Stepper:
    """What surrounds the schedule of a stepper whose parameters live in ``FlatGroup``s: static packs, the
    re-pack behind every Adam launch, graph replay with a warm-up pass that is no step.  The order of the groups, and of
    the plans inside a group, is the order of the launches: a captured graph and the bitwise tests depend on it."""

    def _adopt(self, groups, capture):
        """``groups``: [(FlatGroup, the plans whose packs its Adam launch invalidates), ...]; the packs get fixed addresses"""
        self._groups = {g: tuple(plans) for g, plans in groups}
        for plans in self._groups.values():
            for plan in plans:
                plan.cache.make_static()
        self.capture = capture
        self._graphs = GraphCache()

    def _update(self, group):
        """the end of a step on ``group``: its Adam launch, then the re-pack of the weights it changed"""
        group.adam()
        for plan in self._groups[group]:
            plan.cache.refresh()

    def _restored(self):
        """the state tensors were rewritten on the device: the host's step counts, the fp16 twins and the packs follow"""
        for group, plans in self._groups.items():
            group.resync()
            for plan in plans:
                plan.cache.refresh()

    def _run(self, fn, args, modes, extra_state=()):
        """``fn(*args)``: eagerly, or (``capture``) from the HIP graph of the arguments' signature and ``modes``.  The
        pass that records a graph is no step: every group's state and ``extra_state`` are put back behind it."""
        if not self.capture:
            return fn(*args)
        state = [t for g in self._groups for t in g.state_tensors()] + list(extra_state)
        return self._graphs(fn, args, modes, state, self._restored)


def module_state_cpu(module):
    """a module's state dict as CPU clones (checkpoints)"""
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def load_module_state_(module, src):
    """copy the state dict ``src`` into ``module`` in place: addresses stay, so captured graphs stay valid"""
    with torch.no_grad():
        for k, v in module.state_dict().items():
            v.copy_(src[k])
