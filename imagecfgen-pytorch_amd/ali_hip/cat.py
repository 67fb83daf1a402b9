"""The device path of ``attribute_scms.audio_mnist``: the AudioMNIST attribute SCM on the kernels of csrc/cat.hip.

``bind(graph)`` moves the twelve trained tensors of an ``AudioMNISTCausalGraph`` -- native_speaker's four Linear layers
and the accent net's downstream two -- into ONE flat fp32 buffer in the layout of include/ali_hip.h, and the accent
net's two frozen towers into a second one; the modules' parameters become views, so ``parameters()``, ``state_dict()``
and a torch optimiser keep working, one ``ops.adam`` call steps everything and a kernel reads what the modules hold.

  CatLogProb    ``graph.log_prob`` of native_speaker and accent under autograd: one launch forward, two backward (data
                gradients, then the weight gradients; the incoming gradient is the kernel's ``wgt``)
  CatStepper    a whole training step in three launches (densities + data gradients, weight gradients, Adam), replayed
                from a HIP graph per batch size
  sample / sample_differing / recover_noise / sample_cf    one ``ops.cat_map`` launch each for any number of rows, no host
                read; draws come from the counter RNG keyed by ``torch.initial_seed()`` at an offset that advances per call

The graph must have the reference's structure (``CatState.matches``); anything else runs the torch statement."""
import torch

from . import ops
from .graphs import GraphCache

NODES = ("native_speaker", "accent")
ROOTS = ("country_of_origin", "digit", "age", "gender")
EDGES = {("country_of_origin", "native_speaker"), ("country_of_origin", "accent"), ("native_speaker", "accent")}
_ADAM_EPS = 1e-8
_H, _T = 128, 64


def _mlp(net, widths):
    """the Linear layers of ``net`` when it is Linear(w0, w1) ReLU ... Linear(w[-2], w[-1]), else None"""
    mods = list(net) if isinstance(net, torch.nn.Sequential) else None
    if mods is None or len(mods) != 2 * (len(widths) - 1) - 1:
        return None
    lins = mods[0::2]
    if not all(isinstance(m, torch.nn.ReLU) for m in mods[1::2]):
        return None
    for m, a, b in zip(lins, widths[:-1], widths[1:]):
        if not (isinstance(m, torch.nn.Linear) and m.in_features == a and m.out_features == b and m.bias is not None):
            return None
    return lins


def _layers(graph):
    """(trained Linear layers [6], tower Linear layers [8], (Cc, Cn, Ca)) of a graph of the reference's structure,
    else None"""
    if set(graph.modules) != set(NODES) | set(ROOTS):
        return None
    if {(u, v) for u, vs in graph.adj.items() for v in vs} != EDGES:
        return None
    ns, ac, co = (graph.get_module(k) for k in ("native_speaker", "accent", "country_of_origin"))
    combo = getattr(ac, "model", None)
    if not (hasattr(ns, "model") and hasattr(combo, "downstream") and len(getattr(combo, "models", ())) == 2
            and hasattr(co, "d")):
        return None
    Cc, Cn, Ca = co.n_categories, ns.n_categories, ac.n_categories
    if not all(1 <= c <= 64 for c in (Cc, Cn, Ca)):
        return None
    nat = _mlp(ns.model, [Cc, _H, _H, _H, Cn])
    down = _mlp(combo.downstream, [2 * _T, _T, Ca])
    tc, tn = _mlp(combo.models[0], [Cc, _T, _T, _T, _T]), _mlp(combo.models[1], [Cn, _T, _T, _T, _T])
    if None in (nat, down, tc, tn):
        return None
    return nat + down, tc + tn, (Cc, Cn, Ca)


def _flatten(lins, n, dev):
    """the weights and biases of ``lins`` as views of one new flat buffer of ``n`` floats"""
    flat = torch.empty(n, dtype=torch.float32, device=dev)
    params, off = [], 0
    with torch.no_grad():
        for m in lins:
            for p in (m.weight, m.bias):
                k = p.numel()
                flat[off:off + k].copy_(p.reshape(-1))
                p.data = flat[off:off + k].view(p.shape)
                params.append(p)
                off += k
    assert off == n, (off, n)
    return flat, params


def _inside(params, flat):
    off, base = 0, flat.data_ptr()
    for p in params:
        if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
            return False
        off += p.numel()
    return True


class CatState:
    def __init__(self, graph):
        found = _layers(graph)
        if found is None:
            raise ValueError("cat.bind: needs an AudioMNISTCausalGraph of the reference's structure")
        self.trained, self.frozen, self.sizes = found
        dev = self.trained[0].weight.device
        if dev.type != "cuda" or self.trained[0].weight.dtype != torch.float32:
            raise ValueError("cat.bind: needs fp32 parameters on a CUDA device")
        nth, ntw = ops.cat_sizes(*self.sizes)
        self.theta, self.params = _flatten(self.trained, nth, dev)
        self.towers, self.tower_params = _flatten([m.to(dev) for m in self.frozen], ntw, dev)
        self.mods = tuple(graph.get_module(k) for k in NODES + ROOTS)
        self.offset = 0                                   # of the next draw in the Gumbel stream

    def matches(self, graph):
        """whether ``graph`` still is what was bound: the six modules, the three edges, the layers (by identity, with
        their shapes and activations), and parameters that still live in the two flat buffers"""
        found = _layers(graph)
        if found is None or found[2] != self.sizes:
            return False
        if any(graph.get_module(k) is not m for k, m in zip(NODES + ROOTS, self.mods)):
            return False
        if any(a is not b for a, b in zip(found[0] + found[1], self.trained + self.frozen)):
            return False
        now = [p for m in self.trained for p in (m.weight, m.bias)]
        tow = [p for m in self.frozen for p in (m.weight, m.bias)]
        return (all(a is b for a, b in zip(now, self.params)) and all(a is b for a, b in zip(tow, self.tower_params))
                and _inside(now, self.theta) and _inside(tow, self.towers))

    def take(self, n):
        """the stream offset of a call that uses ``n`` elements; the next call starts behind them"""
        off = self.offset
        self.offset += int(n)
        return off


def bind(graph):
    return CatState(graph)


def state_of(graph, *tensors):
    """the graph's CatState when the device path applies to these tensors (CUDA, fp32 or int64), else None (-> the
    statement)"""
    st = getattr(graph, "_cat", None)
    if st is None or not all(torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.float32, torch.int64) for t in tensors):
        return None
    return st if st.matches(graph) else None


class CatLogProb(torch.autograd.Function):
    """lp [N, 2] of (native_speaker, accent) given their parents; the gradient reaches the twelve trained tensors"""

    @staticmethod
    def forward(ctx, state, country, native, accent, *params):
        lp, _, _ = ops.cat_nll(state.theta, state.towers, country, native, accent, want_out3=False)
        ctx.state = state
        ctx.save_for_backward(country, native, accent)
        return lp

    @staticmethod
    def backward(ctx, g):
        st = ctx.state
        country, native, accent = ctx.saved_tensors
        _, _, gth = ops.cat_nll(st.theta, st.towers, country, native, accent, wgt=g.contiguous(), want_lp=False,
                                want_out3=False, want_grad=True)
        grads, off = [], 0
        for p in st.params:
            grads.append(gth[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return (None,) * 4 + tuple(grads)


def log_prob(st, obs):
    """{native_speaker: [N], accent: [N]} for one-hot / dense fp32 rows of the three attributes"""
    lp = CatLogProb.apply(st, obs["country_of_origin"], obs["native_speaker"], obs["accent"], *st.params)
    return {"native_speaker": lp[:, 0], "accent": lp[:, 1]}


class CatStepper:
    """One Adam step on -mean(lp_native_speaker + lp_accent) per ``step(country, native, accent, index=None)``:
    densities and data gradients -> weight gradients -> Adam, three launches, replayed from a HIP graph per batch size
    (``capture``; the replay's input copy is the fourth).  ``index`` (int64 [n]): the batch is rows ``index`` of the
    three tables.  Returns device scalars {"loss", "lp_native_speaker", "lp_accent"}: views of one buffer that the next
    step overwrites."""

    def __init__(self, graph, lr=1e-2, betas=(0.9, 0.999), capture=True):
        st = getattr(graph, "_cat", None)
        if st is None or not st.matches(graph):
            raise ValueError("CatStepper: needs an AudioMNISTCausalGraph of the reference's structure on a CUDA device")
        self.state, self.lr, self.betas, self.capture = st, float(lr), (float(betas[0]), float(betas[1])), capture
        self.m = torch.zeros_like(st.theta)
        self.v = torch.zeros_like(st.theta)
        self.g = torch.zeros_like(st.theta)
        self.dev_step = torch.zeros(1, dtype=torch.int32, device=st.theta.device)      # completed steps
        self.arrive = torch.zeros(1, dtype=torch.int32, device=st.theta.device)
        self.graphs = GraphCache()

    def _run(self, country, native, accent, index):
        st = self.state
        _, out3, _ = ops.cat_nll(st.theta, st.towers, country, native, accent, index=index, gscale=-1.0, want_lp=False,
                                 gtheta=self.g)
        ops.adam(st.theta, self.g, self.m, self.v, self.lr, self.betas[0], self.betas[1], _ADAM_EPS, 0,
                 dev_step=self.dev_step, arrive=self.arrive)
        return out3

    def step(self, country, native, accent, index=None):
        args = [x.contiguous() for x in (country, native, accent)] + [None if index is None else index.contiguous()]
        if self.capture:
            out3 = self.graphs(self._run, args, state=(self.state.theta, self.m, self.v, self.dev_step))
        else:
            out3 = self._run(*args)
        return {"loss": out3[0], "lp_native_speaker": out3[1], "lp_accent": out3[2]}


def labels(x):
    """[N] int64 classes of labels or one-hot / probability rows (their first maximum)"""
    return (x.argmax(1) if x.dim() > 1 else x.reshape(-1)).to(torch.int64).contiguous()


def rows(x, C):
    """fp32 rows [N, C] of one-hot / dense rows (as they are) or of labels (one-hot)"""
    if x.dim() > 1 and x.is_floating_point():
        return x.float()
    return torch.eye(C, dtype=torch.float32, device=x.device)[x.reshape(-1)]


def _opt_labels(x):
    return None if x is None else labels(x)


def sample(st, country, native=None, accent=None):
    """ancestral draw of (native_speaker, accent) [N] int64 under ``country`` rows; a node given is held"""
    _, Cn, Ca = st.sizes
    y = (_opt_labels(native), _opt_labels(accent))
    r = ops.cat_map(ops.CAT_SAMPLE, st.theta, st.towers, country, Cn, Ca, y=y, seed=torch.initial_seed(),
                    offset=st.take(country.shape[0] * (Cn + Ca)))
    return tuple(y[j] if y[j] is not None else r["out"][j] for j in range(2))


def sample_differing(st, country, key, forbidden, native=None, accent=None):
    """like ``sample``, but node ``key`` is redrawn per row (up to ``ops.CAT_TRIES`` times) until it differs from
    ``forbidden`` [N].  Returns (native_speaker, accent, status int32 [N]: 1 where no try differed)."""
    _, Cn, Ca = st.sizes
    node = NODES.index(key)
    y = [_opt_labels(native), _opt_labels(accent)]
    y[node] = None
    v = [None, None]
    v[node] = labels(forbidden)
    n = country.shape[0]
    r = ops.cat_map(ops.CAT_DIFFER, st.theta, st.towers, country, Cn, Ca, y=y, v=v, node=node, seed=torch.initial_seed(),
                    offset=st.take(n * (ops.CAT_TRIES * (Ca if node else Cn) + Cn + Ca)))
    return tuple(y[j] if y[j] is not None else r["out"][j] for j in range(2)) + (r["status"],)


def recover_noise(st, country, native, accent):
    """the Gumbel posterior noise ([N, Cn], [N, Ca]) of the observed classes under their observed parents"""
    _, Cn, Ca = st.sizes
    r = ops.cat_map(ops.CAT_ABDUCT, st.theta, st.towers, country, Cn, Ca, y=(labels(native), labels(accent)),
                    seed=torch.initial_seed(), offset=st.take(country.shape[0] * (Cn + Ca)))
    return r["noise"][:, :Cn], r["noise"][:, Cn:]


def sample_cf(st, country, native, accent, country_cf=None, native_cf=None, accent_cf=None):
    """abduction, action, prediction in one launch: the counterfactual (native_speaker, accent) [N] int64 of observed
    rows under ``country_cf`` (None: as observed) with the nodes given as ``*_cf`` set to those values"""
    _, Cn, Ca = st.sizes
    v = (_opt_labels(native_cf), _opt_labels(accent_cf))
    r = ops.cat_map(ops.CAT_CF, st.theta, st.towers, country, Cn, Ca, country_cf=country_cf,
                    y=(labels(native), labels(accent)), v=v, cf_mask=sum(1 << j for j in range(2) if v[j] is not None),
                    seed=torch.initial_seed(), offset=st.take(country.shape[0] * (Cn + Ca)))
    return r["out"]
