"""The attribute SCM of MorphoMNIST: thickness -> intensity, slant and digit on their own.

  thickness  Normal -> BatchNorm(1) -> exp
  intensity  Normal -> affine flow conditioned on the raw thickness -> sigmoid -> affine to [i_min, i_max]
  slant      Normal -> rational-linear spline -> affine to [s_min, s_max]
  digit      the training set's class frequencies

On a CUDA device the trainable state lives in one flat buffer (``ali_hip.flow.bind``) and ``log_prob``, ``sample``,
``recover_noise``, ``sample_cf`` and ``train`` run the kernels of csrc/flow.hip; CPU tensors, other dtypes and a graph
whose structure was changed run the torch statement of ``graph.py`` / ``_flows.py``."""
import numpy as np
import torch
from torch import distributions as dist
from torch.distributions import AffineTransform, ExpTransform, TransformedDistribution

from ._flows import BatchNorm, ConditionalTransformedDistribution, Sigmoid32, Spline, conditional_affine_autoregressive
from .causal_module import CategoricalCM, ConditionalTransformedCM, TransformedCM
from .graph import CausalModuleGraph
from .training_utils import batchify

try:
    from tqdm import tqdm
except ImportError:                                        # progress text only
    tqdm = None

_CONTINUOUS = ("thickness", "intensity", "slant")


class MNISTCausalGraph(CausalModuleGraph):
    def __init__(self, a_train: torch.Tensor, intensity_idx=11, slant_idx=12, device="cpu"):
        super().__init__()
        intensity, slant = a_train[:, intensity_idx], a_train[:, slant_idx]
        i_min, s_min = intensity.min(), slant.min()
        consts = torch.stack([i_min, intensity.max() - i_min, s_min, slant.max() - s_min])
        _, counts = torch.unique(a_train[:, :10].argmax(dim=1), return_counts=True)
        self._build(consts, counts / a_train.size(0), device)

    def _build(self, consts, label_probs, device, dtype=None, bind=True):
        """``consts`` = [i_min, i_max - i_min, s_min, s_max - s_min]; ``dtype``: of the parameters (None: fp32);
        ``bind``: whether a CUDA fp32 graph takes the device path"""
        consts = consts.detach().to(device=device, dtype=dtype or consts.dtype)
        self.consts = consts

        def base():
            return dist.Normal(torch.zeros(1, device=device, dtype=dtype), torch.ones(1, device=device, dtype=dtype))

        def placed(module):
            return module.to(device=device, dtype=dtype)
        t_dist = TransformedDistribution(base(), [placed(BatchNorm(1)), ExpTransform()])
        i_dist = ConditionalTransformedDistribution(base(), [placed(conditional_affine_autoregressive(1, 1)),
                                                             Sigmoid32(), AffineTransform(consts[0], consts[1])])
        s_dist = TransformedDistribution(base(), [placed(Spline(1)), AffineTransform(consts[2], consts[3])])
        label_dist = dist.Categorical(probs=label_probs.to(device=device, dtype=dtype or torch.float32))
        self.add_module("thickness", TransformedCM(t_dist))
        self.add_module("intensity", ConditionalTransformedCM(i_dist))
        self.add_module("slant", TransformedCM(s_dist))
        self.add_module("digit", CategoricalCM(label_dist))
        self.add_edge("thickness", "intensity")
        self._flow = None
        if bind and torch.device(device).type == "cuda" and dtype in (None, torch.float32):
            from ali_hip import flow
            self._flow = flow.bind(self)

    def trainable(self):
        """the transforms that hold the trainable state: BatchNorm, the conditional affine flow, the spline"""
        return (self.get_module("thickness").td.transforms[0], self.get_module("intensity").ctd.transforms[0],
                self.get_module("slant").td.transforms[0])

    def statement(self, dtype=torch.float64, device="cpu"):
        """a copy of this graph that runs the torch statement in ``dtype`` on ``device``: the same constants,
        parameters, buffers and training flags"""
        twin = MNISTCausalGraph.__new__(MNISTCausalGraph)
        CausalModuleGraph.__init__(twin)
        twin._build(self.consts, self.get_module("digit").d.probs, device, dtype, bind=False)
        for mine, theirs in zip(self.trainable(), twin.trainable()):
            theirs.load_state_dict({k: v.detach().to(device=device, dtype=dtype) for k, v in mine.state_dict().items()})
            theirs.training = mine.training
        return twin

    def _device_state(self, values):
        if self._flow is None:
            return None
        from ali_hip import flow
        return flow.state_of(self, *values)

    def log_prob(self, obs):
        st = self._device_state([obs[k] for k in _CONTINUOUS]) if all(k in obs for k in _CONTINUOUS) else None
        if st is None:
            return super().log_prob(obs)
        from ali_hip import flow
        lp = flow.log_prob(st, obs)
        if "digit" in obs:
            lp.update(super().log_prob({"digit": obs["digit"]}))
        return lp

    def recover_noise(self, obs):
        cont = {k: obs[k] for k in _CONTINUOUS if k in obs}
        st = self._device_state(list(cont.values())) if cont else None
        if st is None:
            return super().recover_noise(obs)
        from ali_hip import flow
        noise = flow.recover_noise(st, cont)
        if "digit" in obs:
            noise["digit"] = obs["digit"]
        return {k: noise[k] for k in self.modules if k in noise}

    def sample(self, obs_in=None, n=1):
        held = {k: v for k, v in (obs_in or {}).items() if k in _CONTINUOUS}
        st = self._device_state(list(held.values()))
        if st is None:
            return super().sample(obs_in, n)
        from ali_hip import flow
        if obs_in:
            n = next(iter(obs_in.values())).size(0)
        out = dict(obs_in or {})
        drawn = flow.sample(st, held, n)
        for v in self.top_sort():                       # (the reference's key order)
            if v not in out:
                out[v] = drawn[v] if v in drawn else self.get_module(v).d.sample((n,))
        return out

    def sample_cf(self, obs, obs_int):
        full = all(k in obs for k in _CONTINUOUS)
        st = self._device_state([obs[k] for k in _CONTINUOUS] + [v for k, v in obs_int.items() if k in _CONTINUOUS]) \
            if full else None
        if st is None:
            return super().sample_cf(obs, obs_int)
        from ali_hip import flow
        digit = obs["digit"] if "digit" in obs else self.get_module("digit").d.sample()
        out = dict(obs_int)
        cf = flow.sample_cf(st, obs, obs_int)
        for v in self.top_sort():
            if v not in out:
                out[v] = cf[v] if v in cf else digit
        return out


def train(a_train: torch.Tensor, steps=2000, thickness_idx=10, intensity_idx=11, slant_idx=12, device="cpu"):
    """``steps`` epochs of Adam(lr = 1e-2) on the negative joint log-density of the three continuous attributes, in
    batches of 10 000 shuffled rows.  On a CUDA device a step is ``ali_hip.flow.FlowStepper``'s three launches from a
    HIP graph, and the host reads one number per epoch (the progress text).  The epoch means are left in
    ``graph.train_losses``."""
    graph = MNISTCausalGraph(a_train, intensity_idx=intensity_idx, slant_idx=slant_idx, device=device)
    a_train = a_train.to(device=device, dtype=torch.float32)
    cols = [a_train[:, j:j + 1] for j in (thickness_idx, intensity_idx, slant_idx)]
    stepper = optimizer = None
    if graph._flow is not None:
        from ali_hip.flow import FlowStepper
        stepper = FlowStepper(graph, lr=1e-2)
    else:
        params = [p for name in _CONTINUOUS for p in graph.get_module(name).parameters()]
        optimizer = torch.optim.Adam(params, lr=1e-2)

    graph.train_losses = []
    epochs = tqdm(range(steps)) if tqdm is not None else range(steps)
    for _ in epochs:
        idx = torch.from_numpy(np.random.permutation(a_train.size(0))).to(a_train.device)
        batches = list(batchify(*(c[idx] for c in cols), batch_size=10_000))
        epoch_loss = torch.zeros((), device=a_train.device)
        for t, i, s in batches:
            if stepper is not None:
                epoch_loss += stepper.step(t, i, s)["loss"]
                continue
            optimizer.zero_grad()
            lp = graph.log_prob({"thickness": t, "intensity": i, "slant": s})
            loss = -(lp["thickness"] + lp["intensity"] + lp["slant"]).mean()
            loss.backward()
            optimizer.step()
            for name in _CONTINUOUS:
                graph.get_module(name).clear_cache()
            epoch_loss += loss.detach()
        graph.train_losses.append(epoch_loss.item() / len(batches))            # the one host read of the epoch
        if tqdm is not None:
            epochs.set_description(f"loss = {round(graph.train_losses[-1], 4)}")
    return graph
