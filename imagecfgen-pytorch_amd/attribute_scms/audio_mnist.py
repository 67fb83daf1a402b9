"""The attribute SCM of AudioMNIST: country_of_origin -> native_speaker, (country_of_origin, native_speaker) -> accent;
digit, age and gender on their own.  All attributes are categories given as one-hot rows.

The conditional mechanisms are small MLPs (128 / 64 wide).  On a CUDA device the graph binds them to ``ali_hip.cat``:
``log_prob`` (under autograd), ``sample``, ``sample_differing``, ``recover_noise`` and ``sample_cf`` of native_speaker and
accent are one launch each on fp32 / int64 CUDA tensors (csrc/cat.hip), and ``train`` steps through ``CatStepper``.  The
root categories, partial observations, CPU tensors and graphs whose structure was changed run the torch statement of
``graph.py``.  Device draws come from the counter RNG keyed by ``torch.initial_seed()``, not from ``Categorical.sample``.
``ConditionalCategoricalCM.recover_noise`` on its own is the Gumbel-max posterior, one kernel on CUDA tensors.  ``train``
takes the dict of one-hot tensors; reading the data set's zip needs sklearn and is not part of this package."""
import numpy as np
import torch
from torch import distributions as dist

from .causal_module import *  # noqa: F401,F403  (the reference's module surface)
from .causal_module import CategoricalCM, ConditionalCategoricalCM, gumbel_distribution  # noqa: F401
from .graph import CausalModuleGraph
from .training_utils import batchify

try:
    from tqdm import tqdm
except ImportError:                                        # progress text only
    tqdm = None

VALIDATION_RUNS = np.random.RandomState(42).randint(0, 50, size=(10,)).tolist()


def dense_net(n_in: int, n_hidden: int, n_out: int, n_hidden_layers: int = 0,
              hidden_activation=torch.nn.ReLU()) -> torch.nn.Sequential:
    widths = [n_in] + [n_hidden] * (n_hidden_layers + 1)
    layers = []
    for a, b in zip(widths[:-1], widths[1:]):
        layers += [torch.nn.Linear(a, b), hidden_activation]
    return torch.nn.Sequential(*layers, torch.nn.Linear(n_hidden, n_out))


class ComboNet(torch.nn.Module):
    """``downstream`` over the concatenated features of one network per input.  As in the reference the input
    networks are held in a plain tuple: they are not registered, so ``parameters()`` -- what ``train`` optimises -- and
    ``to()`` reach ``downstream`` alone, and the input networks keep their initial weights."""

    def __init__(self, downstream_model, *models):
        super().__init__()
        self.models = models
        self.downstream = downstream_model

    def forward(self, *inputs):
        return self.downstream(torch.cat([f(x) for f, x in zip(self.models, inputs)], dim=-1))


def categorical_mle(data_train: torch.Tensor, device="cpu"):
    """class frequencies of integer labels; classes up to the largest label seen"""
    counts = torch.bincount(data_train.detach().reshape(-1).cpu().long())
    return CategoricalCM(dist.Categorical(probs=(counts / data_train.size(0)).float().to(device)))


def conditional_categorical_mle(n_categories: int, context_dim: int, n_hidden_layers: int = 2, device: str = "cpu"):
    net = dense_net(context_dim, 128, n_categories, n_hidden_layers=n_hidden_layers).to(device)
    return ConditionalCategoricalCM(net, n_categories)


def conditional_double_categorical_mle(n_categories: int, context_dim1: int, context_dim2: int, device="cpu"):
    nn1 = dense_net(context_dim1, 64, 64, n_hidden_layers=2).to(device)
    nn2 = dense_net(context_dim2, 64, 64, n_hidden_layers=2).to(device)
    downstream = dense_net(128, 64, n_categories, n_hidden_layers=0).to(device)
    return ConditionalCategoricalCM(ComboNet(downstream, nn1, nn2), n_categories)


class AudioMNISTData:
    """The reference reads AudioMNIST's meta data from the zip and one-hot encodes it with sklearn; this package takes
    the encoded tensors (``train(ds)``) instead."""

    def __init__(self, path_to_zip: str, device="cpu"):
        raise ImportError("AudioMNISTData needs sklearn (OneHotEncoder, KBinsDiscretizer) and the data set's zip: "
                          "encode the attributes yourself and hand attribute_scms.audio_mnist.train the one-hot dict")


_TRIO = ("country_of_origin", "native_speaker", "accent")
_COND = _TRIO[1:]


class AudioMNISTCausalGraph(CausalModuleGraph):
    def __init__(self, ds: dict, device: str = "cpu"):
        super().__init__()

        def root(key):
            return categorical_mle(ds[key].argmax(dim=1), device=device)
        n_country, n_native, n_accent = (ds[k].size(1) for k in _TRIO)
        self.add_module("country_of_origin", root("country_of_origin"))
        self.add_module("native_speaker", conditional_categorical_mle(n_native, n_country, device=device))
        self.add_module("accent", conditional_double_categorical_mle(n_accent, n_country, n_native, device=device))
        for key in ("digit", "age", "gender"):
            self.add_module(key, root(key))
        self.add_edge("country_of_origin", "native_speaker")
        self.add_edge("country_of_origin", "accent")
        self.add_edge("native_speaker", "accent")
        self._cat = None
        if torch.device(device).type == "cuda":
            from ali_hip import cat
            self._cat = cat.bind(self)

    def _device_state(self, values):
        """the bound CatState when the kernels apply to these values (CUDA tensors, the structure unchanged)"""
        if self._cat is None:
            return None
        from ali_hip import cat
        return cat.state_of(self, *values)

    def _trio_rows(self, values):
        from ali_hip import cat
        return [cat.rows(values[k], self.modules[k].n_categories) for k in _TRIO]

    def log_prob(self, obs):
        trio = [obs.get(k) for k in _TRIO]
        rows = all(torch.is_tensor(t) and t.dim() == 2 and t.dtype == torch.float32 for t in trio)
        st = self._device_state(trio) if rows else None
        if st is None:
            return super().log_prob(obs)
        from ali_hip import cat
        lp = super().log_prob({k: v for k, v in obs.items() if k not in _COND})
        lp.update(cat.log_prob(st, obs))
        return {v: lp[v] for v in self._observed(obs)}

    def recover_noise(self, obs):
        st = self._device_state([obs[k] for k in _TRIO]) if all(k in obs for k in _TRIO) else None
        if st is None:
            return super().recover_noise(obs)
        from ali_hip import cat
        noise = super().recover_noise({k: v for k, v in obs.items() if k not in _COND})
        noise["native_speaker"], noise["accent"] = cat.recover_noise(st, *self._trio_rows(obs)[:1], obs["native_speaker"],
                                                                     obs["accent"])
        return {v: noise[v] for v in self._observed(obs)}

    def sample(self, obs_in=None, n: int = 1):
        held = dict(obs_in or {})
        st = self._device_state([held[k] for k in _TRIO if k in held])
        if st is None or all(k in held for k in _COND):
            return super().sample(obs_in, n)
        from ali_hip import cat
        if held:
            n = next(iter(held.values())).size(0)
        out = dict(held)
        for v in self.modules:                                # the root categories keep the statement's code
            if v not in out and v not in _COND:
                out[v] = self._draw(v, out, (n,))
        country = cat.rows(out["country_of_origin"], self.modules["country_of_origin"].n_categories)
        drawn = cat.sample(st, country, held.get("native_speaker"), held.get("accent"))
        for k, v in zip(_COND, drawn):
            out.setdefault(k, v)
        return out

    def sample_differing(self, obs_in, key, forbidden, max_tries: int = 64):
        """An ancestral sample in which ``key`` differs from ``forbidden`` [n] (labels or one-hot rows): per row,
        ``key`` is redrawn under its parents until it differs, at most ``max_tries`` draws, and each row keeps its first
        differing draw -- what the counterfactual-score scripts' whole-batch redraw loop gives per row.  What ``obs_in``
        holds stays; ancestors of ``key`` that are not held are drawn once, descendants under the kept value.  Returns
        (values: the dict ``sample`` returns, status [n] int32: 1 where no draw differed -- ``values[key]`` is then the
        last draw).  On CUDA tensors with ``max_tries`` = 64 it is one launch and no host read."""
        held = {k: v for k, v in (obs_in or {}).items() if k != key}
        forb = forbidden.argmax(1) if forbidden.dim() > 1 else forbidden.reshape(-1)
        n = forb.size(0)
        st = None
        if key in _COND and max_tries == 64 and forb.is_cuda:
            st = self._device_state([held[k] for k in _TRIO if k in held] + [forb.to(torch.int64)])
        if st is not None:
            from ali_hip import cat
            out = dict(held)
            for v in self.modules:
                if v not in out and v not in _COND:
                    out[v] = self._draw(v, out, (n,))
            country = cat.rows(out["country_of_origin"], self.modules["country_of_origin"].n_categories)
            native, accent, status = cat.sample_differing(st, country, key, forb, held.get("native_speaker"),
                                                          held.get("accent"))
            out.setdefault("native_speaker", native)
            out.setdefault("accent", accent)
            return out, status
        out, status = dict(held), None
        for v in self.top_sort():                             # the statement: parents before children
            if v in out:
                continue
            vals = self._draw(v, out, (n,))
            if v == key:
                pending, tries = vals == forb, 1
                while tries < max_tries and pending.any():
                    vals = torch.where(pending, self._draw(v, out, (n,)), vals)
                    pending, tries = vals == forb, tries + 1
                status = pending.to(torch.int32)
            out[v] = vals
        return out, status

    def sample_cf(self, obs, obs_int):
        full = all(k in obs for k in self.modules)
        values = [obs[k] for k in _TRIO] + [obs_int[k] for k in _TRIO if k in obs_int] if full else []
        st = self._device_state(values) if full else None
        if st is None:
            return super().sample_cf(obs, obs_int)
        from ali_hip import cat
        country, _, _ = self._trio_rows(obs)
        country_cf = None
        if "country_of_origin" in obs_int:
            country_cf = cat.rows(obs_int["country_of_origin"], self.modules["country_of_origin"].n_categories)
        native, accent = cat.sample_cf(st, country, obs["native_speaker"], obs["accent"], country_cf=country_cf,
                                       native_cf=obs_int.get("native_speaker"), accent_cf=obs_int.get("accent"))
        out = dict(obs_int)
        for k in self.modules:                                # a root's noise is its value
            if k not in out:
                out[k] = native if k == "native_speaker" else accent if k == "accent" else obs[k]
        return out


def train(ds: dict, steps=2000, device="cpu", lr=1e-2, batch_size=10_000):
    """``ds``: {attribute: one-hot rows [N, n]} (the reference reads them from the zip's path).  Adam on the negative
    log-likelihood of native_speaker and accent given their parents, batches of 10 000 shuffled rows; the epoch means
    are left in ``graph.train_losses``.  On a CUDA device a step is ``ali_hip.cat.CatStepper``'s: the epoch's
    permutation is uploaded once and passed as the kernels' row index, and the host reads one number per epoch."""
    ds = {k: v.float().to(device) for k, v in ds.items() if k != "audio"}
    graph = AudioMNISTCausalGraph(ds, device=device)
    keys = ("country_of_origin", "native_speaker", "accent", "age")
    graph.train_losses = []
    epochs = tqdm(range(steps)) if tqdm is not None else range(steps)
    n_rows = ds[keys[0]].size(0)
    if graph._cat is not None:
        from ali_hip.cat import CatStepper
        stepper = CatStepper(graph, lr=lr)
        tables = [ds[k].contiguous() for k in _TRIO]
        for _ in epochs:
            idx = torch.from_numpy(np.random.permutation(n_rows)).to(device)
            epoch_loss, n_batches = torch.zeros((), device=device), 0
            for s in range(0, n_rows, batch_size):
                epoch_loss += stepper.step(*tables, index=idx[s:s + batch_size])["loss"]
                n_batches += 1
            graph.train_losses.append(epoch_loss.item() / n_batches)
            if tqdm is not None:
                epochs.set_description(f"loss = {round(graph.train_losses[-1], 4)}")
        return graph
    params = [p for k in ("native_speaker", "accent") for p in graph.get_module(k).parameters()]
    optimizer = torch.optim.Adam(params, lr=lr)
    for _ in epochs:
        idx = torch.from_numpy(np.random.permutation(n_rows)).to(device)
        batches = list(batchify(*(ds[k][idx] for k in keys), batch_size=batch_size))
        epoch_loss = torch.zeros((), device=device)
        for batch in batches:
            optimizer.zero_grad()
            lp = graph.log_prob(dict(zip(keys, batch)))
            loss = -(lp["native_speaker"] + lp["accent"]).mean()
            loss.backward()
            optimizer.step()
            epoch_loss += loss.detach()
        graph.train_losses.append(epoch_loss.item() / len(batches))
        if tqdm is not None:
            epochs.set_description(f"loss = {round(graph.train_losses[-1], 4)}")
    return graph
