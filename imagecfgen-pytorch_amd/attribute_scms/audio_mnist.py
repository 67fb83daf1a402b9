"""The attribute SCM of AudioMNIST: country_of_origin -> native_speaker, (country_of_origin, native_speaker) -> accent;
digit, age and gender on their own.  All attributes are categories given as one-hot rows.

The conditional mechanisms are small MLPs (128 / 64 wide) that stay on torch and rocBLAS; their counterfactual noise is
the Gumbel-max posterior, one kernel on CUDA tensors (``ConditionalCategoricalCM.recover_noise``).  ``train`` takes the
dict of one-hot tensors; reading the data set's zip needs sklearn and is not part of this package."""
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


class AudioMNISTCausalGraph(CausalModuleGraph):
    def __init__(self, ds: dict, device: str = "cpu"):
        super().__init__()

        def root(key):
            return categorical_mle(ds[key].argmax(dim=1), device=device)
        n_country, n_native, n_accent = (ds[k].size(1) for k in ("country_of_origin", "native_speaker", "accent"))
        self.add_module("country_of_origin", root("country_of_origin"))
        self.add_module("native_speaker", conditional_categorical_mle(n_native, n_country, device=device))
        self.add_module("accent", conditional_double_categorical_mle(n_accent, n_country, n_native, device=device))
        for key in ("digit", "age", "gender"):
            self.add_module(key, root(key))
        self.add_edge("country_of_origin", "native_speaker")
        self.add_edge("country_of_origin", "accent")
        self.add_edge("native_speaker", "accent")


def train(ds: dict, steps=2000, device="cpu", lr=1e-2):
    """``ds``: {attribute: one-hot rows [N, n]} (the reference reads them from the zip's path).  Adam on the negative
    log-likelihood of native_speaker and accent given their parents, batches of 10 000 shuffled rows; the epoch means
    are left in ``graph.train_losses``."""
    ds = {k: v.float().to(device) for k, v in ds.items() if k != "audio"}
    graph = AudioMNISTCausalGraph(ds, device=device)
    params = [p for k in ("native_speaker", "accent") for p in graph.get_module(k).parameters()]
    optimizer = torch.optim.Adam(params, lr=lr)
    keys = ("country_of_origin", "native_speaker", "accent", "age")
    graph.train_losses = []
    epochs = tqdm(range(steps)) if tqdm is not None else range(steps)
    for _ in epochs:
        idx = torch.from_numpy(np.random.permutation(ds[keys[0]].size(0))).to(device)
        batches = list(batchify(*(ds[k][idx] for k in keys), batch_size=10_000))
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
