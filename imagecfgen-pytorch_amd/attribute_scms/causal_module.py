"""Causal mechanisms: a distribution p(value | parents) together with its noise -- ``recover_noise`` (abduction) and
``generate`` (prediction) -- on ``torch.distributions`` and the transforms of ``_flows`` (no pyro).

On CUDA tensors ``ConditionalCategoricalCM.recover_noise`` runs the Gumbel posterior in one kernel
(``ali_hip.ops.gumbel_posterior``); on the CPU it is the torch statement below."""
from abc import abstractmethod

import torch
from torch import distributions as dist
from torch.distributions import AffineTransform, ExpTransform, TransformedDistribution

from ._flows import ConditionalTransformedDistribution  # noqa: F401  (the type of ConditionalTransformedCM.ctd)
from .training_utils import dist_parameters, nf_forward, nf_inverse


class CausalModuleBase(torch.nn.Module):
    @abstractmethod
    def noise_distribution(self, *args, **kwargs):
        """p(U)"""
        raise NotImplementedError

    @abstractmethod
    def recover_noise(self, obs, *context, **kwargs):
        """a sample of p(U | obs, context)"""
        raise NotImplementedError

    @abstractmethod
    def condition(self, *context, **kwargs):
        """p(obs | context)"""
        raise NotImplementedError

    @abstractmethod
    def generate(self, noise, *context, **kwargs):
        raise NotImplementedError

    def forward(self, *context, **kwargs):
        return self.condition(*context, **kwargs)


def _each_transform(transforms, name):
    for t in transforms:
        if hasattr(t, name):
            getattr(t, name)()


class TransformedCM(CausalModuleBase):
    def __init__(self, td: TransformedDistribution):
        super().__init__()
        self.td = td

    def eval(self):
        _each_transform(self.td.transforms, "eval")

    def clear_cache(self):
        _each_transform(self.td.transforms, "clear_cache")

    def noise_distribution(self, *args, **kwargs):
        return self.td.base_dist

    def recover_noise(self, obs, *context, **kwargs):
        return nf_inverse(self.td, obs)

    def condition(self, *context, **kwargs):
        return self.td

    def parameters(self, recurse=True):
        return dist_parameters(self.td)

    def generate(self, noise, *context, **kwargs):
        return nf_forward(self.td, noise)


class CategoricalCM(CausalModuleBase):
    """a root category: the value is its own noise"""

    def __init__(self, d: dist.Categorical):
        super().__init__()
        self.d = d

    @property
    def n_categories(self):
        return self.d.probs.size(0)

    def noise_distribution(self, *args, **kwargs):
        return self.d

    def recover_noise(self, obs, *context, **kwargs):
        return obs

    def condition(self, *context, **kwargs):
        return self.d

    def parameters(self, recurse=True):
        return []

    def generate(self, noise, *context, **kwargs):
        return noise


class ConditionalTransformedCM:
    def __init__(self, ctd):
        self.ctd = ctd

    def condition(self, *context) -> TransformedCM:
        return TransformedCM(self.ctd.condition(*context))

    def parameters(self):
        return dist_parameters(self.ctd)

    def clear_cache(self):
        _each_transform(self.ctd.transforms, "clear_cache")

    def eval(self):
        _each_transform(self.ctd.transforms, "eval")


def gumbel_distribution() -> TransformedDistribution:
    """Gumbel(0, 1) as -log(-log U), U uniform on (0, 1)"""
    steps = [ExpTransform().inv, AffineTransform(0, -1), ExpTransform().inv, AffineTransform(0, -1)]
    return TransformedDistribution(dist.Uniform(0, 1), steps)


def gumbel_posterior(logits, y, g):
    """Gumbel-max posterior noise [N, C] for observed classes ``y`` [N] from prior draws ``g`` [N, C]:
    noise_y = g_y + lse(logits) - logit_y;  noise_l = -log(exp(-g_l - logit_l) + exp(-g_y - logit_y)) - logit_l.
    ``argmax(logits + noise) == y``.  lse is max-shifted."""
    y = y.reshape(-1, 1)
    gy, zy = g.gather(1, y), logits.gather(1, y)
    noise = -torch.log(torch.exp(-g - logits) + torch.exp(-gy - zy)) - logits
    return noise.scatter(1, y, gy + torch.logsumexp(logits, dim=-1, keepdim=True) - zy)


class ConditionalCategoricalCM(CausalModuleBase):
    def __init__(self, model: torch.nn.Module, n_categories: int):
        super().__init__()
        self.model = model
        self.gumbel = gumbel_distribution()
        self.n_categories = n_categories

    def noise_distribution(self, *args, **kwargs):
        return self.gumbel

    def recover_noise(self, y, *context, **kwargs):
        logits = self.model(*context)
        y = y.flatten()
        if logits.is_cuda:
            from ali_hip import flow
            return flow.gumbel_posterior(logits.detach(), y)
        g = self.gumbel.sample((y.size(0), self.n_categories)).to(logits)
        return gumbel_posterior(logits, y, g)

    def condition(self, *context, **kwargs):
        return dist.Categorical(logits=self.model(*context))

    def parameters(self, recurse=True):
        return self.model.parameters()

    def generate(self, noise, *context, **kwargs):
        return (self.model(*context) + noise).argmax(dim=1)
