"""A directed acyclic graph of causal mechanisms: joint log-density, ancestral sampling, and counterfactuals as
abduction (``recover_noise``), action (``obs_int``) and prediction (``generate``)."""
from collections import defaultdict
from typing import Dict, Optional

import torch

from .causal_module import CategoricalCM, CausalModuleBase, ConditionalCategoricalCM

_CATEGORICAL = (ConditionalCategoricalCM, CategoricalCM)


class CausalModuleGraph:
    def __init__(self):
        self.modules = {}
        self.adj = defaultdict(set)
        self.adj_rev = defaultdict(set)

    def get_module(self, key: str):
        return self.modules.get(key)

    def add_module(self, key: str, module):
        self.modules[key] = module

    def assert_has_module(self, key):
        assert key in self.modules, "modules must be added with add_module first"

    def add_edge(self, u, v):
        self.assert_has_module(u)
        self.assert_has_module(v)
        self.adj[u].add(v)
        self.adj_rev[v].add(u)

    def remove_edge(self, u, v):
        self.assert_has_module(u)
        self.assert_has_module(v)
        self.adj[u].remove(v)
        self.adj_rev[v].remove(u)

    def parents(self, u):
        self.assert_has_module(u)
        return sorted(self.adj_rev[u])

    def children(self, u):
        self.assert_has_module(u)
        return sorted(self.adj[u])

    def top_sort(self):
        """Kahn's algorithm; among the ready nodes the order is a set's pop order"""
        indeg = {v: len(self.adj_rev[v]) for v in self.modules}
        ready = {v for v, n in indeg.items() if n == 0}
        order = []
        while ready:
            v = ready.pop()
            order.append(v)
            for c in self.children(v):
                indeg[c] -= 1
                if indeg[c] == 0:
                    ready.add(c)
        return order

    def _parent_vals(self, v, values):
        """the values of v's parents as mechanism inputs: categories as one-hot rows on the parents' device (labels are
        encoded; one-hot rows, which ``log_prob`` also accepts for the value itself, pass as they are)"""
        out = []
        for u in self.parents(v):
            if isinstance(self.modules[u], _CATEGORICAL):
                if values[u].ndim > 1 and values[u].is_floating_point():
                    out.append(values[u])
                    continue
                idx = values[u].flatten()
                out.append(torch.eye(self.modules[u].n_categories, device=idx.device)[idx])
            else:
                out.append(values[u])
        return out

    def _bound(self, v, parent_vals):
        """mechanism v under its parents: a CausalModuleBase"""
        m = self.modules[v]
        return m if isinstance(m, CausalModuleBase) else m.condition(*parent_vals)

    def _observed(self, obs):
        return [v for v in self.modules if v in obs and all(u in obs for u in self.parents(v))]

    def recover_noise(self, obs: Dict[str, torch.Tensor]):
        noise = {}
        for v in self._observed(obs):
            pv = self._parent_vals(v, obs)
            noise[v] = self._bound(v, pv).recover_noise(obs[v], *pv)
        return noise

    def log_prob(self, obs: Dict[str, torch.Tensor]):
        lp = {}
        for v in self._observed(obs):
            val = obs[v]
            if isinstance(self.modules[v], _CATEGORICAL) and val.ndim > 1:
                val = val.argmax(1)
            pv = self._parent_vals(v, obs)
            lp[v] = self._bound(v, pv).forward(*pv).log_prob(val)
        return lp

    def _draw(self, v, values, shape):
        pv = self._parent_vals(v, values)
        d = self._bound(v, pv).condition(*pv)
        return d.sample() if isinstance(self.modules[v], ConditionalCategoricalCM) else d.sample(shape)

    def sample(self, obs_in: Optional[Dict[str, torch.Tensor]] = None, n: int = 1) -> Dict[str, torch.Tensor]:
        """ancestral samples; the entries of ``obs_in`` are held constant.  [n] categories, [n, 1] continuous values"""
        if obs_in:
            n = next(iter(obs_in.values())).size(0)
        out = dict(obs_in or {})
        for v in self.top_sort():
            if v not in out:
                out[v] = self._draw(v, out, (n,))
        return out

    def sample_cf(self, obs: Dict[str, torch.Tensor], obs_int: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        obs = dict(obs)
        for v in self.top_sort():                    # what was not observed is drawn under what was
            if v not in obs:
                obs[v] = self._draw(v, obs, ())
        out = dict(obs_int)
        noise = self.recover_noise(obs)
        for v in self.top_sort():
            if v not in out:
                pv = self._parent_vals(v, out)
                out[v] = self._bound(v, pv).generate(noise[v], *pv)
        return out
