"""The host side of ``ali_hip.graphs`` (keys, optional arguments, the version watch) and ``FlatGroup``'s
``torch.optim.Adam`` state dicts: no GPU needed."""
import copy

import pytest
import torch
import torch.nn as nn

from ali_hip.graphs import GraphCache, graph_key, sig, split_args
from ali_hip.step import FlatGroup


def test_sig_of_a_tensor_a_dict_and_none():
    x = torch.zeros(2, 3, dtype=torch.float16)
    assert sig(None) is None
    assert sig(x) == ((2, 3), torch.float16)
    d = {"b": torch.zeros(4, 1), "a": torch.zeros(4, 10, dtype=torch.int32)}
    assert sig(d) == (("a", (4, 10), torch.int32), ("b", (4, 1), torch.float32))


def test_key_ignores_insertion_order_and_sees_shape_and_dtype():
    x, a, b = torch.zeros(4, 1, 28, 28), torch.zeros(4, 10), torch.zeros(4, 1)
    key = graph_key([x, {"a": a, "b": b}, None], (True,))
    assert key == graph_key([x.clone(), {"b": b, "a": a}, None], (True,))
    assert hash(key) == hash(graph_key([x, {"b": b, "a": a}, None], (True,)))
    for other in (graph_key([x[:3], {"a": a, "b": b}, None], (True,)),                 # a shape
                  graph_key([x.double(), {"a": a, "b": b}, None], (True,)),            # a dtype
                  graph_key([x, {"a": a, "b": b.int()}, None], (True,)),               # a dtype inside the dict
                  graph_key([x, {"a": a, "b": b[:, :0]}, None], (True,)),              # a shape inside the dict
                  graph_key([x, {"a": a}, None], (True,)),                             # a key less
                  graph_key([x, {"a": a, "b": b}, b], (True,)),                        # an optional argument given
                  graph_key([x, {"a": a, "b": b}, None], (False,))):                   # what the caller adds
        assert other != key


@pytest.mark.parametrize("holes", [(0,), (1,), (3,), (0, 3), (0, 1, 2, 3), ()])
def test_split_and_rebuild_round_trip_with_none_anywhere(holes):
    args = [torch.full((1,), float(i)) for i in range(3)] + [{"k": torch.ones(2)}]
    for i in holes:
        args[i] = None
    present, rebuild = split_args(args)
    assert len(present) == 4 - len(holes) and all(p is not None for p in present)
    full = rebuild(present)
    assert len(full) == 4 and all(f is a for f, a in zip(full, args))
    stand_ins = [object() for _ in present]                   # (a graph calls it with its own copies)
    again = rebuild(stand_ins)
    assert [f for f in again if f is not None] == stand_ins and [i for i, f in enumerate(again) if f is None] == list(holes)


def test_version_watch_clears_on_a_write_not_on_a_read():
    m, other = nn.Linear(3, 2), nn.Linear(3, 2)
    cache = GraphCache(modules=[m])
    cache.sync()
    cache.entries["k"] = "a recorded graph"
    cache.sync()
    m(torch.zeros(1, 3)), m.weight.sum(), m.weight.detach().clone()
    with torch.no_grad():
        other.weight.mul_(2.0)                                # not watched
    cache.sync()
    assert len(cache) == 1 and "k" in cache
    with torch.no_grad():
        m.bias.mul_(1.0)
    cache.sync()
    assert len(cache) == 0 and "k" not in cache
    cache.entries["k"] = "recorded again"
    cache.sync()
    assert len(cache) == 1
    cache.clear()
    assert len(cache) == 0


def _group():
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 2))
    group = FlatGroup(list(model.parameters()), 1e-3, (0.5, 0.9), 1e-7)
    g = torch.Generator().manual_seed(1)
    group.m.copy_(torch.randn(group.n, generator=g))
    group.v.copy_(torch.rand(group.n, generator=g))
    group.step_t.fill_(7)
    return model, group


def test_flat_group_state_dict_is_an_adam_state_dict():
    model, group = _group()
    assert [t.data_ptr() for t in group.state_tensors()] == [t.data_ptr() for t in (group.flat, group.m, group.v,
                                                                                    group.step_t)]
    sd = group.torch_state_dict()
    opt = torch.optim.Adam(model.parameters(), lr=1.0)
    opt.load_state_dict(copy.deepcopy(sd))
    pg = opt.param_groups[0]
    assert (pg["lr"], tuple(pg["betas"]), pg["eps"]) == (1e-3, (0.5, 0.9), 1e-7)
    for p, mv, vv in zip(model.parameters(), group.m_views, group.v_views):
        st = opt.state[p]
        assert float(st["step"]) == 7.0 and torch.equal(st["exp_avg"], mv) and torch.equal(st["exp_avg_sq"], vv)
    m0, v0 = group.m.clone(), group.v.clone()
    group.m.zero_(), group.v.fill_(3.0), group.step_t.fill_(0)
    group.load_torch_state_dict(opt.state_dict())
    assert torch.equal(group.m, m0) and torch.equal(group.v, v0)
    assert int(group.step_t.item()) == 7 and group.steps == 7


def test_a_parameter_without_adam_state_gets_zero_moments():
    model, group = _group()
    sd = group.torch_state_dict()
    del sd["state"][1]                                        # the first layer's bias
    m0, v0 = [t.clone() for t in group.m_views], [t.clone() for t in group.v_views]
    group.load_torch_state_dict(sd)
    for i, (mv, vv) in enumerate(zip(group.m_views, group.v_views)):
        if i == 1:
            assert not mv.any() and not vv.any()
        else:
            assert torch.equal(mv, m0[i]) and torch.equal(vv, v0[i])
    assert int(group.step_t.item()) == 7


def test_resync_reads_the_step_count_from_the_device_counter():
    _, group = _group()
    assert group.steps == 0
    group.resync()
    assert group.steps == 7
