"""The stepper protocol of ``ali_hip.trainer`` on stub groups and plans (what is called, in which order, and what a
warm-up pass leaves behind) and the two module-state loops of the checkpoints: no GPU needed."""
import torch
import torch.nn as nn

import ali_hip.step
import ali_hip.trainer
from ali_hip.trainer import Stepper, load_module_state_, module_state_cpu


class _Cache:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def make_static(self):
        self.log.append(("make_static", self.name))

    def refresh(self):
        self.log.append(("refresh", self.name))


class _Plan:
    def __init__(self, name, log):
        self.cache = _Cache(name, log)


class _Group:
    """what a Stepper asks of a FlatGroup: adam, state_tensors, resync"""

    def __init__(self, name, log, value):
        self.name, self.log = name, log
        self.tensors = [torch.full((3,), float(value)), torch.full((1,), int(value), dtype=torch.int32)]

    def adam(self):
        self.log.append(("adam", self.name))

    def state_tensors(self):
        return self.tensors

    def resync(self):
        self.log.append(("resync", self.name))


class _MissingGraph:
    """``GraphCache.__call__`` on a miss, minus the capture: snapshot ``state``, run ``fn`` once, put the snapshot back,
    call ``restored()``"""

    def __init__(self):
        self.calls = []

    def __call__(self, fn, args, extra=(), state=(), restored=None):
        self.calls.append((fn, args, extra, list(state)))
        snap = [t.clone() for t in state]
        out = fn(*args)
        for t, v in zip(state, snap):
            t.copy_(v)
        restored()
        return out


def _stepper(capture):
    log = []
    g0, g1 = _Group("g0", log, 1), _Group("g1", log, 2)
    plans = {n: _Plan(n, log) for n in ("a", "b", "c")}
    s = Stepper()
    s._adopt([(g0, [plans["a"], plans["b"]]), (g1, [plans["c"]])], capture)
    return s, log, g0, g1


def test_adopt_makes_every_plan_static_once_in_listed_order():
    s, log, _, _ = _stepper(True)
    assert log == [("make_static", "a"), ("make_static", "b"), ("make_static", "c")]
    assert s.capture is True and isinstance(s._graphs, ali_hip.trainer.GraphCache) and len(s._graphs) == 0
    assert _stepper(False)[0].capture is False


def test_update_is_adam_then_the_refresh_of_that_groups_plans_only():
    s, log, g0, g1 = _stepper(False)
    del log[:]
    s._update(g0)
    assert log == [("adam", "g0"), ("refresh", "a"), ("refresh", "b")]
    del log[:]
    s._update(g1)
    assert log == [("adam", "g1"), ("refresh", "c")]


def test_run_without_capture_calls_fn_and_never_the_graphs():
    s, log, _, _ = _stepper(False)

    def no_graphs(*a, **k):
        raise AssertionError("_graphs was called with capture off")
    s._graphs = no_graphs
    del log[:]
    assert s._run(lambda a, b: (a, b), (1, 2), (True,), [torch.zeros(1)]) == (1, 2)
    assert log == []


def test_run_with_capture_hands_over_the_state_and_a_warm_up_is_no_step():
    s, log, g0, g1 = _stepper(True)
    fake = s._graphs = _MissingGraph()
    extra = torch.full((1,), 5, dtype=torch.int64)
    del log[:]

    def fn(x):
        g0.tensors[0].add_(1.0)                    # what a step does to its state: all of it must come back
        g1.tensors[1].add_(1)
        extra.add_(1)
        s._update(g1)
        return x * 2

    x = torch.ones(2)
    out = s._run(fn, (x,), ("modes",), [extra])
    assert torch.equal(out, x * 2)
    (got_fn, got_args, got_extra, state), = fake.calls
    assert got_fn is fn and got_args == (x,) and got_extra == ("modes",)
    want = g0.tensors + g1.tensors + [extra]
    assert len(state) == len(want) and all(a is b for a, b in zip(state, want))
    # the step's own launches, then the put-back's: group by group, the count first, then that group's packs
    assert log == [("adam", "g1"), ("refresh", "c"),
                   ("resync", "g0"), ("refresh", "a"), ("refresh", "b"), ("resync", "g1"), ("refresh", "c")]
    assert torch.equal(g0.tensors[0], torch.full((3,), 1.0)) and int(g0.tensors[1]) == 1
    assert torch.equal(g1.tensors[0], torch.full((3,), 2.0)) and int(g1.tensors[1]) == 2
    assert int(extra) == 5


def test_run_without_extra_state_hands_over_the_groups_alone():
    s, _, g0, g1 = _stepper(True)
    fake = s._graphs = _MissingGraph()
    s._run(lambda: None, (), ())
    state = fake.calls[0][3]
    assert [t.data_ptr() for t in state] == [t.data_ptr() for t in g0.tensors + g1.tensors]


def _model(seed):
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Conv2d(1, 2, 3), nn.BatchNorm2d(2))
    m.train()
    m(torch.randn(4, 1, 5, 5))                     # running statistics and num_batches_tracked move off their defaults
    return m


def test_module_state_round_trip_is_exact_and_in_place():
    src, dst = _model(0), _model(1)
    sd = module_state_cpu(src)
    assert set(sd) == set(src.state_dict()) and "1.running_var" in sd and "1.num_batches_tracked" in sd
    for k, v in src.state_dict().items():
        assert sd[k].device.type == "cpu" and sd[k].data_ptr() != v.data_ptr() and not sd[k].requires_grad
    assert any(not torch.equal(v, sd[k]) for k, v in dst.state_dict().items())
    ptrs = [p.data_ptr() for p in dst.parameters()] + [b.data_ptr() for b in dst.buffers()]
    with torch.no_grad():
        src[0].weight.add_(1.0)                    # a clone: what was saved does not follow its source
    load_module_state_(dst, sd)
    assert [p.data_ptr() for p in dst.parameters()] + [b.data_ptr() for b in dst.buffers()] == ptrs
    assert all(p.requires_grad for p in dst.parameters())
    for k, v in dst.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    assert not torch.equal(dst[0].weight, src[0].weight)


def test_flat_group_is_one_class_under_both_import_paths():
    assert ali_hip.step.FlatGroup is ali_hip.trainer.FlatGroup
    assert ali_hip.trainer.FlatGroup.__module__ == "ali_hip.trainer"
