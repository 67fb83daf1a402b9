"""Replaying a call from a HIP graph per input signature: the one protocol of every stepper, scorer and sampler.

``GraphCache`` keys a call by the shapes and dtypes of its arguments (``sig``) plus whatever else the caller names; on a
miss the call runs once outside capture on static copies of the arguments (``_Graphed``: packs, workspace, plans), the
state it touched is put back (a warm-up is no training step), and it is recorded; a hit copies the arguments in with one
launch and replays.  ``AliStepper`` records its segmented iteration on ``_Graphed`` directly."""
import gc

import torch

from . import ops


class _Graphed:
    """HIP graphs of one input signature: static copies of the inputs (tensors, dicts of tensors); ``warm`` run on them
    once on a side stream outside capture (packs, workspace, plans), then ``restore`` (a warm-up is no training step);
    one graph per ``capture``, on the current stream, all in one pool.  A call copies inputs in and replays in order."""

    def __init__(self, inputs, warm, restore=None):
        self.inputs = [{k: x.clone() for k, x in v.items()} if isinstance(v, dict) else v.clone() for v in inputs]
        self.graphs, self.out, self._pool = [], None, torch.cuda.graph_pool_handle()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm(*self.inputs)
        torch.cuda.current_stream().wait_stream(side)
        if restore is not None:
            restore()

    def capture(self, fn, *args):
        g = torch.cuda.CUDAGraph()
        # No cyclic garbage collection while the stream captures: a collection that starts inside the capture finalises
        # whatever dead cycles earlier work left behind, and releasing their device memory or graphs is not permitted
        # on a capturing thread (the process aborts).  They go at the next collection after the capture instead.
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, pool=self._pool, capture_error_mode="thread_local"):
                out = fn(*args)
        finally:
            if was_enabled:
                gc.enable()
        self.graphs.append(g)
        return out

    def load(self, inputs):
        ops.copy_multi([p for st, v in zip(self.inputs, inputs)
                        for p in ([(st[k], x) for k, x in v.items()] if isinstance(v, dict) else [(st, v)])])

    def replay(self, n=1):
        """``n`` more runs on the inputs as they stand (a caller whose state lives in the tensors the graph updates)"""
        for _ in range(n):
            for g in self.graphs:
                g.replay()
        return self.out

    def __call__(self, *inputs):
        self.load(inputs)
        return self.replay()


def sig(v):
    """what a graph depends on of one argument: None, a tensor's (shape, dtype), a dict's sorted (key, shape, dtype)"""
    if v is None:
        return None
    if isinstance(v, dict):
        return tuple((k, tuple(x.shape), x.dtype) for k, x in sorted(v.items()))
    return tuple(v.shape), v.dtype


def graph_key(args, extra=()):
    return tuple(sig(a) for a in args), extra


def split_args(args):
    """(the entries of ``args`` that are not None, ``rebuild``): ``rebuild(present)`` is the full list again, None
    back in its places -- a graph holds copies of the arguments given, the call still takes all of them"""
    where = [i for i, a in enumerate(args) if a is not None]

    def rebuild(present):
        full = [None] * len(args)
        for i, a in zip(where, present):
            full[i] = a
        return full
    return [args[i] for i in where], rebuild


class GraphCache:
    """{graph_key: _Graphed} of one callable object.  ``modules`` (inference users): graph replays run no host code,
    and a re-pack after a weight update lands in new buffers, so the graphs recorded for older versions of these
    modules' parameters are dropped (such callers update weights rarely, if ever)."""

    def __init__(self, modules=()):
        self.entries = {}
        self.modules = tuple(modules)
        self._versions = None

    def __len__(self):
        return len(self.entries)

    def __contains__(self, key):
        return key in self.entries

    def clear(self):
        self.entries.clear()

    def sync(self):
        v = tuple(p._version for m in self.modules for p in m.parameters())
        if v != self._versions:
            self.entries.clear()
            self._versions = v

    def __call__(self, fn, args, extra=(), state=(), restored=None):
        """``fn(*args)`` from the graph of ``(args' signatures, extra)``; ``args``: tensors, dicts of tensors or None.
        Recording it first runs ``fn`` once for real: the ``state`` tensors are put back behind that pass, then
        ``restored()`` brings whatever the host derives from them in line.  Returns ``fn``'s result at recording: the
        same tensors on every replay."""
        if self.modules:
            self.sync()
        key = graph_key(args, extra)
        present, rebuild = split_args(args)
        ent = self.entries.get(key)
        if ent is None:
            snap = [t.clone() for t in state]

            def run(*present):
                return fn(*rebuild(present))

            def restore():
                for t, v in zip(state, snap):
                    t.copy_(v)
                if restored is not None:
                    restored()
            ent = _Graphed(present, run, restore)
            ent.out = ent.capture(run, *ent.inputs)
            self.entries[key] = ent
        return ent(*present)

    def replay(self, args, extra=(), n=1):
        """``n`` more runs of the graph ``__call__`` recorded for ``(args' signatures, extra)``, on the inputs it holds"""
        return self.entries[graph_key(args, extra)].replay(n)
