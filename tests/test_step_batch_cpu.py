"""``ali_hip.step._Batch``: the value AliStepper threads through an iteration, and the three things a graph replay
derives from it -- what it loads (``tensors``), the batch on the graphs' static copies (``rebind``) and the batch's part
of the graph key (``graph_key``).  The expected tuples are written out by hand for the four input modes: host batch with
``z``, host batch with ``z=None`` (drawn on the device), host batch with an announced next batch, indexed batch."""
import types

import torch

from ali_hip.step import _Batch

B = 3


def _host(seed=0):
    g = torch.Generator().manual_seed(seed)
    images, z = torch.randn(B, 1, 4, 4, generator=g), torch.randn(B, 8, 1, 1, generator=g)
    return images, {"digit": torch.randn(B, 10, generator=g)}, z


def _clones(ts):
    return tuple({k: v.clone() for k, v in t.items()} if isinstance(t, dict) else t.clone() for t in ts)


def _same(got, want):
    assert len(got) == len(want)
    assert all(g is w for g, w in zip(got, want))


def test_host_batch_with_z():
    im, c, z = _host()
    b = _Batch.host(im, c, z)
    assert (b.images, b.c, b.z, b.ahead, b.source, b.index) == (im, c, z, None, None, None)
    _same(b.tensors(), (im, c, z))
    assert b.graph_key() == ((B, 1, 4, 4), False)
    st = _clones(b.tensors())
    r = b.rebind(st)
    _same((r.images, r.c, r.z), st)
    assert r.ahead is None and r.source is None and r.index is None
    assert b.identity() == (im.data_ptr(), (B, 1, 4, 4), z.data_ptr(), (B, 8, 1, 1))


def test_host_batch_device_drawn_z():
    im, c, _ = _host()
    b = _Batch.host(im, c)
    _same(b.tensors(), (im, c))
    assert b.graph_key() == ((B, 1, 4, 4), False, "z")
    st = _clones(b.tensors())
    r = b.rebind(list(st))                  # (_Graphed keeps its static inputs in a list)
    _same((r.images, r.c), st)
    assert r.z is None and r.ahead is None and r.source is None and r.index is None


def test_host_batch_with_ahead():
    im, c, z = _host()
    im2, c2, z2 = _host(1)
    b = _Batch.host(im, c, z, ahead=(im2, c2, z2))
    assert isinstance(b.ahead, _Batch) and b.ahead.ahead is None
    _same(b.tensors(), (im, c, z, im2, c2, z2))
    assert b.graph_key() == ((B, 1, 4, 4), True)
    st = _clones(b.tensors())
    r = b.rebind(st)
    _same((r.images, r.c, r.z, r.ahead.images, r.ahead.c, r.ahead.z), st)
    assert isinstance(r.ahead, _Batch) and r.ahead.ahead is None and r.source is None
    assert b.ahead.identity() == (im2.data_ptr(), (B, 1, 4, 4), z2.data_ptr(), (B, 8, 1, 1))
    # the public tuple may also come as a list; dropping the announcement gives the plain batch's key and tensors
    plain = _Batch.host(im, c, z, ahead=[im2, c2, z2])._replace(ahead=None)
    _same(plain.tensors(), (im, c, z))
    assert plain.graph_key() == ((B, 1, 4, 4), False)


def test_indexed_batch():
    source = types.SimpleNamespace(key=("mnist", 60000))
    index = torch.arange(5, dtype=torch.int64)
    b = _Batch.indexed(source, index)
    assert (b.images, b.c, b.z, b.ahead) == (None, None, None, None) and b.source is source and b.index is index
    _same(b.tensors(), (index,))
    assert b.graph_key() == ((("mnist", 60000), 5), False, "indexed")
    st = _clones(b.tensors())
    r = b.rebind(st)
    assert r.index is st[0] and r.source is source
    assert (r.images, r.c, r.z, r.ahead) == (None, None, None, None)


def test_graph_keys_tell_the_modes_apart_and_ignore_addresses():
    im, c, z = _host()
    source = types.SimpleNamespace(key=("mnist", 60000))
    modes = [_Batch.host(im, c, z), _Batch.host(im, c), _Batch.host(im, c, z, ahead=_host(1)),
             _Batch.indexed(source, torch.arange(B, dtype=torch.int64))]
    assert len({b.graph_key() for b in modes}) == 4
    im2, c2, z2 = _host(2)
    assert im2.data_ptr() != im.data_ptr()
    again = [_Batch.host(im2, c2, z2), _Batch.host(im2, c2), _Batch.host(im2, c2, z2, ahead=_host(3)),
             _Batch.indexed(source, torch.arange(B, 2 * B, dtype=torch.int64))]
    assert [b.graph_key() for b in again] == [b.graph_key() for b in modes]
    assert again[0].identity() != modes[0].identity()
    # another batch size is another graph
    assert _Batch.host(im[:2], c, z[:2]).graph_key() != modes[0].graph_key()
    assert _Batch.indexed(source, torch.arange(2, dtype=torch.int64)).graph_key() != modes[3].graph_key()


def test_replay_key_is_the_schedule_around_the_batch_part():
    """AliStepper._replay's complete key: ("seg" | "one", <where>, do_eg, pipe, <ahead announced>[, "z" | "indexed"]) --
    the batch's part goes around (do_eg, pipe) exactly like this."""
    im, c, z = _host()
    source = types.SimpleNamespace(key="k")

    def full(b, mode="seg", do_eg=True, pipe=False):
        where, *rest = b.graph_key()
        return (mode, where, do_eg, pipe, *rest)

    assert full(_Batch.host(im, c, z), "one") == ("one", (B, 1, 4, 4), True, False, False)
    assert full(_Batch.host(im, c), "one", do_eg=False) == ("one", (B, 1, 4, 4), False, False, False, "z")
    assert full(_Batch.host(im, c, z, ahead=(im, c, z)), pipe=True) == ("seg", (B, 1, 4, 4), True, True, True)
    assert full(_Batch.indexed(source, torch.arange(4))) == ("seg", ("k", 4), True, False, False, "indexed")
