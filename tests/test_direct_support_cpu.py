"""``chain.route`` may not promise a direct one-channel kernel that the launch refuses.

The routes "tconv1" (a stride-1 ``ConvTranspose2d(C -> 1)``), "first_direct" (weight gradient of a stride-1 first
``Conv2d``) and planes "direct" (its consumed-plane data gradient) end in ``ali_tconv1_fwd`` / ``ali_tconv1_dgrad`` /
``ali_tconv1_wgrad``.  Those refuse shapes of their own -- a rectangular kernel on the forward, R * S outside
{1, 4, 9, 16, 25} on the data gradient, more taps than ``ceil(T / (256 / K)) <= 7`` accumulators hold on the weight
gradient, R or S above 5 -- and a refusal in the middle of a backward pass is a ``RuntimeError`` where the GEMM route
of the stage's kind would have served.  The sweep below walks every (kind, channels, R, S, pad, c_log) of the domain,
asks ``route`` and holds every direct answer against ``ops.tconv1_route``, the launches' own plan.  No GPU: the models
live on the meta device, the query is host arithmetic."""
import itertools

import pytest
import torch
import torch.nn as nn

CHANNELS = (32, 64, 128, 256)
SIDES = range(1, 8)
PADS = range(0, 3)
B, H, W = 4, 9, 11          # R, S <= 7 leave an output map of at least 3 x 5 at every pad


def _stage(seq):
    from ali_hip import chain
    plan = chain.ChainPlan(seq)
    assert len(plan.stages) == 1
    return plan.stages[0]


def launches(st, rt, in_shape, c_log):
    """[(label, op, args, kwargs)]: every ali_tconv1_* launch the stage's Route ``rt`` stands for, as chain.py issues
    them (``_stage_forward``, ``_param_grads``, ``_plane_grads``, ``_data_grad``)"""
    m = st.mod
    (R, S), pad = m.kernel_size, m.padding[0]
    Bn, Hn, Wn, Cp = in_shape
    out = []
    if st.kind == "convT":      # the many-channel map is the layer's input
        big = (Bn, Hn, Wn, Cp, R, S, pad)
        if rt.fwd == "tconv1":
            out.append(("tconv1 fwd", "fwd", big, {}))
        if "tconv1" in (rt.wgrad[0], rt.wgrad_fold[0]):
            out.append(("tconv1 wgrad", "wgrad", big, {"nc": 1}))
        if rt.dgrad == "tconv1":
            out.append(("tconv1 dgrad", "dgrad", big, {}))
    else:                       # the many-channel map is the gradient of the layer's output
        big = (Bn, Hn + 2 * pad - R + 1, Wn + 2 * pad - S + 1, m.out_channels, R, S, pad)
        if "first_direct" in (rt.wgrad[0], rt.wgrad_fold[0]):
            out.append(("first_direct wgrad", "wgrad", big, {"nc": c_log}))
        if rt.planes == "direct":
            out.append(("planes direct", "fwd", big, {}))
    return out


def _sweep():
    """yields (point, stage, route, in_shape, c_log) over the whole domain"""
    from ali_hip import chain
    for ch, R, S, pad in itertools.product(CHANNELS, SIDES, SIDES, PADS):
        with torch.device("meta"):
            tail = nn.Sequential(nn.ConvTranspose2d(ch, 1, (R, S), padding=pad), nn.Tanh())
            first = nn.Sequential(nn.Conv2d(8, ch, (R, S), padding=pad), nn.LeakyReLU(0.2))
        st = _stage(tail)
        shape = (B, H, W, ch)
        yield ("convT", ch, R, S, pad, ch), st, chain.route(st, shape, ch), shape, ch
        st = _stage(first)
        shape = (B, H, W, 8)
        for c_log in range(1, 9):
            yield ("conv", ch, R, S, pad, c_log), st, chain.route(st, shape, c_log), shape, c_log


def test_no_route_promises_a_launch_the_kernels_refuse():
    from ali_hip import ops
    ops.reload_tuning()
    broken, direct, points = [], 0, 0
    for point, st, rt, shape, c_log in _sweep():
        points += 1
        for label, op, args, kw in launches(st, rt, shape, c_log):
            direct += 1
            if ops.tconv1_route(op, *args, **kw) is None:
                broken.append((point, label))
    print(f"DIRECT-SUPPORT points={points} direct launches={direct} refused={len(broken)}")
    assert points == len(CHANNELS) * 49 * 3 * (1 + 8) and direct > 1000        # (not vacuous)
    assert not broken, f"{len(broken)} promised launches are refused, e.g. {broken[:8]}"


# (kind, channels, R, S, c_log) -> what the stage must route to.  The first two are the shapes that used to plan fine
# and raise from the C ABI in the backward pass; the others pin that the fix did not simply switch the routes off.
PINNED = {
    ("conv", 128, 5, 5, 3): dict(wgrad="conv", planes="direct"),          # 25 taps at 2 per accumulator: 13 > 7
    ("convT", 128, 4, 4, 128): dict(fwd="scatter_gemm", wgrad="convT", dgrad="convT"),
    ("convT", 256, 3, 3, 256): dict(fwd="scatter_gemm", wgrad="convT", dgrad="convT"),
    ("convT", 64, 3, 4, 64): dict(fwd="scatter", wgrad="convT_scatter", dgrad="convT"),   # rectangular: fwd refuses
    ("conv", 64, 3, 5, 5): dict(wgrad="first_direct", planes="scatter"),   # ... the weight gradient takes it
    ("conv", 64, 5, 5, 5): dict(wgrad="first_direct", planes="direct"),
    ("conv", 256, 2, 3, 1): dict(wgrad="first_direct", planes="scatter"),
    ("conv", 256, 1, 1, 8): dict(wgrad="first_direct", planes="direct"),
    ("convT", 64, 4, 4, 64): dict(fwd="tconv1", wgrad="tconv1", dgrad="tconv1"),
    ("convT", 128, 3, 3, 128): dict(fwd="tconv1", wgrad="tconv1", dgrad="tconv1"),
    ("convT", 256, 2, 2, 256): dict(fwd="tconv1", wgrad="tconv1", dgrad="tconv1"),
    ("convT", 32, 5, 5, 32): dict(fwd="tconv1", wgrad="tconv1", dgrad="tconv1"),
}


@pytest.mark.parametrize("key", sorted(PINNED), ids=lambda k: "-".join(map(str, k)))
def test_pinned_points(key):
    from ali_hip import chain, ops
    ops.reload_tuning()
    kind, ch, R, S, c_log = key
    with torch.device("meta"):
        seq = (nn.Sequential(nn.ConvTranspose2d(ch, 1, (R, S))) if kind == "convT"
               else nn.Sequential(nn.Conv2d(8, ch, (R, S))))
    rt = chain.route(_stage(seq), (B, H, W, ch if kind == "convT" else 8), c_log)
    got = dict(fwd=rt.fwd, wgrad=rt.wgrad[0], dgrad=rt.dgrad, planes=rt.planes)
    assert {k: got[k] for k in PINNED[key]} == PINNED[key], (key, rt)


def test_query_names_and_refusals():
    """the wrapper's names, and the refusals the issue lists -- none of them needs a device"""
    from ali_hip import ops
    ops.reload_tuning()
    assert ops.tconv1_route("fwd", 4, 7, 9, 64, 5, 5, 0) == "fwd_mfma<2,4>"
    assert ops.tconv1_route("fwd", 4, 7, 9, 128, 4, 4, 1) == "fwd<16,4>"
    assert ops.tconv1_route("dgrad", 4, 7, 9, 64, 1, 4, 0) == "dgrad_band<4>"
    assert ops.tconv1_route("wgrad", 4, 7, 9, 32, 2, 3, 0, nc=5) == "wgrad_rb<5,3>"
    assert ops.tconv1_route("wgrad", 4, 7, 9, 64, 3, 3, 1, nc=1) == "wgrad_mfma<1,8>"
    assert ops.tconv1_route("wgrad", 4, 7, 9, 64, 3, 3, 1, nc=3) == "wgrad<3>"
    assert ops.tconv1_route("fwd", 4, 7, 9, 64, 3, 4, 0) is None            # R != S on the forward
    assert ops.tconv1_route("fwd", 4, 7, 9, 64, 6, 6, 0) is None            # S = 6
    assert ops.tconv1_route("dgrad", 4, 7, 9, 64, 1, 6, 0) is None
    assert ops.tconv1_route("wgrad", 4, 7, 9, 128, 4, 4, 0) is None         # 16 taps over 2 groups: 8 accumulators
    assert ops.tconv1_route("wgrad", 4, 7, 9, 256, 3, 3, 0) is None         # 9 taps, one group
    assert ops.tconv1_route("dgrad", 4, 7, 9, 48, 3, 3, 0) is None          # K / 4 = 12 does not divide 256
    assert ops.tconv1_route("wgrad", 4, 7, 9, 64, 3, 3, 0, nc=9) is None
    assert ops.tconv1_route("wgrad", 4, 7, 9, 64, 3, 3, 0, nc=2, ws_bytes=8192) is None     # workspace too small
    with ops.tuning(ALI_NO_T1_MFMA=1):
        assert ops.tconv1_route("fwd", 4, 7, 9, 64, 5, 5, 0) == "fwd<25,5>"
        assert ops.tconv1_route("dgrad", 4, 7, 9, 64, 5, 5, 0) == "dgrad<25>"
        assert ops.tconv1_route("wgrad", 4, 7, 9, 64, 5, 5, 0) == "wgrad<1>"
    assert ops.tconv1_route("fwd", 4, 7, 9, 64, 5, 5, 0) == "fwd_mfma<2,4>"
