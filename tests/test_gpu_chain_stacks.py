"""``ali_hip.chain.run_chain`` against fp64 autograd on small stacks: every route and every between-stage decision
(mask folding, BatchNorm partials, the stand-alone ``ali_bn_*`` passes, the GEMM that replaces a kernel without an
epilogue) that no shipped model reaches.  The stacks are ``SYNTHETIC`` of test_chain_routes.py, which pins their routes
by name, and ``chain_stacks.NEW_STACKS``.

Reference: the stock modules on the CPU in fp64 under autograd, Dropout2d masks from one ``MaskTape``.  Yardstick: a
deep copy in CPU fp32 with the same masks replayed.  Device: ``run_chain`` under ``dropout.injected_masks``, one random
cotangent.  With e(t) = max|t - ref64| and s = max|ref64|, for the output, the input gradient (logical channels) and
every parameter gradient:
    e(device) <= 2e-4 * s                                  (RTOL, never loosened)
    e(device) <= max(4 * e(cpu fp32), 4 * 2^-23 * s)       (the project's 4x yardstick; the floor is four fp32 ulps at
                                                            the tensor's scale: on tensors this small the host's own
                                                            error is often below one ulp, and four times a lucky
                                                            rounding is less than any other summation order can promise)
BatchNorm buffers: running statistics to 1e-5 * s and ``num_batches_tracked`` exactly in train mode, bit-identical to
their values before the pass in eval mode.  The inputs are re-seeded (24 draws at most) until the fp64 forward has no
LeakyReLU or ReLU input within 4e-7 * max of zero (``ActTieWatch``); the comparison pass is strict about it.
DESIGN.md 4 has the measured e(device) / e(cpu fp32) per stack (worst: 3.93, the bias gradient of ``tconv1_tanh``; no
tensor needed the floor or ``CAP_ONLY``)."""
import copy

import pytest
import torch
import torch.nn as nn

import ali_oracle as orc
from chain_stacks import NEW_STACKS
from test_chain_routes import SYNTHETIC, SYNTHETIC_EXPECTED, _walk
from test_gpu_modules import TieWatch

gpu = pytest.mark.gpu

RTOL = 2e-4               # of max|ref64|: never loosened
YARD = 4.0                # times the deviation of the CPU fp32 evaluation
FLOOR = 4.0 * 2.0 ** -23  # of max|ref64|: four fp32 ulps at the tensor's scale
BUF_TOL = 1e-5            # running statistics (test_gpu_kernels.py, test_gpu_modules.py)

STACKS = {**SYNTHETIC, **NEW_STACKS}
EXTRA = ["first_bn", "first_unpadded", "convT_bn_drop", "tanh_drop", "scatter_gemm", "bn_flat", "linear_unflat_bn"]

# (stack, mode, tensor) -> why the 4x yardstick does not apply (the 2e-4 cap still does).  At most 3; see DESIGN.md 4.
CAP_ONLY = {}


class ActTieWatch(TieWatch):
    """``TieWatch`` over the LeakyReLU and the ReLU inputs (ReLU runs as LeakyReLU with slope 0 on the device)"""

    def __init__(self, *mods, strict=False):
        self.ties, self.strict = 0, strict
        self.hooks = [m.register_forward_hook(self._hook) for mod in mods for m in mod.modules()
                      if isinstance(m, (nn.LeakyReLU, nn.ReLU))]


def _has(seq, *kinds):
    return any(isinstance(m, kinds) or type(m).__name__ == "TapedDropout2d" and nn.Dropout2d in kinds for m in seq)


def build(name):
    """the stack on the CPU in fp32: fixed seed, Dropout2d swapped for the taped stand-in at the same index,
    non-trivial BatchNorm parameters and running statistics"""
    make = STACKS[name][0]
    torch.manual_seed(1000 + sorted(STACKS).index(name))
    seq = make()
    g = torch.Generator().manual_seed(77)
    for i, m in enumerate(seq):
        if isinstance(m, nn.Dropout2d):
            seq[i] = orc.TapedDropout2d(m.p)
        elif isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=g))
                if m.running_mean is not None:
                    m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return seq


def to_ref_input(x_nhwc, c_log, seq):
    """the reference's view of the device input: logical channels as NCHW, or [B, c_log] in front of a Linear"""
    x = x_nhwc[..., :c_log]
    first = next(m for m in seq if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)))
    return x.reshape(x.shape[0], c_log).clone() if isinstance(first, nn.Linear) else x.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    """a reference tensor ([B,C,H,W] or [B,C]) in the device's layout"""
    return t.permute(0, 2, 3, 1).contiguous() if t.dim() == 4 else t.reshape(t.shape[0], 1, 1, -1)


def host_pass(seq, x, cot, masks, dtype, strict=False):
    """one forward + backward of a deep copy of ``seq`` in ``dtype`` with ``masks`` replayed: a dict of results, the
    copy itself under "model" (its BatchNorm buffers are the ones after the pass)"""
    m = copy.deepcopy(seq).to(dtype)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    xr = x.to(dtype).requires_grad_(True)
    with orc.use_tape(orc.MaskTape(replay=masks)), ActTieWatch(m, strict=strict):
        y = m(xr)
    y.backward(cot.to(dtype))
    return {"y": y.detach(), "gx": xr.grad, "gp": {k: p.grad for k, p in m.named_parameters()},
            "buf": {k: v for k, v in m.state_dict().items() if "running" in k or "num_batches" in k},
            "before": before, "model": m}


def half_forward(res, x, masks, dtype):
    """forward of ``res``'s model after every parameter was halved in place (a copy: ``res`` stays as it is)"""
    m = copy.deepcopy(res["model"])
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
        with orc.use_tape(orc.MaskTape(replay=masks)):
            return m(x.to(dtype))


_REF = {}


def reference(name, mode):
    """tie-free input, cotangent, masks and the fp64 / fp32 host passes of (stack, mode): computed once, never changed"""
    key = (name, mode)
    if key in _REF:
        return _REF[key]
    _, shape, c_log = STACKS[name]
    seq = build(name).train(mode == "train")
    for v in range(24):                                  # (tie_free's draws, with the watcher of both activations)
        g = torch.Generator().manual_seed(500 + 31 * v)
        x = torch.zeros(shape)
        x[..., :c_log] = torch.randn(shape[:3] + (c_log,), generator=g)
        xr = to_ref_input(x, c_log, seq)
        probe = copy.deepcopy(seq).double()
        torch.manual_seed(900 + v)                       # (the tape draws from the global CPU generator)
        tape = orc.MaskTape()
        with orc.use_tape(tape), ActTieWatch(probe) as tw, torch.no_grad():
            y = probe(xr.double())
        if tw.ties == 0:
            break
    else:
        pytest.fail(f"{name}/{mode}: no tie-free case in 24 draws")
    cot = torch.randn(y.shape, generator=g)
    r64 = host_pass(seq, xr, cot, tape.masks, torch.float64, strict=True)
    r32 = host_pass(seq, xr, cot, tape.masks, torch.float32)
    half = (half_forward(r64, xr, tape.masks, torch.float64), half_forward(r32, xr, tape.masks, torch.float32))
    _REF[key] = dict(seq=seq, x=x, cot=cot, masks=tape.masks, c_log=c_log, r64=r64, r32=r32, half=half)
    return _REF[key]


def _check(label, got, ref, f32, cap_key=None):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    s = ref.abs().max().item()
    e_dev = (got - ref).abs().max().item()
    e_cpu = (f32.double() - ref).abs().max().item()
    print(f"CHAIN {label} e_dev={e_dev:.3e} e_cpu={e_cpu:.3e} scale={s:.3e} ratio={e_dev / max(e_cpu, 1e-300):.2f}")
    assert e_dev == e_dev, f"{label}: NaN"
    assert e_dev <= RTOL * s, f"{label}: max err {e_dev:.3e} vs {RTOL} * {s:.3e}"
    if cap_key not in CAP_ONLY:
        bound = max(YARD * e_cpu, FLOOR * s)
        assert e_dev <= bound, f"{label}: max err {e_dev:.3e} > max({YARD} * {e_cpu:.3e}, 4 ulp * {s:.3e})"


def device_pass(r, need_gx=True, need_params=True, train=True):
    """``run_chain`` of a fresh device copy on the reference's input; returns (model, x, y)"""
    from ali_hip import chain, dropout
    dev = copy.deepcopy(r["seq"]).cuda().train(train)
    for p in dev.parameters():
        p.requires_grad_(need_params)
    xd = r["x"].cuda().requires_grad_(need_gx)
    with dropout.injected_masks(r["masks"]):
        y = chain.run_chain(dev, xd, r["c_log"])
        assert dropout.masks_consumed() == len(r["masks"])
    y.backward(nhwc(r["cot"]).cuda())
    return dev, xd, y


def check_gx(label, r, xd, key):
    _check(f"{label} gx", xd.grad[..., :r["c_log"]], nhwc(r["r64"]["gx"]), nhwc(r["r32"]["gx"]), key + ("gx",))


def check_param_grads(label, r, dev, key):
    for k, p in dev.named_parameters():
        assert p.grad is not None, f"{label}: {k}.grad is missing"
        _check(f"{label} {k}.grad", p.grad, r["r64"]["gp"][k], r["r32"]["gp"][k], key + (k + ".grad",))


MODES = [(n, "train") for n in STACKS] + [(n, "eval") for n in STACKS
                                          if _has(STACKS[n][0](), nn.BatchNorm2d, nn.Dropout2d)]


@gpu
@pytest.mark.parametrize("name,mode", MODES, ids=[f"{n}-{m}" for n, m in MODES])
def test_stack_matches_fp64_autograd(name, mode):
    r = reference(name, mode)
    key, label = (name, mode), f"{name}/{mode}"
    if name == "head_odd":             # the taped stand-in is planned as the Dropout2d it replaces
        with torch.device("meta"):
            taped = nn.Sequential(orc.TapedDropout2d(0.2), nn.Conv2d(6, 1, 1))
        assert _walk(taped, *STACKS[name][1:])[1:] == SYNTHETIC_EXPECTED[name]
    assert (len(r["masks"]) > 0) == (mode == "train" and _has(r["seq"], nn.Dropout2d))
    dev, xd, y = device_pass(r, train=mode == "train")
    _check(f"{label} y", y, nhwc(r["r64"]["y"]), nhwc(r["r32"]["y"]), key + ("y",))
    check_gx(label, r, xd, key)
    check_param_grads(label, r, dev, key)
    bufs = {k: v for k, v in dev.state_dict().items() if "running" in k or "num_batches" in k}
    assert sorted(bufs) == sorted(r["r64"]["buf"])
    for k, v in bufs.items():
        if mode == "eval":
            assert torch.equal(v.cpu(), r["r64"]["before"][k].to(v.dtype)), f"{label} {k}: changed in eval mode"
        elif "num_batches" in k:
            assert int(v) == int(r["r64"]["buf"][k]) == int(r["r64"]["before"][k]) + 1, f"{label} {k}"
        else:
            ref = r["r64"]["buf"][k]
            err, s = (v.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
            print(f"CHAIN {label} {k} err={err:.3e} scale={s:.3e}")
            assert err <= BUF_TOL * s, f"{label} {k}: {err:.3e} vs {BUF_TOL} * {s:.3e}"


@gpu
@pytest.mark.parametrize("name", EXTRA)
def test_frozen_parameters_only_the_input_gradient(name):
    """the explainers' use (``need_params=False``)"""
    r = reference(name, "train")
    dev, xd, _ = device_pass(r, need_params=False)
    check_gx(f"{name}/frozen", r, xd, (name, "frozen"))
    assert all(p.grad is None for p in dev.parameters())


@gpu
@pytest.mark.parametrize("name", EXTRA)
def test_no_input_gradient_keeps_the_parameter_gradients(name):
    """(``first_bn``: the BatchNorm in front of the first conv still gets its gradients from the data-gradient pass)"""
    r = reference(name, "train")
    dev, xd, _ = device_pass(r, need_gx=False)
    assert xd.grad is None
    check_param_grads(f"{name}/no-gx", r, dev, (name, "no-gx"))


@gpu
@pytest.mark.parametrize("name", EXTRA)
def test_packs_follow_an_in_place_parameter_edit(name):
    """every parameter halved in place after a first pass: the same plan's forward must read the new values (a
    ``PackCache`` entry that missed the version bump shows up here)"""
    from ali_hip import chain, dropout
    r = reference(name, "train")
    dev, _, _ = device_pass(r)
    plan = chain.get_plan(dev)
    with torch.no_grad():
        for p in dev.parameters():
            p.mul_(0.5)
    with dropout.injected_masks(r["masks"]), torch.no_grad():
        y = chain.run_chain(dev, r["x"].cuda(), r["c_log"])
    assert chain.get_plan(dev) is plan
    _check(f"{name}/halved y", y, nhwc(r["half"][0]), nhwc(r["half"][1]), (name, "halved", "y"))


# ---------------------------------------------------------------------- grouped passes
# name -> (B, H, W, K, pre-ops, the BatchNorm statistics ride the first conv's epilogue)
GROUPED = {
    "aligned_drop_bn": (4, 10, 10, 16, ["drop", "bn"], True),
    "aligned_bn_drop": (4, 10, 10, 16, ["bn", "drop"], True),
    "misaligned_vec": (6, 7, 6, 16, ["bn"], False),           # 60-row passes, 16 channels: the float4 group launch
    "misaligned_scalar": (6, 7, 6, 6, ["bn", "drop"], False),   # 6 channels: the scalar per-group loop
}


def grouped_stack(K, pre):
    torch.manual_seed(4242 + K + len(pre))
    mid = {"drop": lambda: orc.TapedDropout2d(0.25), "bn": lambda: nn.BatchNorm2d(K)}
    seq = nn.Sequential(nn.Conv2d(8, K, 3), nn.LeakyReLU(0.1), *[mid[k]() for k in pre], nn.Conv2d(K, 8, 3),
                        nn.LeakyReLU(0.2))
    g = torch.Generator().manual_seed(78)
    bn = next(m for m in seq if isinstance(m, nn.BatchNorm2d))
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(K, generator=g))
        bn.bias.copy_(0.3 * torch.randn(K, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(K, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(K, generator=g))
    return seq


def grouped_host(seq, xs, cots, masks, dtype, strict=False):
    """two consecutive train-mode forwards, then one backward per pass with the gradients zeroed in between"""
    m = copy.deepcopy(seq).to(dtype).train()
    xr = [x.to(dtype).requires_grad_(True) for x in xs]
    with orc.use_tape(orc.MaskTape(replay=masks)), ActTieWatch(m, strict=strict):
        ys = [m(x) for x in xr]
    out = []
    for x, y, cot in zip(xr, ys, cots):
        m.zero_grad()
        y.backward(cot.to(dtype))
        out.append({"y": y.detach(), "gx": x.grad, "gp": {k: p.grad.clone() for k, p in m.named_parameters()}})
    return out, {k: v for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


def grouped_reference(case):
    """(stack, NHWC input, cotangents, masks, fp64 passes, fp64 buffers, fp32 passes) of a grouped case"""
    B, H, W, K, pre, _ = GROUPED[case]
    seq = grouped_stack(K, pre).train()
    for v in range(24):
        g = torch.Generator().manual_seed(700 + 31 * v)
        x = torch.randn(B, H, W, 8, generator=g)
        xs = [x[:B // 2].permute(0, 3, 1, 2).contiguous(), x[B // 2:].permute(0, 3, 1, 2).contiguous()]
        probe = copy.deepcopy(seq).double()
        torch.manual_seed(950 + v)
        tape = orc.MaskTape()
        with orc.use_tape(tape), ActTieWatch(probe) as tw, torch.no_grad():
            ys = [probe(t.double()) for t in xs]
        if tw.ties == 0:
            break
    else:
        pytest.fail(f"{case}: no tie-free case in 24 draws")
    cots = [torch.randn(y.shape, generator=g) for y in ys]
    assert len(tape.masks) == (2 if "drop" in pre else 0)
    r64, buf64 = grouped_host(seq, xs, cots, tape.masks, torch.float64, strict=True)
    r32, _ = grouped_host(seq, xs, cots, tape.masks, torch.float32)
    return seq, x, cots, tape.masks, r64, buf64, r32


@gpu
@pytest.mark.parametrize("case", sorted(GROUPED))
def test_grouped_passes_equal_consecutive_calls(case, monkeypatch):
    from ali_hip import chain, dropout, ops
    B, rides = GROUPED[case][0], GROUPED[case][5]
    seq, x, cots, masks, r64, buf64, r32 = grouped_reference(case)
    dev = copy.deepcopy(seq).cuda().train()
    plan = chain.get_plan(dev)
    calls = []

    def spy(name):
        real = getattr(ops, name)

        def wrapped(*a, **k):
            calls.append((name, k.get("groups")))
            return real(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    spy("bn_stats"), spy("bn_stats_from_partials")
    # the mask of a request: the two passes' masks, concatenated along the sample axis
    with dropout.injected_masks([torch.cat(masks, dim=0)] if masks else []), torch.no_grad():
        y, saved = chain.chain_forward(plan, x.cuda(), True, 8, save=True, groups=2)
    # which side of _for_next_stage's predicate the case is on, from the library's own tile choice
    slots, tile_rows, pixel_major = ops.conv_mtiles(saved[0].geom, 0)
    P, Q = saved[0].out_shape[1:3]
    rows_g = (B // 2) * (1 if pixel_major else P * Q)
    assert (slots > 0 and rows_g % tile_rows == 0 and (not pixel_major or B % tile_rows == 0)) == rides, \
        (case, slots, tile_rows, pixel_major, rows_g)
    assert calls == ([("bn_stats_from_partials", None)] if rides else [("bn_stats", 2)])
    names = {id(p): k for k, p in dev.named_parameters()}
    for gi in range(2):
        lo, hi = gi * (B // 2), (gi + 1) * (B // 2)
        label = f"grouped/{case}/pass{gi}"
        _check(f"{label} y", y[lo:hi], nhwc(r64[gi]["y"]), nhwc(r32[gi]["y"]))
        with torch.no_grad():
            gx, grads = chain.chain_backward(plan, chain.slice_saved(saved, gi, 2), nhwc(cots[gi]).cuda(), 8, True)
        _check(f"{label} gx", gx, nhwc(r64[gi]["gx"]), nhwc(r32[gi]["gx"]))
        assert sorted(names[i] for i in grads) == sorted(r64[gi]["gp"])
        for i, gr in grads.items():
            _check(f"{label} {names[i]}.grad", gr, r64[gi]["gp"][names[i]], r32[gi]["gp"][names[i]])
    for k, v in dev.state_dict().items():
        if "num_batches" in k:
            assert int(v) == int(buf64[k]) == 2, k
        elif "running" in k:
            err, s = (v.double().cpu() - buf64[k]).abs().max().item(), buf64[k].abs().max().item()
            print(f"CHAIN grouped/{case} {k} err={err:.3e} scale={s:.3e}")
            assert err <= BUF_TOL * s, f"{case} {k}: {err:.3e} vs {BUF_TOL} * {s:.3e}"
