"""The Discriminator head's backward pass in one launch (csrc/elementwise.hip: ``ali_head_bwd``).  It
replaces the data-gradient GEMM with one gathered channel (mask and act' in its epilogue) and ``ali_head_wgrad``, and
keeps their arithmetic and summation order: every output is compared BIT FOR BIT with the launches it replaces, on
the same operands, and held to a float64 restatement at the bound tests/test_gpu_kernels.py uses for the GEMM, the GEMV's
weight gradient (RTOL) and its bias gradient (1e-5).  The chain runs with ALI_NO_HEAD_BWD set and unset; the stepper
with both switches of the pull request (ALI_NO_HEAD_BWD, and ALI_NO_GZ_CHAIN: G'(z) as the third chain of the D-real
rounds) set and unset.

Shapes: B = 64 is full blocks everywhere, B = 130 leaves ragged rows in every kernel (64 rows a block in the data
gradient, 8 row lanes of 8 accumulators in the weight gradient: a third, partly empty pass); C = 1024 is the product's
head, C = 20 is less than one 32-column block."""
import pytest
import torch
import torch.nn as nn

from test_gpu_input_pipeline import _assert_same_result, _assert_same_state, _dataset, _host_batch, _mnist_models
from test_gpu_kernels import close

pytestmark = pytest.mark.gpu

DSLOPE = 0.1
SWITCHES = ("ALI_NO_HEAD_BWD", "ALI_NO_GZ_CHAIN")


def _ops():
    from ali_hip import ops
    return ops


def _rows(t, wide):
    """``t`` [B, C] on the device: dense, or as the column range [32, 32 + C) of a buffer 96 floats wider"""
    if not wide:
        return t.cuda()
    buf = torch.full((t.shape[0], t.shape[1] + 96), 7.0, device="cuda")
    buf[:, 32:32 + t.shape[1]] = t.cuda()
    return buf[:, 32:32 + t.shape[1]]


# ------------------------------------------------------------------------------------------------ ali_head_bwd
@pytest.mark.parametrize("wg", [True, False], ids=["dw_db", "data_only"])
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "column_range"])
@pytest.mark.parametrize("C", [1024, 20])
@pytest.mark.parametrize("B", [64, 130])
def test_head_bwd_equals_the_gemm_and_head_wgrad(B, C, wide, wg):
    """g = gl (x) w with the Dropout2d mask and LeakyReLU' of the previous stage, dw and db: bit for bit what
    ``conv_bwd_data`` (the operands of ``chain._data_grad``) and ``head_wgrad`` leave.  ``wide``: the rows of the
    weight-gradient operand x and of the mask are column ranges of wider buffers."""
    ops = _ops()
    gen = torch.Generator().manual_seed(B + C + wide)
    gl = torch.randn(B, generator=gen) / B
    w = torch.randn(C, generator=gen) / C ** 0.5
    yprev = torch.randn(B, C, generator=gen)
    x = torch.randn(B, C, generator=gen)
    mask = (torch.rand(B, C, generator=gen) > 0.2).float() * 1.25
    gld, wd, ypd, xd = gl.cuda(), w.cuda(), yprev.cuda(), _rows(x, wide)
    mk_full = mkd = _rows(mask, wide)

    # the launches it replaces
    geom = ops.geom(B, 1, 1, C, 1, 1, 1, 1, 1, 1, 0)
    g_old = torch.full((B, 1, 1, C), float("nan"), device="cuda")
    ep = ops.epilogue(dact_y=ypd.reshape(B, 1, 1, C), dact=ops.ACT_LEAKY, dslope=DSLOPE)
    ep.mask, ep.mask_ld = mkd.data_ptr(), mkd.stride(0)
    ep.refs["mask"] = mkd
    ops.conv_bwd_data(geom, gld.reshape(B, 1, 1, 1), wd.reshape(C, 1, 1), g_old, ep, live=(C, None))
    dw_old, db_old = torch.full((C,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    ops.head_wgrad(xd, gld, dw_old, db_old)

    g_new = torch.full((B, C), float("nan"), device="cuda")
    dw_new, db_new = (torch.full((C,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda"))
    if wg:       # (twice: an arrival counter left non-zero by the first launch would spoil the second)
        ops.head_bwd(gld, wd, ypd, ops.ACT_LEAKY, DSLOPE, mk_full, g_new, xd, torch.empty_like(dw_new), torch.empty_like(db_new))
        ops.head_bwd(gld, wd, ypd, ops.ACT_LEAKY, DSLOPE, mk_full, g_new, xd, dw_new, db_new)
        ws = ops.workspace(g_new.device)
        assert int(ws[:ops.WS_RESERVED].view(torch.int32).abs().sum()) == 0, "arrival counter left non-zero"
    else:
        ops.head_bwd(gld, wd, ypd, ops.ACT_LEAKY, DSLOPE, mk_full, g_new)
    torch.cuda.synchronize()
    assert torch.equal(g_new, g_old.reshape(B, C)), f"g: max diff {(g_new - g_old.reshape(B, C)).abs().max().item():.3e}"
    if wg:
        assert torch.equal(dw_new, dw_old) and torch.equal(db_new, db_old)
    else:
        assert torch.isnan(dw_new).all() and torch.isnan(db_new).all(), "dw == NULL: nothing may be written"
    ref = (gl.double()[:, None] * w.double()[None, :]) * mask.double() * torch.where(yprev > 0, 1.0, DSLOPE).double()
    close(g_new, ref.float(), what="head bwd g")
    if wg:
        close(dw_new, (gl.double() @ x.double()).float(), what="head bwd dw")
        close(db_new, gl.double().sum().float().reshape(1), rtol=1e-5, what="head bwd db")


def test_head_bwd_without_mask_and_activation():
    """no Dropout2d and no activation in front of the head: the plain outer product, as the GEMM with a plain epilogue"""
    ops = _ops()
    B, C = 70, 36
    gen = torch.Generator().manual_seed(5)
    gl, w = torch.randn(B, generator=gen).cuda(), torch.randn(C, generator=gen).cuda()
    g_old = torch.full((B, 1, 1, C), float("nan"), device="cuda")
    ops.conv_bwd_data(ops.geom(B, 1, 1, C, 1, 1, 1, 1, 1, 1, 0), gl.reshape(B, 1, 1, 1), w.reshape(C, 1, 1), g_old,
                      ops.epilogue(), live=(C, None))
    g_new = ops.head_bwd(gl, w, None, ops.ACT_NONE, 0.0, None, torch.full((B, C), float("nan"), device="cuda"))
    assert torch.equal(g_new, g_old.reshape(B, C))
    assert torch.equal(g_new, gl[:, None] * w[None, :])


def test_head_bwd_refuses_bad_operands():
    ops = _ops()
    g = torch.empty(8, 16, device="cuda")
    gl, w, x = torch.zeros(8, device="cuda"), torch.zeros(16, device="cuda"), torch.zeros(8, 16, device="cuda")
    with pytest.raises(RuntimeError):          # an activation without the saved output it is evaluated on
        ops.head_bwd(gl, w, None, ops.ACT_LEAKY, 0.1, None, g)
    with pytest.raises(RuntimeError):          # db without dw
        ops.head_bwd(gl, w, None, ops.ACT_NONE, 0.0, None, g, x, None, torch.zeros(1, device="cuda"))
    with pytest.raises(ValueError):
        ops.head_bwd(gl, w, None, ops.ACT_NONE, 0.0, torch.ones(8, 12, device="cuda"), g)


# ------------------------------------------------------------------------------------------------ the chain's routes
def _head_stack(C):
    torch.manual_seed(C)
    return nn.Sequential(nn.Dropout2d(0.2), nn.Conv2d(C, C, 1), nn.LeakyReLU(0.1),
                         nn.Dropout2d(0.2), nn.Conv2d(C, 1, 1)).cuda()


@pytest.mark.parametrize("need_params", [True, False], ids=["params", "data_only"])
@pytest.mark.parametrize("B,C", [(64, 1024), (130, 20)])
def test_chain_head_route_switch_on_and_off(B, C, need_params, monkeypatch):
    """A dxz-like stack (Dropout2d, 1x1 conv, LeakyReLU, Dropout2d, head) forward and backward, once on ``head_bwd`` and
    once with ALI_NO_HEAD_BWD=1: same bits everywhere, and each run took the launches its switch names."""
    from ali_hip import chain, dropout
    ops = _ops()
    seq = _head_stack(C)
    plan = chain.get_plan(seq)
    gen = torch.Generator().manual_seed(B + C)
    x = torch.randn(B, 1, 1, C, generator=gen).cuda()
    gy = (torch.randn(B, 1, 1, 1, generator=gen) / B).cuda()
    masks = [(torch.rand(B, C, generator=gen) > 0.2).float().cuda() * 1.25 for _ in range(2)]
    calls = []
    for name in ("head_bwd", "head_wgrad", "conv_bwd_data"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)

    def run():
        calls.clear()
        with dropout.injected_masks([m.clone() for m in masks]), torch.no_grad():
            y, saved = chain.chain_forward(plan, x, True, C, save=True)
            gx, grads = chain.chain_backward(plan, saved, gy, C, True, need_params)
        names = {id(p): k for k, p in seq.named_parameters()}
        torch.cuda.synchronize()
        return [y, gx] + [grads[i] for i in sorted(grads, key=names.get)], list(calls)

    new, calls_new = run()
    with ops.tuning(ALI_NO_HEAD_BWD=1):
        old, calls_old = run()
    assert calls_new.count("head_bwd") == 1 and "head_wgrad" not in calls_new and calls_new.count("conv_bwd_data") == 1
    assert "head_bwd" not in calls_old and calls_old.count("conv_bwd_data") == 2
    assert calls_old.count("head_wgrad") == int(need_params)
    assert len(new) == len(old) == 2 + (4 if need_params else 0)
    for i, (a, b) in enumerate(zip(new, old)):
        assert not torch.isnan(a).any() and torch.equal(a, b), f"output {i} differs between the routes"


# ------------------------------------------------------------------------------------------------ the whole step
@pytest.mark.parametrize("capture", [False, True], ids=["eager", "graph"])
def test_step_is_bitwise_the_same_with_all_switches_off_and_on(capture):
    """Two AliStepper iterations at B = 64 (graph: capture, then a replay) with both switches set vs unset: the
    losses, every parameter, buffer and Adam moment are equal bit for bit."""
    import ali_hip
    from ali_hip.step import AliStepper
    ops = _ops()
    x, a = _dataset(64, seed=12)
    images, c = _host_batch(x, a, torch.arange(64))
    z = torch.randn(2, 64, 512, 1, 1, generator=torch.Generator().manual_seed(4)).cuda()

    def run():
        ali_hip.manual_seed(21)
        st = AliStepper(*_mnist_models(), capture=capture)
        return st, [{k: v.clone() for k, v in st.step(images, c, z[i]).items()} for i in range(2)]

    sa, ra = run()
    with ops.tuning(**{k: 1 for k in SWITCHES}):
        sb, rb = run()
    for i in range(2):
        _assert_same_result(ra[i], rb[i], f"iteration {i}")
    _assert_same_state(sa, sb, f"capture={capture}")
