"""The three kernels of csrc/cfmetrics.hip: ali_mse, ali_cf_recon, ali_oracle_scores.

Reference: the torch statement on the CPU in fp64; yardstick: the same in CPU fp32; with e(t) = max|t - ref64| every
continuous result is held to the two bounds of test_gpu_conv_geometry.py through ``_check`` of test_gpu_xent.py,
    e(device) <= YARD * e(cpu fp32)     and     e(device) <= RTOL * max|ref64|.
Where the CPU-fp32 result equals fp64 by construction (y == x, ocf == ox, the os column of given logits, NaN columns)
the comparison is exact.  Every call is made twice: the same bits; the workspace's reserved head is zero afterwards.
"""
import pytest
import torch

from test_gpu_xent import _check

gpu = pytest.mark.gpu


def _head_is_zero():
    from ali_hip import ops
    assert int(ops.workspace(torch.device("cuda"))[:4096].count_nonzero()) == 0


# --------------------------------------------------------------------------------------------------------------- mse
MSE_SIZES = [1, 3, 63, 65, 784, 784 * 5, 784 * 257]


def _mse_ref(y, x, gscale, tanh_out, dt):
    yy = y.to(dt).requires_grad_(True)
    loss = (yy - x.to(dt)).square().mean()
    (g,) = torch.autograd.grad(loss * gscale, yy)
    if tanh_out:
        g = g * (1 - yy.detach() ** 2)
    return loss.detach(), g


@gpu
@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_loss_and_gradient(n):
    from ali_hip import ops
    g = torch.Generator().manual_seed(n)
    y = torch.tanh(torch.randn(n, generator=g))
    x = torch.rand(n, generator=g) * 2 - 1
    yd, xd = y.cuda(), x.cuda()
    for tanh_out in (False, True):
        for gscale in (1.0, 0.5):
            l64, g64 = _mse_ref(y, x, gscale, tanh_out, torch.float64)
            l32, g32 = _mse_ref(y, x, gscale, tanh_out, torch.float32)
            loss, grad = ops.mse(yd, xd, gscale=gscale, tanh_out=tanh_out)
            again = ops.mse(yd, xd, gscale=gscale, tanh_out=tanh_out)
            label = f"mse n={n} tanh={tanh_out} gs={gscale}"
            assert loss.dim() == 0
            _check(label + " loss", loss, l64, l32)
            _check(label + " grad", grad, g64, g32)
            assert torch.equal(loss, again[0]) and torch.equal(grad, again[1]), label
            bare, none = ops.mse(yd, xd, gscale=gscale, want_grad=False, tanh_out=tanh_out)
            assert none is None and torch.equal(bare, loss), label
    # an operand that is not 16-byte aligned takes the element-wise path: the same loss within the bounds
    if n > 1:
        l64, g64 = _mse_ref(y[1:], x[1:], 1.0, True, torch.float64)
        l32, g32 = _mse_ref(y[1:], x[1:], 1.0, True, torch.float32)
        loss, grad = ops.mse(yd[1:], xd[1:], tanh_out=True)
        _check(f"mse n={n} unaligned loss", loss, l64, l32)
        _check(f"mse n={n} unaligned grad", grad, g64, g32)
    # y == x: loss and gradient exactly zero
    loss, grad = ops.mse(yd, yd.clone(), tanh_out=True)
    assert loss.item() == 0.0 and torch.equal(grad, torch.zeros_like(grad))
    _head_is_zero()


# ---------------------------------------------------------------------------------------------------------- cf_recon
RECON_SHAPES = [(B, N, A) for B in (1, 5, 64, 257) for N in (1, 63, 784, 785) for A in (2, 11)]


def _recon_ref(x, recon, orig, target, dt):
    x, recon = x.to(dt), recon.to(dt)
    rows = torch.arange(x.shape[0])
    r_o, r_t = recon[orig.long(), rows], recon[target.long(), rows]
    return torch.stack([x.abs().sum(1), (x - r_o).square().sum(1), (x - r_t).square().sum(1),
                        (r_t - recon[-1]).square().sum(1)], dim=1)


@gpu
@pytest.mark.parametrize("B,N,A", RECON_SHAPES, ids=[f"B{b}-N{n}-A{a}" for b, n, a in RECON_SHAPES])
def test_cf_recon_columns(B, N, A):
    from ali_hip import ops
    g = torch.Generator().manual_seed(100 * B + N + A)
    x = torch.rand(B, N, generator=g) * 2 - 1
    recon = torch.rand(A, B, N, generator=g) * 2 - 1
    orig = torch.randint(0, A - 1, (B,), generator=g, dtype=torch.int32)
    target = torch.randint(0, A - 1, (B,), generator=g, dtype=torch.int32)
    target[::3] = orig[::3]                                   # rows with orig == target
    if B >= 5:
        orig[1] = target[1] = 0                               # both at the first plane
        orig[2] = target[2] = A - 2                           # both at the last class plane
    want64, want32 = _recon_ref(x, recon, orig, target, torch.float64), _recon_ref(x, recon, orig, target, torch.float32)
    xd, rd, od, td = x.cuda(), recon.cuda(), orig.cuda(), target.cuda()
    out = ops.cf_recon(xd, rd, od, td)
    label = f"cf_recon B={B} N={N} A={A}"
    for i, name in enumerate(("l1", "o_rec", "t_rec", "all_rec")):
        _check(f"{label} {name}", out[:, i], want64[:, i], want32[:, i])
    same = (orig == target).cuda()
    assert torch.equal(out[same, 1], out[same, 2]), label
    assert torch.equal(out, ops.cf_recon(xd, rd, od, td)), label
    # non-contiguous recon: planes and rows of a wider buffer (row pitch N + 3: the element-wise path where N % 4 == 0)
    wide = torch.full((A + 1, B + 2, N + 3), float("nan"), device="cuda")
    view = wide[1:, 1:B + 1, 2:N + 2]
    view.copy_(rd)
    assert not view.is_contiguous() or B * N == 1
    strided = ops.cf_recon(xd, view, od, td)
    for i, name in enumerate(("l1", "o_rec", "t_rec", "all_rec")):
        _check(f"{label} strided {name}", strided[:, i], want64[:, i], want32[:, i])
    # the same on 16-byte boundaries (pitch N + 4, offset 4): the float4 path with ld_row != N and ld_plane != B * N
    if N % 4 == 0:
        wide4 = torch.full((A + 1, B + 2, N + 4), float("nan"), device="cuda")
        view4 = wide4[1:, 1:B + 1, 4:]
        view4.copy_(rd)
        assert view4.data_ptr() % 16 == 0 and view4.stride(1) == N + 4 and view4.stride(0) == (B + 2) * (N + 4)
        strided4 = ops.cf_recon(xd, view4, od, td)
        assert torch.equal(strided4, out), label             # the same lanes add the same elements in the same order
    # one label out of range: NaN in the columns that depend on it, every other row and column untouched
    for which, bad in (("orig", A - 1), ("target", -1), ("target", A + 5)):
        o2, t2 = od.clone(), td.clone()
        r = B // 2
        (o2 if which == "orig" else t2)[r] = bad
        got = ops.cf_recon(xd, rd, o2, t2)
        nan_cols = [1] if which == "orig" else [2, 3]
        keep = torch.ones(B, 4, dtype=torch.bool, device="cuda")
        keep[r, nan_cols] = False
        assert torch.isnan(got[r, nan_cols]).all() and torch.equal(got[keep], out[keep]), (label, which, bad)


# ----------------------------------------------------------------------------------------------------- oracle_scores
ORACLE_SHAPES = [(B, J, C) for B in (1, 5, 257) for J in (1, 10) for C in (1, 2, 10, 65, 257)]
ORACLE_VARIANTS = ("normal", "scale80", "scale1e4", "ties")


def _oracle_inputs(B, J, C, variant):
    g = torch.Generator().manual_seed(1000 * B + 10 * C + J)
    ox, ocf = torch.randn(J, B, C, generator=g), torch.randn(J, B, C, generator=g)
    if variant == "scale80":
        ox, ocf = ox * 80.0, ocf * 80.0
    elif variant == "scale1e4":
        ox, ocf = ox * 1e4, ocf * 1e4
    elif variant == "ties":
        for j in range(J):
            for b in range(B):
                top = ocf[j, b].max().item() + 1.0
                k = 3 * b + j
                ocf[j, b, [k % C, (k + 64) % C, (k + 7) % C]] = top      # one lane's columns (k, k + 64), another lane
    am = ocf.argmax(2)                                                   # [J, B], the first maximum
    pred = am[(torch.arange(B) * 7) % J, torch.arange(B)].clone()        # agrees with one oracle per row ...
    pred[::4] = (pred[::4] + 1) % C                                      # ... or (C > 1) with none
    return pred.to(torch.int32), ox.contiguous(), ocf.contiguous()


def _js(p, q):
    p, q = p.softmax(-1), q.softmax(-1)
    m = 0.5 * (p + q)
    lm = (m + 1e-6).log()
    return 0.5 * ((p * ((p + 1e-6).log() - lm)).sum(-1) + (q * ((q + 1e-6).log() - lm)).sum(-1))


@gpu
@pytest.mark.parametrize("B,J,C", ORACLE_SHAPES, ids=[f"B{b}-J{j}-C{c}" for b, j, c in ORACLE_SHAPES])
def test_oracle_scores(B, J, C):
    from ali_hip import ops
    for variant in ORACLE_VARIANTS:
        pred, ox, ocf = _oracle_inputs(B, J, C, variant)
        want_os = (pred.long().reshape(1, B) == ocf.argmax(2)).t().to(torch.int32)          # [B, J]
        lvs64, lvs32 = _js(ox.double(), ocf.double()).t(), _js(ox, ocf).t()
        pd, oxd, ocfd = pred.cuda(), ox.cuda(), ocf.cuda()
        os_, lvs = ops.oracle_scores(pd, oxd, ocfd)
        label = f"oracle B={B} J={J} C={C} {variant}"
        assert os_.dtype == torch.int32 and tuple(os_.shape) == (B, J) and tuple(lvs.shape) == (B, J)
        assert torch.equal(os_.cpu(), want_os), label
        _check(label + " lvs", lvs, lvs64, lvs32)
        again = ops.oracle_scores(pd, oxd, ocfd)
        assert torch.equal(os_, again[0]) and torch.equal(lvs, again[1]), label
        # the two halves of one [J, 2, B, C] buffer (how CfMetrics holds them): the same bits
        pair = torch.stack([oxd, ocfd], dim=1)
        halves = ops.oracle_scores(pd, pair[:, 0], pair[:, 1])
        assert torch.equal(os_, halves[0]) and torch.equal(lvs, halves[1]), label
        # ocf == ox: m = p bit for bit, every term p * (L - L)
        _, zero = ops.oracle_scores(pd, ocfd, ocfd.clone())
        assert torch.equal(zero, torch.zeros_like(zero)), label
    _head_is_zero()
