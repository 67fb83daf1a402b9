"""ali_softmax_xent (csrc/xent.hip): loss, gradient, arg-max, hit count and the device-side hit counter.

Reference: torch's cross_entropy with probability targets and autograd on the CPU in fp64; yardstick: the same in CPU
fp32.  With e(t) = max|t - ref64| the loss and the gradient are held to the two bounds of test_gpu_conv_geometry.py,
    e(device) <= YARD * e(cpu fp32)     and     e(device) <= RTOL * max|ref64|,
both imported from there.  Predictions, hit counts and the int64 accumulator are compared exactly: the logits and
targets are given (not computed on the device), and the first maximum of a given fp32 row is not a matter of rounding.

Inputs per shape: plain normal logits with one-hot targets; rows scaled to +-80 and +-1e4 (exp overflows without the
max shift); soft targets that do not sum to 1; all-zero target rows; ties of the row maximum in logits and targets,
placed in one lane's columns (j, j + 64) and in different lanes where C allows.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_geometry import RTOL, YARD

gpu = pytest.mark.gpu

SHAPES = [(B, C) for B in (1, 5, 64, 257) for C in (1, 2, 3, 10, 60, 65, 257)]
VARIANTS = ("normal", "scale80", "scale1e4", "soft", "zero_rows", "ties")
GSCALE = {"normal": 1.0, "soft": 0.5}


def _inputs(B, C, variant):
    g = torch.Generator().manual_seed(1000 * B + C)
    z = torch.randn(B, C, generator=g)
    t = torch.eye(C)[torch.randint(0, C, (B,), generator=g)]
    if variant == "scale80":
        z = z * 80.0
    elif variant == "scale1e4":
        z = z * 1e4
    elif variant == "soft":
        t = torch.rand(B, C, generator=g) * torch.linspace(0.2, 1.7, B).reshape(B, 1)     # row sums are not 1
    elif variant == "zero_rows":
        t[::2] = 0.0
    elif variant == "ties":
        for b in range(B):
            top = z[b].max().item() + 1.0
            cols = [(3 * b) % C, (3 * b + 64) % C, (3 * b + 7) % C]       # same lane (j, j + 64) and another lane
            z[b, cols] = top
            tc = [(5 * b + 1) % C, (5 * b + 65) % C]
            t[b] = 0.25
            t[b, tc] = 0.75
    return z.contiguous(), t.contiguous()


_REF = {}


def reference(B, C, variant):
    key = (B, C, variant)
    if key not in _REF:
        z, t = _inputs(B, C, variant)
        gs = GSCALE.get(variant, 1.0)
        out = {}
        for name, dt in (("ref", torch.float64), ("f32", torch.float32)):
            zz = z.to(dt).requires_grad_(True)
            loss = F.cross_entropy(zz, t.to(dt))
            (grad,) = torch.autograd.grad(loss * gs, zz)
            out[name] = (loss.detach(), grad)
        pred = z.argmax(1)
        hits = int((pred == t.argmax(1)).sum())
        _REF[key] = (z, t, gs, out, pred, hits)
    return _REF[key]


def _check(label, got, ref, f32):
    got = got.detach().double().cpu()
    scale = ref.abs().max().item()
    e_dev = (got - ref).abs().max().item()
    e_cpu = (f32.double() - ref).abs().max().item()
    print(f"XENT {label} e_dev={e_dev:.3e} e_cpu={e_cpu:.3e} scale={scale:.3e}")
    assert e_dev == e_dev, f"{label}: NaN"
    assert e_dev <= RTOL * scale, f"{label}: max err {e_dev:.3e} vs {RTOL} * {scale:.3e}"
    assert e_dev <= YARD * e_cpu, f"{label}: max err {e_dev:.3e} > {YARD} * {e_cpu:.3e} (CPU fp32)"


@gpu
@pytest.mark.parametrize("B,C", SHAPES, ids=[f"B{b}-C{c}" for b, c in SHAPES])
def test_loss_gradient_prediction_and_hits(B, C):
    from ali_hip import ops
    acc = torch.zeros(1, dtype=torch.int64, device="cuda")
    want_acc = 0
    for variant in VARIANTS:
        z, t, gs, out, pred, hits = reference(B, C, variant)
        zd, td = z.cuda(), t.cuda()
        out2, gl, pd = ops.softmax_xent(zd, td, gscale=gs, want_pred=True, hits_accum=acc)
        again = ops.softmax_xent(zd, td, gscale=gs, want_pred=True, hits_accum=acc)
        want_acc += 2 * hits
        label = f"B={B} C={C} {variant}"
        _check(label + " loss", out2[0], out["ref"][0], out["f32"][0])
        _check(label + " grad", gl, out["ref"][1], out["f32"][1])
        assert torch.equal(pd.cpu().long(), pred), label
        assert out2[1].item() == float(hits), label
        assert acc.item() == want_acc, label                      # two successive calls each added their hits
        for a, b in zip((out2, gl, pd), again):                  # the same bits on every run
            assert torch.equal(a, b), label
        # without the optional outputs: the same loss and hit count
        bare, none_g, none_p = ops.softmax_xent(zd, td, gscale=gs, want_grad=False)
        assert none_g is None and none_p is None and torch.equal(bare, out2), label
    assert int(ops.workspace(torch.device("cuda"))[:4096].count_nonzero()) == 0      # the arrival counter is back at zero
