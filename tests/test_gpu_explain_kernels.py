"""The kernels of csrc/explain.hip, one by one, against this file's fp64 torch statements.

Values are held to the two bounds of test_gpu_xent.py's ``_check`` (at most YARD times the error of the same statement
in CPU fp32, and at most RTOL of max|ref64|).  Everything discrete -- which logit receives the hinge gradient, the
predictions, the order and the hit count of the selection, the step counters -- is compared exactly, at equal inputs.
``cf_join`` is one fp32 add of two given fp32 numbers and is compared exactly as well.  The Adam update is checked at the
device's own gradient and state against an fp64 statement of torch.optim.Adam with the bound test_gpu_classifiers.py
derives: 1e-6 * lr (the update's own rounding) + 6e-8 * max|w| (the fp32 spacing of the variable).
"""
import pytest
import torch

from test_gpu_xent import _check

gpu = pytest.mark.gpu


def _ops():
    from ali_hip import ops
    return ops


# ------------------------------------------------------------------------------------------------------ row_dist
@gpu
@pytest.mark.parametrize("N", [1, 63, 784, 4099])
@pytest.mark.parametrize("S", [1, 3, 100])
def test_row_dist(S, N):
    ops = _ops()
    g = torch.Generator().manual_seed(17 * S + N)
    y = torch.randn(S, N, generator=g)
    for broadcast in (True, False):
        x = torch.randn(1 if broadcast else S, N, generator=g)
        if N > 2:
            y[S // 2, 1] = x[0 if broadcast else S // 2, 1]            # a zero difference
        for mode, name in ((ops.DIST_L1, "l1"), (ops.DIST_L2, "l2")):
            def stmt(dt):
                d = y.to(dt) - x.to(dt)
                return (d.abs() if name == "l1" else d.square()).mean(dim=1)
            got = ops.row_dist(x.cuda(), y.cuda(), mode)
            again = ops.row_dist(x.cuda(), y.cuda(), mode)
            assert got.shape == (S,) and torch.equal(got, again)
            _check(f"row_dist S={S} N={N} bc={broadcast} {name}", got, stmt(torch.float64), stmt(torch.float32))


@gpu
def test_row_dist_image_shaped_rows_and_a_given_output():
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(1, 1, 28, 28, generator=g), torch.randn(5, 1, 28, 28, generator=g)
    out = torch.full((5,), -1.0, device="cuda")
    assert ops.row_dist(x.cuda(), y.cuda(), ops.DIST_L2, out=out) is out
    ref = (x.double() - y.double()).square().mean(dim=[1, 2, 3])
    _check("row_dist images", out, ref, (x - y).square().mean(dim=[1, 2, 3]))
    with pytest.raises(ValueError):
        ops.row_dist(torch.zeros(2, 784, device="cuda"), y.cuda())


# ------------------------------------------------------------------------------------------------------ cf_hinge
def _hinge_stmt(z, t, orig, m, c, dt):
    z = z.to(dt).requires_grad_(True)
    hs = []
    for b in range(z.shape[0]):
        if t[b] >= 0:
            best = None
            for i in range(z.shape[1]):                    # strict >: the first maximum
                if i != t[b] and (best is None or z[b, i].item() > best.item()):
                    best = z[b, i]
            hs.append(best - z[b, t[b]])
        else:
            hs.append((z[b] - orig[b].to(dt)).square().mean())
    h = torch.stack(hs)
    (grad,) = torch.autograd.grad((c * h).sum(), z)
    return torch.stack([c * h + m.to(dt), h, m.to(dt)], dim=1).detach(), grad


@gpu
@pytest.mark.parametrize("C", [2, 3, 10, 65])
@pytest.mark.parametrize("B", [1, 5])
def test_cf_hinge(B, C):
    ops = _ops()
    g = torch.Generator().manual_seed(100 * B + C)
    c = 10.0
    for variant in ("first", "last", "middle", "tie", "no_target", "mixed"):
        z = torch.randn(B, C, generator=g)
        m = torch.rand(B, generator=g)
        orig = torch.softmax(torch.randn(B, C, generator=g), dim=1)
        t = {"first": [0] * B, "last": [C - 1] * B, "middle": [C // 2] * B, "tie": [(b + 1) % C for b in range(B)],
             "no_target": [-1] * B, "mixed": [(-1 if b % 2 else b % C) for b in range(B)]}[variant]
        if variant == "tie" and C >= 3:
            for b in range(B):
                cols = [j for j in range(C) if j != t[b]][:2]
                if C == 65 and b == 0:
                    cols = [0, 64]                          # one lane's columns (j and j + 64)
                z[b, cols] = z[b].max().item() + 1.0        # the two largest other logits are equal
        tt = torch.tensor(t, dtype=torch.int32)
        out, gl = ops.cf_hinge(z.cuda(), tt.cuda(), m.cuda(), c, orig_pred=orig.cuda())
        ref, gref = _hinge_stmt(z, t, orig, m, c, torch.float64)
        f32, g32 = _hinge_stmt(z, t, orig, m, c, torch.float32)
        label = f"cf_hinge B={B} C={C} {variant}"
        assert torch.equal(gl.cpu() != 0, gref != 0), label          # where the gradient lands: exact
        assert torch.equal(gl.cpu().sign(), gref.sign().float()), label
        _check(label + " out", out, ref, f32)
        _check(label + " grad", gl, gref, g32)
        if variant == "tie" and C >= 3:
            for b in range(B):
                others = [j for j in range(C) if j != t[b]]
                top = max(z[b, j].item() for j in others)
                first = min(j for j in others if z[b, j].item() == top)
                assert gl[b, first].item() == c and gl[b, t[b]].item() == -c and int((gl[b] != 0).sum()) == 2
        out2, none = ops.cf_hinge(z.cuda(), tt.cuda(), m.cuda(), c, orig_pred=orig.cuda(), want_grad=False)
        assert none is None and torch.equal(out2, out)


# ------------------------------------------------------------------------------------------------------- cf_join
@gpu
@pytest.mark.parametrize("N", [6, 784])
@pytest.mark.parametrize("B,xB", [(1, 1), (3, 3), (3, 1)])
def test_cf_join_is_the_fp32_statement(B, xB, N):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 1000 + N + xB)
    gx = torch.randn(B, N, 4, generator=g) * 1e-2
    x = torch.randn(xB, N, generator=g)
    x_cf = torch.randn(B, N, generator=g)
    x_cf[:, ::3] = x.expand(B, N)[:, ::3]                       # equal entries: the L1 term's gradient is 0 there
    xc = x_cf.clone().requires_grad_(True)
    (x.expand(B, N) - xc).abs().reshape(B, -1).mean(dim=1).sum().backward()
    want = gx[..., 0] + xc.grad
    assert int((xc.grad == 0).sum()) >= B * (N // 3)
    got = ops.cf_join(gx.reshape(B, N, 1, 4).cuda(), x_cf.cuda(), x.cuda())
    assert got.shape == (B, N) and torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------- cf_input_fwd / cf_input_step
def _layout(name):
    """(segments, table widths, n_log): kind, width, src_off, dst_off, table, attr_off"""
    ops = _ops()
    if name == "mnist":            # z 512 trained, digit softmax into a table, three continuous of which two are ignored
        segs = [(ops.CF_SOFTMAX, 10, 0, 512, 0, 0), (ops.CF_COPY, 1, 0, 768, -1, 10), (ops.CF_TANH, 1, 10, 769, -1, 11),
                (ops.CF_COPY, 1, 1, 770, -1, 12), (ops.CF_TANH, 512, 11, 0, -1, -1)]
        return segs, [10], 771
    if name == "audio":            # six categoricals of differing widths, one of them given, z trained
        widths = [10, 60, 2, 5, 7, 3]
        segs, raw, attr = [], 0, 0
        for j, w in enumerate(widths):
            if j == 3:
                segs.append((ops.CF_COPY, w, 0, 512 + 256 * j, j, attr))
            else:
                segs.append(((ops.CF_TANH if j == 4 else ops.CF_SOFTMAX), w, raw, 512 + 256 * j, j, attr))
                raw += w
            attr += w
        segs.append((ops.CF_TANH, 512, raw, 0, -1, -1))
        return segs, widths, 512 + 256 * 6
    # the encoder's codes are copied, no continuous attribute is trained
    segs = [(ops.CF_SOFTMAX, 10, 0, 512, 0, 0), (ops.CF_COPY, 1, 512, 768, -1, 10), (ops.CF_COPY, 512, 0, 0, -1, -1)]
    return segs, [10], 769


def _input_stmt(segs, tables, n_log, ld, raw, given, dt):
    ops = _ops()
    B = raw.shape[0]
    attrs = {}
    cols = []
    for kind, w, src, dst, tab, aoff in segs:
        v = (given if kind == ops.CF_COPY else raw)[:, src:src + w]
        v = v.tanh() if kind == ops.CF_TANH else (v.softmax(1) if kind == ops.CF_SOFTMAX else v)
        if aoff >= 0:
            attrs[aoff] = v
        out = v.matmul(tables[tab].to(dt)) if tab >= 0 else v
        cols.append((dst, out))
    parts = sorted(cols, key=lambda c: c[0])
    row = torch.cat([p for _, p in parts] + [torch.zeros(B, ld - n_log, dtype=dt)], dim=1)
    a = torch.cat([attrs[k] for k in sorted(attrs)], dim=1)
    return row, a


def _adam_stmt(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / (1 - b2 ** t) ** 0.5 + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v


@gpu
@pytest.mark.parametrize("name", ["mnist", "audio", "codes"])
@pytest.mark.parametrize("B", [1, 3])
def test_cf_input_fwd_and_step(name, B):
    ops = _ops()
    segs, widths, n_log = _layout(name)
    ld = n_log + (-n_log) % 32
    g = torch.Generator().manual_seed(7 * B + len(segs))
    tables = [torch.randn(w, 256, generator=g) for w in widths]
    lay = ops.CfLayout(segs, [t.cuda() for t in tables], n_log, ld)
    raw = torch.randn(B, lay.raw_ld, generator=g)
    given = torch.randn(B, lay.given_ld, generator=g) if lay.given_ld else None
    cot = torch.randn(B, ld, generator=g)
    lr = 0.1
    trained = torch.zeros(lay.raw_ld, dtype=torch.bool)
    for kind, w, src, *_ in segs:
        if kind != ops.CF_COPY:
            trained[src:src + w] = True
    assert bool(trained.all())

    def stmt(dt):
        r = raw.to(dt).requires_grad_(True)
        row, a = _input_stmt(segs, tables, n_log, ld, r, None if given is None else given.to(dt), dt)
        (gr,) = torch.autograd.grad((row * cot.to(dt)).sum(), r)
        return row.detach(), a.detach(), gr
    row64, a64, g64 = stmt(torch.float64)
    row32, a32, g32 = stmt(torch.float32)

    d_raw = raw.cuda()
    d_given = None if given is None else given.cuda()
    rows, attrs = ops.cf_input_fwd(lay, d_raw, d_given)
    label = f"cf_input {name} B={B}"
    assert rows.shape == (B, ld) and attrs.shape == (B, lay.attrs_ld)
    assert bool((rows[:, n_log:] == 0).all())
    _check(label + " rows", rows, row64, row32)
    _check(label + " attrs", attrs, a64, a32)
    for kind, w, src, dst, tab, aoff in segs:                 # what is given is copied, not recomputed
        if kind == ops.CF_COPY and tab < 0:
            assert torch.equal(rows[:, dst:dst + w].cpu(), given[:, src:src + w])

    m, v = torch.zeros_like(d_raw), torch.zeros_like(d_raw)
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    graw = torch.zeros_like(d_raw)
    state = (raw.double(), torch.zeros(B, lay.raw_ld, dtype=torch.float64), torch.zeros(B, lay.raw_ld, dtype=torch.float64))
    for t in (1, 2):                                          # the second step pins the counter and the moments
        if t == 2:
            rows, attrs = ops.cf_input_fwd(lay, d_raw, d_given)
        ops.cf_input_step(lay, cot.cuda(), rows, attrs, d_raw, m, v, step, lr, graw=graw)
        if t == 1:
            _check(label + " grad", graw, g64, g32)
        assert step.tolist() == [t] * B
        want_p, want_m, want_v = _adam_stmt(state[0], graw.double().cpu(), state[1], state[2], t, lr)
        err = (d_raw.double().cpu() - want_p).abs().max().item()
        bound = 1e-6 * lr + 6e-8 * state[0].abs().max().item()
        print(f"CFIN {label} step {t} update err={err:.3e} bound={bound:.3e}")
        assert err <= bound, (label, t, err, bound)
        assert (m.double().cpu() - want_m).abs().max().item() <= 6e-8 * want_m.abs().max().item() + 1e-30
        assert (v.double().cpu() - want_v).abs().max().item() <= 6e-8 * want_v.abs().max().item() + 1e-30
        if t == 1:
            assert bool((d_raw.cpu() != raw).all())
        state = (d_raw.double().cpu(), m.double().cpu(), v.double().cpu())


@gpu
def test_cf_input_rows_keep_their_own_step_counters():
    """a row that has taken more steps than its neighbour gets its own bias correction"""
    ops = _ops()
    segs = [(ops.CF_TANH, 4, 0, 0, -1, 0)]
    lay = ops.CfLayout(segs, [], 4, 32)
    raw = torch.tensor([[0.1, -0.2, 0.3, 0.4]] * 2, device="cuda")
    m, v = torch.zeros_like(raw), torch.zeros_like(raw)
    step = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
    rows, attrs = ops.cf_input_fwd(lay, raw, None)
    cot = torch.ones(2, 32, device="cuda")
    before = raw.double().cpu()
    graw = torch.zeros_like(raw)
    ops.cf_input_step(lay, cot, rows, attrs, raw, m, v, step, 0.01, graw=graw)
    assert step.tolist() == [1, 6]
    for b, t in ((0, 1), (1, 6)):
        z = torch.zeros(4, dtype=torch.float64)
        want, _, _ = _adam_stmt(before[b], graw[b].double().cpu(), z, z, t, 0.01)
        assert (raw[b].double().cpu() - want).abs().max().item() <= 1e-6 * 0.01 + 6e-8 * 0.4


# ----------------------------------------------------------------------------------------------------- cf_select
def _select_stmt(logit, metric, target):
    pred = logit.argmax(1)
    hit = pred == target
    rows = torch.arange(logit.shape[0])
    hits = rows[hit][metric[hit].argsort(stable=True)]
    return pred.int(), torch.cat([hits, rows[~hit]]).int(), int(hit.sum())


@gpu
@pytest.mark.parametrize("S", [1, 2, 64, 100, 1024])
def test_cf_select(S):
    ops = _ops()
    C, target = 10, 4
    g = torch.Generator().manual_seed(S)
    for variant in ("all", "none", "mixed", "duplicates", "logit_ties", "nan_metric"):
        logit = torch.randn(S, C, generator=g)
        metric = torch.rand(S, generator=g)
        if variant == "all":
            logit[:, target] = 9.0
        elif variant == "none":
            logit[:, target] = -9.0
        else:
            logit[::2, target] = 9.0
        if variant == "duplicates":
            metric = (metric * 4).floor() / 4                  # many equal values: row order decides
        if variant == "logit_ties" and S > 1:
            logit[::2, target + 1] = 9.0                       # the first maximum is the target ...
            logit[1::4, target - 1] = logit[1::4].max().item() + 1.0
            logit[1::4, target] = logit[1::4, target - 1]      # ... and here it is not
        if variant == "nan_metric" and S > 2:
            metric[::3] = float("nan")                         # behind every number, in row order
        tt = torch.tensor([target], dtype=torch.int32, device="cuda")
        pred, order, n_hit = ops.cf_select(logit.cuda(), metric.cuda(), tt)
        want_pred, want_order, want_n = _select_stmt(logit, metric, target)
        label = f"cf_select S={S} {variant}"
        assert torch.equal(pred.cpu(), want_pred), label
        assert int(n_hit.item()) == want_n, label
        assert torch.equal(order.cpu(), want_order), label
        assert sorted(order.tolist()) == list(range(S)), label
