"""GPU parity of the small kernels around the GEMMs (conditioning, loss, Adam, Dropout2d masks, counters, spectrogram
tail, conditioning planes), called through the ``ali_hip.ops`` wrappers the way the product calls them, against plain
float64 restatements on the CPU.

Rules:
- data movement and single fp32 multiplies are compared exactly (``torch.equal``);
- sums are held to an element-wise bound set by the length of the summation (the classic
  ``|fl(sum) - sum| <= n * 2^-24 * sum |terms|``), never to a tolerance relative to the tensor's maximum.  Every such
  test also asserts, on the CPU, that the reference with one sample dropped (or one class term doubled) violates the
  bound: the tolerance can fail;
- batches around one 256-thread block (1, 255, 256, 257) and sizes above the element-wise grid cap (2048 blocks x 256
  threads, x4 for Adam) that force the grid-stride loops."""
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # unit round-off of fp32
EW_CAP = 2048 * 256                 # elements one pass of a capped element-wise grid covers (ew_grid)
EDGE_B = (1, 255, 256, 257)


def _ops():
    from ali_hip import ops
    return ops


def _dev():
    return torch.device("cuda")


def assert_within(got, ref, bound, buggy, what):
    """|got - ref| <= bound element-wise; and the planted-bug reference ``buggy`` must violate the same bound somewhere
    (checked first, on the CPU: a bound that no plausible bug can break proves nothing)."""
    ref, bound, buggy = ref.double(), bound.double(), buggy.double()
    assert ((buggy - ref).abs() > bound).any(), f"{what}: the bound does not tell the planted bug apart"
    err = (got.detach().double().cpu() - ref).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} entries out of bound; worst excess "
                           f"{(err - bound).max().item():.3e}")


def _attr_rows(g, B, n, kind):
    """[B, n] categorical attribute rows.  hot / int: exact one-hots (fp32 / int32, whalecalls' int32 one-hots);
    soft: random fp32 rows with planted ties (two equal maxima), an all-zero row and all-negative rows;
    int_soft: int32 rows in [-2, 2] (ties everywhere); prob: non-negative soft rows with zeros (soft attributes)."""
    if kind in ("hot", "int"):
        t = F.one_hot(torch.randint(0, n, (B,), generator=g), n)
        return t.to(torch.int32) if kind == "int" else t.float()
    if kind == "int_soft":
        return torch.randint(-2, 3, (B, n), generator=g).to(torch.int32)
    if kind == "prob":
        t = torch.rand(B, n, generator=g) * (torch.rand(B, n, generator=g) > 0.3).float()
        t[torch.arange(B), torch.randint(0, n, (B,), generator=g)] += 0.5        # no all-zero row
        return t
    t = torch.randn(B, n, generator=g)
    if n >= 2:
        for r in range(0, B, 7):             # two equal maxima, the second one later in the row
            a, b = sorted(torch.randperm(n, generator=g)[:2].tolist())
            t[r, a] = t[r, b] = t[r].max() + 1.0
        t[3::11] = 0.0                        # all-zero rows: index 0
        t[5::13] = -t[5::13].abs() - 0.5      # all negative
    return t


# ---------------------------------------------------------------------------------------------- attr_pack (exact)
ATTR_CFG = [(1, 0, ("hot",)), (1, 1, ("int",)), (3, 2, ("hot", "int", "soft")), (3, 4, ("soft", "int_soft", "hot")),
            (8, 3, ("hot", "int", "soft", "int_soft", "hot", "soft", "int", "hot"))]


@pytest.mark.parametrize("B", EDGE_B + (1030,))
@pytest.mark.parametrize("n_cat,n_cont,kinds", ATTR_CFG, ids=[f"cat{c[0]}_cont{c[1]}" for c in ATTR_CFG])
def test_attr_pack_argmax_and_continuous(B, n_cat, n_cont, kinds):
    """idx == CPU torch.argmax (first maximum: ties, all-zero rows, negatives); cont == the continuous attributes, given
    as [B] and as [B,1]."""
    ops = _ops()
    g = torch.Generator().manual_seed(B * 31 + n_cat * 7 + n_cont)
    ncls = [(2, 10, 33, 3, 17, 5, 8, 2)[j] for j in range(n_cat)]
    cats = [_attr_rows(g, B, n, k) for n, k in zip(ncls, kinds)]
    conts = [torch.randn((B,) if j % 2 == 0 else (B, 1), generator=g) for j in range(n_cont)]
    idx, cont = ops.attr_pack([c.to(_dev()) for c in cats], [c.to(_dev()) for c in conts], B, _dev())
    ref = torch.stack([torch.argmax(c.double(), dim=1) for c in cats], dim=1).to(torch.int32)
    assert torch.equal(idx.cpu(), ref)
    if n_cont:
        assert torch.equal(cont.cpu(), torch.stack([c.reshape(B) for c in conts], dim=1))
    else:
        assert cont is None


def test_attr_pack_rejects_too_many_attributes():
    """the kernel's argument block holds 8 categorical and 4 continuous attributes: more must raise, not overflow"""
    ops = _ops()
    B = 4
    oh = torch.eye(3, device=_dev())[torch.tensor([0, 1, 2, 0])].contiguous()
    c = torch.randn(B, device=_dev())
    with pytest.raises(RuntimeError, match="ali_attr_pack"):
        ops.attr_pack([oh] * 9, [], B, _dev())
    with pytest.raises(RuntimeError, match="ali_attr_pack"):
        ops.attr_pack([oh], [c] * 5, B, _dev())
    idx, cont = ops.attr_pack([oh] * 8, [c] * 4, B, _dev())          # the limits themselves are accepted
    assert torch.equal(idx.cpu(), torch.tensor([0, 1, 2, 0], dtype=torch.int32)[:, None].repeat(1, 8))
    assert torch.equal(cont.cpu(), c.cpu()[:, None].repeat(1, 4))


# ---------------------------------------------------------------------------------------------- g_input
GIN_CFG = [(512, 1, 3, "hot"), (512, 1, 1, "int"), (512, 3, 0, "int"), (512, 8, 2, "prob"), (512, 3, 1, "soft"),
           (37, 1, 2, "prob")]


@pytest.mark.parametrize("B", EDGE_B)
@pytest.mark.parametrize("extra_ld", [0, 64])
@pytest.mark.parametrize("zdim,n_emb,n_cont,kind", GIN_CFG, ids=[f"z{c[0]}_t{c[1]}_c{c[2]}_{c[3]}" for c in GIN_CFG])
def test_g_input_rows(B, extra_ld, zdim, n_emb, n_cont, kind):
    """[z | onehot_j @ T_j ... | cont | 0] vs torch.cat of the float64 products (mnist.py:96: onehot.matmul(weight)).
    z, cont, exact one-hot rows and the padding up to ``ld`` are exact; soft rows are a sum over the classes."""
    ops = _ops()
    g = torch.Generator().manual_seed(B + 97 * n_emb + n_cont + extra_ld + zdim)
    ncls = [(10, 2, 33, 5, 10, 3, 17, 4)[j] for j in range(n_emb)]
    n_log = zdim + 256 * n_emb + n_cont
    ld = n_log + (-n_log) % 32 + extra_ld
    z = torch.randn(B, zdim, generator=g)
    ohs = [_attr_rows(g, B, n, kind) for n in ncls]
    tabs = [torch.randn(n, 256, generator=g) for n in ncls]
    cont = torch.randn(B, n_cont, generator=g) if n_cont else None
    out = torch.full((B, ld), float("nan"), device=_dev())
    ops.g_input(z.to(_dev()), [o.to(_dev()) for o in ohs], [t.to(_dev()) for t in tabs],
                None if cont is None else cont.to(_dev()), ld, out=out)
    got = out.cpu()
    assert torch.equal(got[:, :zdim], z)
    if n_cont:
        assert torch.equal(got[:, zdim + 256 * n_emb:n_log], cont)
    assert torch.equal(got[:, n_log:], torch.zeros(B, ld - n_log))
    for j, (oh, T) in enumerate(zip(ohs, tabs)):
        part = got[:, zdim + 256 * j:zdim + 256 * (j + 1)]
        ref = oh.double() @ T.double()
        if kind in ("hot", "int"):
            assert torch.equal(part, ref.float()), f"table {j}: one-hot rows must be copied exactly"
            continue
        # sum over n classes: n products + n - 1 additions in fp32
        bound = (ncls[j] + 1) * U * (oh.double().abs() @ T.double().abs())
        k = int(torch.argmax(oh.double().abs().sum(0)))
        buggy = ref + oh[:, k:k + 1].double() * T[k:k + 1].double()       # one class term counted twice
        assert_within(part, ref, bound, buggy, f"table {j}")


# ---------------------------------------------------------------------------------------------- g_input_table_grad
@pytest.mark.parametrize("B", (1, 15, 16, 17, 512, 1024))
@pytest.mark.parametrize("ncls", (1, 2, 10, 33))
@pytest.mark.parametrize("kind", ("hot", "int", "prob"))
def test_g_input_table_grad(B, ncls, kind):
    """out = onehot^T @ g[:, off:off+256] of the second table of a real gin layout (z 512 | 2 tables | 1 cont, stride
    rounded to 32), vs float64; two launches bitwise equal (fixed order, no atomics)."""
    ops = _ops()
    g = torch.Generator().manual_seed(B * 7 + ncls + len(kind))
    n_log = 512 + 2 * 256 + 1
    ld = n_log + (-n_log) % 32
    off = 512 + 256
    oh = _attr_rows(g, B, ncls, kind)
    gg = torch.randn(B, ld, generator=g)
    out = torch.full((ncls, 256), float("nan"), device=_dev())
    ohd, gd = oh.to(_dev()), gg.to(_dev())
    ops.g_input_table_grad(ohd, gd, off, out)
    again = torch.full_like(out, float("nan"))
    ops.g_input_table_grad(ohd, gd, off, again)
    assert torch.equal(out, again)
    a, b = oh.double(), gg[:, off:off + 256].double()
    ref = a.t() @ b
    bound = (B + 1) * U * (a.abs().t() @ b.abs())
    # one sample dropped: the heaviest sample of the attribute
    s = int(torch.argmax(a.abs().sum(1)))
    buggy = ref - a[s:s + 1].t() @ b[s:s + 1]
    assert_within(out, ref, bound, buggy, "table grad")


# ---------------------------------------------------------------------------------------------- BCE with logits
PLANTED = (0.0, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)


def _logits(g, n):
    x = torch.randn(n, 1, generator=g) * 3
    if n > len(PLANTED):                   # sample 0 stays a drawn one (the one the bug checks drop)
        pos = torch.randperm(n - 1, generator=g)[:len(PLANTED)] + 1
        x[pos, 0] = torch.tensor(PLANTED)
    return x


def _bce_terms(x, t):
    """float64 per-sample BCE of the fp32 logits and the |terms| of the fp32 formula (for the rounding bound)"""
    xd = x.double().reshape(-1)
    td = torch.full_like(xd, float(torch.tensor(t, dtype=torch.float32)))   # the kernel's target is an fp32 value
    loss = F.binary_cross_entropy_with_logits(xd, td, reduction="none")
    mag = xd.clamp(min=0) + (xd * td).abs() + torch.log1p(torch.exp(-xd.abs()))
    return loss, mag, td


def _median_index(v):
    return int(torch.argsort(v)[(v.numel() - 1) // 2])


def _check_mean(got, terms, mag, what):
    """mean of B fp32 terms summed in double: per-term fp32 error <= 4 u |term|, the double sum adds B * 2^-53,
    the final fp32 rounding u |mean|"""
    B = terms.numel()
    ref = terms.mean()
    bound = (4 + 2 + B * 2.0 ** -29) * U * mag.mean()
    s = _median_index(terms)
    buggy = (terms.sum() - terms[s]) / B                                        # one sample dropped from the sum
    assert_within(torch.tensor(got), ref, bound.reshape(()), buggy, what)


def _check_grad(gl, x, t_of_row, gscale, B):
    """gradient vs float64 autograd of ``gscale * sum of the per-pass means``: gscale * (sigmoid - t) / B, with
    an absolute bound of a few u * gscale / B (sigmoid ~3 ulp, the subtraction, the division)"""
    xr = x.double().reshape(-1).clone().requires_grad_(True)
    loss = gscale * F.binary_cross_entropy_with_logits(xr, t_of_row, reduction="sum") / B
    loss.backward()
    ref = xr.grad
    bound = torch.full_like(ref, 8 * U * gscale / B)
    buggy = ref.clone()
    buggy[0] = 0.0                                                               # sample 0 dropped from the loss
    assert_within(gl.reshape(-1), ref, bound, buggy, "bce grad")


@pytest.mark.parametrize("B", EDGE_B + (512, 1000, 4096))
@pytest.mark.parametrize("ta,tb", [(0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (0.3, 0.3)])
@pytest.mark.parametrize("gscale", [0.5, 0.5 * 1024])
def test_bce_logits_pair(B, ta, tb, gscale):
    """out3 = [(loss_a + loss_b)/2, mean sigmoid(a), mean sigmoid(b)] vs float64 binary_cross_entropy_with_logits /
    sigmoid().mean(); glogit = gscale * (sigmoid - t) / B (the stepper passes 0.5 * loss scale: d of the halved sum)."""
    ops = _ops()
    g = torch.Generator().manual_seed(B + int(10 * ta) + 3 * int(tb) + int(gscale))
    x = _logits(g, 2 * B)
    out3, gl = ops.bce_logits_pair(x.to(_dev()), B, ta, tb, gscale)
    out3n, gln = ops.bce_logits_pair(x.to(_dev()), B, ta, tb, gscale, want_grad=False)
    assert gln is None and torch.equal(out3n, out3)
    got = out3.cpu().double()
    la, ma, tda = _bce_terms(x[:B], ta)
    lb, mb, tdb = _bce_terms(x[B:], tb)
    # (mean_a + mean_b) / 2: the bound of each mean, halved, plus the two fp32 roundings of the combination
    ref = (la.mean() + lb.mean()) / 2
    bound = ((6 + B * 2.0 ** -29) * U * (ma.mean() + mb.mean()) / 2 + 2 * U * ref.abs()).reshape(())
    s = _median_index(la)
    buggy = ((la.sum() - la[s]) / B + lb.mean()) / 2
    assert_within(got[0], ref, bound, buggy, "pair loss")
    for k, xs in ((1, x[:B]), (2, x[B:])):
        sg = torch.sigmoid(xs.double().reshape(-1))
        _check_mean(got[k].item(), sg, sg, f"mean sigmoid {k}")
    _check_grad(gl, x, torch.cat([tda, tdb]), gscale, B)


@pytest.mark.parametrize("B", EDGE_B + (512, 1000, 4096))
@pytest.mark.parametrize("t", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("gscale", [1.0, 1024.0])
def test_bce_logits(B, t, gscale):
    ops = _ops()
    g = torch.Generator().manual_seed(B * 3 + int(10 * t) + int(gscale))
    x = _logits(g, B)
    out2, gl = ops.bce_logits(x.to(_dev()), t, gscale)
    out2n, gln = ops.bce_logits(x.to(_dev()), t, gscale, want_grad=False)
    assert gln is None and torch.equal(out2n, out2)
    got = out2.cpu().double()
    loss, mag, td = _bce_terms(x, t)
    _check_mean(got[0].item(), loss, mag, "loss")
    sg = torch.sigmoid(x.double().reshape(-1))
    _check_mean(got[1].item(), sg, sg, "mean sigmoid")
    _check_grad(gl, x, td, gscale, B)


# ---------------------------------------------------------------------------------------------- Adam
LR, BETAS, EPS = 1e-4, (0.5, 0.999), 1e-8      # mnist.py:176-179


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


class _AdamF64:
    """float64 restatement of torch.optim.Adam (no amsgrad / decay) with the hyper-parameters rounded to fp32, as the
    C ABI receives them.  Keeps, per element, the rounding bound of the fp32 kernel: per step u |p| for the update's
    rounding into p, 8 t u |m| / denom for the (cancelling) moving average m, 32 u |update| for v, sqrt, the divisions
    and the bias corrections."""

    def __init__(self, p, lr=LR, betas=BETAS, eps=EPS, step_shift=0):
        self.p = p.double().clone()
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.lr, self.b1, self.b2, self.eps = _f32(lr), _f32(betas[0]), _f32(betas[1]), _f32(eps)
        self.t, self.shift = 0, step_shift
        self.m_abs = torch.zeros_like(self.p)
        self.bound = torch.zeros_like(self.p)

    def step(self, grad):
        self.t += 1
        t = self.t + self.shift
        g = grad.double()
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.m_abs = self.b1 * self.m_abs + (1 - self.b1) * g.abs()
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        step_size = self.lr / (1 - self.b1 ** t)
        denom = self.v.sqrt() / (1 - self.b2 ** t) ** 0.5 + self.eps
        upd = step_size * self.m / denom
        self.p = self.p - upd
        # m may cancel: its fp32 error (2 u per step) is relative to the magnitudes it was summed from (m_abs)
        self.bound = self.bound + U * self.p.abs() + step_size * (8 * self.t * U) * self.m_abs / denom + 32 * U * upd.abs()


def _torch_adam(p):
    pr = torch.nn.Parameter(p.clone())
    return pr, torch.optim.Adam([pr], lr=LR, betas=BETAS, eps=EPS, foreach=False)


@pytest.mark.parametrize("n", [1, 1023, 10007, 3 << 20])
@pytest.mark.parametrize("mode,grad_scale", [("host", 1.0), ("dev_step", 0.5), ("arrive", 0.125), ("arrive", 1.0)])
def test_adam_step_conventions(n, mode, grad_scale):
    """ali_adam in the three step conventions of include/ali_hip.h, with grad_scale and the fp16 twin, vs a float64
    restatement (element-wise bound) and torch.optim.Adam(foreach=False) in fp32 (the 1e-7 bar of
    test_gpu_kernels.py).  |p| ~ 0.01 keeps one fp32 ulp of p far below 1e-7; at n = 3 * 2^20 the capped grid (2048
    blocks) strides and 2048 blocks arrive."""
    ops = _ops()
    g = torch.Generator().manual_seed(n + int(8 * grad_scale) + len(mode))
    p = torch.randn(n, generator=g) * 0.01
    ref, off_by_one = _AdamF64(p), _AdamF64(p, step_shift=1)
    pr, opt = _torch_adam(p)
    pd, m, v = p.to(_dev()), torch.zeros(n, device=_dev()), torch.zeros(n, device=_dev())
    p16 = torch.empty(n, dtype=torch.float16, device=_dev())
    dev_step = torch.zeros(1, dtype=torch.int32, device=_dev())
    arrive = torch.zeros(1, dtype=torch.int32, device=_dev())
    steps = 3
    for k in range(1, steps + 1):
        gr = torch.randn(n, generator=g)
        gs = gr * grad_scale                           # exact: power-of-two scales
        ref.step(gs)
        off_by_one.step(gs)
        pr.grad = gs.clone()
        opt.step()
        if mode == "host":
            ops.adam(pd, gr.to(_dev()), m, v, LR, *BETAS, EPS, k, grad_scale=grad_scale, p16=p16)
        elif mode == "dev_step":                       # the device scalar holds the 1-based number of this step
            dev_step.fill_(k)
            ops.adam(pd, gr.to(_dev()), m, v, LR, *BETAS, EPS, 0, dev_step=dev_step, grad_scale=grad_scale, p16=p16)
            assert dev_step.item() == k
        else:                                          # the device scalar counts completed steps, the launch advances it
            ops.adam(pd, gr.to(_dev()), m, v, LR, *BETAS, EPS, 0, dev_step=dev_step, grad_scale=grad_scale,
                     arrive=arrive, p16=p16)
            assert dev_step.item() == k and arrive.item() == 0
    got = pd.cpu()
    assert_within(got, ref.p, ref.bound, off_by_one.p, f"adam {mode}")
    assert (got - pr.detach()).abs().max().item() < 1e-7
    assert torch.equal(p16, pd.half()), "p16 must be the fp16 rounding of the updated parameters"


def test_adam_arrive_in_a_captured_graph():
    """One ``arrive`` launch captured on a single stream and replayed 3 times: each replay advances dev_step by exactly
    one and leaves ``arrive`` at zero; the weights equal three torch.optim.Adam steps (a new gradient before each)."""
    ops = _ops()
    n = 3 << 20
    g = torch.Generator().manual_seed(5)
    p = torch.randn(n, generator=g) * 0.01
    ref = _AdamF64(p)
    pr, opt = _torch_adam(p)
    pd, m, v = p.to(_dev()), torch.zeros(n, device=_dev()), torch.zeros(n, device=_dev())
    gd = torch.zeros(n, device=_dev())
    p16 = torch.empty(n, dtype=torch.float16, device=_dev())
    dev_step = torch.zeros(1, dtype=torch.int32, device=_dev())
    arrive = torch.zeros(1, dtype=torch.int32, device=_dev())
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        ops.adam(pd, gd, m, v, LR, *BETAS, EPS, 0, dev_step=dev_step, arrive=arrive, p16=p16)
    torch.cuda.synchronize()
    # capture does not run the launch: the state is still that of zero completed steps
    assert dev_step.item() == 0 and arrive.item() == 0 and torch.equal(pd.cpu(), p)
    for k in range(1, 4):
        gr = torch.randn(n, generator=g)
        gd.copy_(gr)
        graph.replay()
        torch.cuda.synchronize()
        assert dev_step.item() == k and arrive.item() == 0, (k, dev_step.item(), arrive.item())
        ref.step(gr)
        pr.grad = gr.clone()
        opt.step()
    got = pd.cpu()
    off_by_one = _AdamF64(p, step_shift=1)
    g2 = torch.Generator().manual_seed(5)
    torch.randn(n, generator=g2)
    for _ in range(3):
        off_by_one.step(torch.randn(n, generator=g2))
    assert_within(got, ref.p, ref.bound, off_by_one.p, "adam graph replays")
    assert (got - pr.detach()).abs().max().item() < 1e-7
    assert torch.equal(p16, pd.half())
    del graph


# ---------------------------------------------------------------------------------------------- counters
def test_add_i64_multi_sums_duplicate_counters():
    """A counter named twice in one call (inside one chunk of 16 jobs, and across chunks) receives every increment."""
    ops = _ops()
    buf = torch.tensor([5, 1 << 40, -3, 0], dtype=torch.int64, device=_dev())
    cs = [buf[i:i + 1] for i in range(4)]
    ops.add_i64_multi([cs[0], cs[1], cs[0], cs[2], cs[0]], [1, 2, 3, 4, 5])
    assert buf.cpu().tolist() == [5 + 9, (1 << 40) + 2, -3 + 4, 0]
    # 40 jobs: three launches of <= 16, every counter in every chunk, some twice in a row
    jobs = [cs[(i * 7) % 4] if i % 5 else cs[3] for i in range(40)]
    incs = [(i + 1) * (1 if i % 3 else 1 << 33) for i in range(40)]
    expect = buf.cpu().tolist()
    for c, k in zip(jobs, incs):
        expect[cs.index(c)] += k
    ops.add_i64_multi(jobs, incs)
    assert buf.cpu().tolist() == expect


# ---------------------------------------------------------------------------------------------- Dropout2d masks
def _inv(p):
    one = torch.tensor(1.0)
    return one / (one - torch.tensor(p, dtype=torch.float32))     # the kernel's fp32 1 / (1 - p)


def _pad_cols(m, cpad):
    out = torch.ones(m.shape[0], cpad, device=m.device)
    out[:, :m.shape[1]] = m
    return out


SEGS = [(6, 5, 8, 0.2), (6, 5, 8, 0.2), (7, 1, 4, 0.5), (9, 3, 4, 0.9), (33, 64, 64, 0.0), (512, 32, 32, 0.2),
        (2, 1024, 1024, 0.5), (160, 1024, 1024, 0.2), (70000, 3, 4, 0.5), (257, 1, 1, 0.9)]


@pytest.mark.parametrize("counter", [None, 0, 1, 1 << 33])
def test_dropout_mask_multi_equals_one_launch_per_segment(counter):
    """ali_dropout_mask_multi == one ali_dropout_mask per segment at offset = cumulative logical draws, laid out into
    cpad columns; padding exactly 1; values exactly {0, fp32 1/(1-p)}; keep fraction within 5 sigma of 1 - p;
    adjacent identical segments draw different masks.  Segments longer than 128 x 1024 elements make the capped grid
    stride."""
    ops = _ops()
    seed = 0x5EED
    ctr = None if counter is None else torch.tensor([counter], dtype=torch.int64, device=_dev())
    ends, off = [], 0
    for B, cl, cp, _ in SEGS:
        off += B * cp
        ends.append(off)
    out = torch.full((off,), float("nan"), device=_dev())
    ops.dropout_mask_multi(seed, ctr, ends, [s[3] for s in SEGS], [s[1] for s in SEGS], [s[2] for s in SEGS], out)
    draws, lo, masks = 0, 0, []
    for (B, cl, cp, p), hi in zip(SEGS, ends):
        got = out[lo:hi].view(B, cp)
        one = ops.dropout_mask(seed, draws, p, B, cl, _dev(), ctr)
        assert torch.equal(got, _pad_cols(one, cp)), (B, cl, cp, p)
        logical = got[:, :cl].cpu()
        assert torch.equal(got[:, cl:].cpu(), torch.ones(B, cp - cl))
        if p == 0.0:
            assert torch.equal(logical, torch.ones(B, cl))
        else:
            vals = set(torch.unique(logical).tolist())
            assert vals <= {0.0, _inv(p).item()}, vals
            N = B * cl
            keep = (logical > 0).double().mean().item()
            assert abs(keep - (1 - p)) <= 5 * (p * (1 - p) / N) ** 0.5 + 1e-12, (B, cl, p, keep)
        masks.append(logical)
        draws += B * cl
        lo = hi
    assert not torch.equal(masks[0], masks[1]), "adjacent segments repeat each other's draws"
    if counter is not None:                      # a different iteration counter gives different masks
        other = torch.full_like(out, float("nan"))
        ctr2 = torch.tensor([counter + 1], dtype=torch.int64, device=_dev())
        ops.dropout_mask_multi(seed, ctr2, ends, [s[3] for s in SEGS], [s[1] for s in SEGS], [s[2] for s in SEGS],
                               other)
        big = slice(ends[7] - 160 * 1024, ends[7])
        assert not torch.equal(other[big], out[big])


def test_dropout_mask_segment_limits_and_grid_stride():
    ops = _ops()
    seed = 11
    ends = [8 * (i + 1) for i in range(64)]
    out = torch.empty(ends[-1], device=_dev())
    ops.dropout_mask_multi(seed, None, ends, [0.5] * 64, [3] * 64, [4] * 64, out)
    ref = ops.dropout_mask(seed, 0, 0.5, 2 * 64, 3, _dev())                  # 64 segments of 2 rows = one 128-row mask
    assert torch.equal(out.view(128, 4), _pad_cols(ref, 4))
    with pytest.raises(RuntimeError, match="ali_dropout_mask_multi"):
        ops.dropout_mask_multi(seed, None, ends + [ends[-1] + 8], [0.5] * 65, [3] * 65, [4] * 65,
                               torch.empty(ends[-1] + 8, device=_dev()))
    # one mask above the element-wise grid cap: the grid-stride loop equals its two halves launched on their own
    B, C = EW_CAP // 64 + 37, 64
    whole = ops.dropout_mask(seed, 5, 0.2, B, C, _dev())
    h = B // 2
    halves = torch.cat([ops.dropout_mask(seed, 5, 0.2, h, C, _dev()), ops.dropout_mask(seed, 5 + h * C, 0.2, B - h, C, _dev())])
    assert torch.equal(whole, halves)


@pytest.fixture
def _dropout_state():
    from ali_hip import dropout
    saved = dict(dropout._state)
    dropout.manual_seed(4242)
    yield dropout
    dropout._state.clear()
    dropout._state.update(saved)


REQS = [(6, 5, 0.2, 8), (6, 32, 0.2, 32), (6, 64, 0.5, 64), (12, 1024, 0.2, 1024), (6, 3, 0.5, 4), (6, 64, 0.5, 64)]


def _run_iteration(dropout, ctr, owner, reqs):
    dropout.begin_iteration(ctr, owner, tag="glue")
    masks = [dropout.next_mask(B, C, p, _dev(), cp).clone() for B, C, p, cp in reqs]
    dropout.end_iteration()
    return masks


def test_dropout_plan_multi_launch_equals_per_mask_draws(_dropout_state):
    """dropout.py: the first iteration draws one launch per mask and records the plan; the next, at the same counter
    value, produces every mask from the plan's one multi launch: every mask must be equal.  A request sequence that
    changes mid-iteration falls back to the per-mask path with the draws of a fresh recording."""
    dropout = _dropout_state
    ctr = torch.tensor([3], dtype=torch.int64, device=_dev())
    owner = types.SimpleNamespace()
    first = _run_iteration(dropout, ctr, owner, REQS)
    plan = owner._mask_plans["glue"]
    dropout.begin_iteration(ctr, owner, tag="glue")
    buf = plan["buf"]
    second = []
    for B, C, p, cp in REQS:
        m = dropout.next_mask(B, C, p, _dev(), cp)
        # served from the plan's buffer (the multi launch), not drawn again
        assert buf.data_ptr() <= m.data_ptr() < buf.data_ptr() + buf.numel() * 4
        second.append(m.clone())
    dropout.end_iteration()
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), f"request {i}: multi-launch mask differs from the per-mask draw"
    assert not torch.equal(first[2], first[5]), "two requests of one iteration share draws"
    # changed sequence: request 2 is another shape -> the rest of the iteration is drawn one launch per mask
    changed = REQS[:2] + [(6, 48, 0.5, 48)] + REQS[3:]
    mixed = _run_iteration(dropout, ctr, owner, changed)
    fresh = _run_iteration(dropout, ctr, types.SimpleNamespace(), changed)
    for i, (a, b) in enumerate(zip(mixed, fresh)):
        assert torch.equal(a, b), f"request {i} after the fallback"
    assert torch.equal(mixed[0], first[0]) and torch.equal(mixed[1], first[1])


# ---------------------------------------------------------------------------------------------- rowmask_mul (exact)
ROWMASK = [(B, r, C) for B in (1, 3, 512) for r in (1, 49, 196) for C in (3, 64, 1024) if B * r * C <= (1 << 25)]
ROWMASK += [(257, 49, 3), (1024, 1, 1024)]


@pytest.mark.parametrize("B,rows,C", ROWMASK)
def test_rowmask_mul_exact(B, rows, C):
    ops = _ops()
    g = torch.Generator().manual_seed(B + rows + C)
    x = torch.randn(B, rows, C, generator=g)
    mask = (torch.rand(B, C, generator=g) > 0.3).float() * 1.25
    mask[:, ::7] = 3.0
    out = ops.rowmask_mul(x.to(_dev()), mask.to(_dev()), B, rows, C)
    assert torch.equal(out.cpu(), x * mask[:, None, :])


# ---------------------------------------------------------------------------------------------- spect_post
@pytest.mark.parametrize("T", (1, 31, 32, 33, 250))
@pytest.mark.parametrize("Fq", (1, 33, 129, 257, 513))
def test_spect_post(T, Fq):
    """power, log, [B,T,F] -> [B,F,T] and the fused standardise + clip of spect_to_img vs float64 (_spect.py):
    |err| <= 2e-6 where re^2 + im^2 >= 1e-3; saturated entries exactly +-1."""
    ops = _ops()
    g = torch.Generator().manual_seed(T * 1000 + Fq)
    B = 3 if T * Fq < 40000 else 2
    y = torch.randn(B, T, 2 * Fq, generator=g)
    y[:, 4::5, :3] = 0.0                                           # power 0: the 1e-6 floor (saturates at -1)
    y[:, 0, 0] = 30.0                                              # power 900: saturates at +1
    k = 3.0
    mean = torch.randn(T, generator=g) * 0.5
    std = torch.rand(T, generator=g) * 0.7 + 0.3
    yd = y.to(_dev())
    out = ops.spect_post(yd, B, T, Fq, torch.full((B, Fq, T), float("nan"), device=_dev()))
    img = ops.spect_post(yd, B, T, Fq, torch.full((B, Fq, T), float("nan"), device=_dev()), mean.to(_dev()),
                         std.to(_dev()), k)
    yy = y.double()
    power = (yy[..., :Fq] ** 2 + yy[..., Fq:] ** 2).transpose(1, 2)                   # [B, F, T]
    ref = (power + 1e-6).log()
    sel = power >= 1e-3
    assert sel.any() and not torch.isnan(out).any() and not torch.isnan(img).any()
    err = (out.cpu().double() - ref).abs()
    assert err[sel].max().item() <= 2e-6
    z = (ref - mean.double()) / (std.double() + 1e-6)
    ref_img = torch.clip(z, -k, k) / k
    got_img = img.cpu().double()
    assert (got_img - ref_img).abs()[sel].max().item() <= 2e-6
    sat = z.abs() > k * (1 + 1e-4)
    assert sat.any() and torch.equal(got_img[sat], torch.sign(z[sat]))


# ---------------------------------------------------------------------------------------------- conditioning planes
def _plane_modules(table, H, W):
    emb = torch.nn.Embedding(table.shape[0], 256).double()
    with torch.no_grad():
        emb.weight.copy_(table.double())
    return emb, torch.nn.Sequential(emb, torch.nn.Unflatten(1, (1, 16, 16)), torch.nn.Upsample(size=(H, W)),
                                    torch.nn.Tanh())


PLANES = [  # B, H, W, table rows (n_emb of them), n_cont, Cpad, mask row stride (0: no mask)
    (1, 256, 256, (10,), 0, 4, 0), (3, 128, 256, (2, 5), 1, 4, 6), (9, 256, 256, (10, 2, 3, 7, 4, 33), 1, 8, 11),
    (3, 512, 512, (3,), 2, 4, 4), (1, 512, 512, (4, 2, 9), 0, 4, 9), (9, 28, 28, (10,), 3, 8, 13),
    (3, 200, 256, (2, 3, 5, 7), 2, 8, 0)]


@pytest.mark.parametrize("B,H,W,rows,n_cont,Cpad,mask_ld", PLANES)
def test_assemble_planes_wide_maps_tables_and_mask(B, H, W, rows, n_cont, Cpad, mask_ld):
    """ali_assemble_planes vs Embedding -> Unflatten -> Upsample(nearest) -> Tanh in float64, the image and the
    continuous planes, times a Dropout2d mask whose row stride exceeds Cpad.  W % 256 == 0 takes the whole-row walk.
    Image / continuous channels: one fp32 multiply, exact; tanh channels: 4 u; padding channels exactly 0."""
    ops = _ops()
    g = torch.Generator().manual_seed(B * H + W + len(rows))
    n_emb = len(rows)
    X = torch.randn(B, H, W, generator=g)
    tabs = [torch.randn(n, 256, generator=g) for n in rows]
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in rows], dim=1).to(torch.int32)
    cont = torch.randn(B, n_cont, generator=g) if n_cont else None
    mask = None
    if mask_ld:
        mask = (torch.rand(B, mask_ld, generator=g) > 0.3).float() * 1.25
        mask[:, 1::3] = 2.0
    out = torch.full((B, H, W, Cpad), float("nan"), device=_dev())
    ops.assemble_planes(X.to(_dev()), idx.to(_dev()), [t.to(_dev()) for t in tabs],
                        None if cont is None else cont.to(_dev()), B, H, W, Cpad, out=out,
                        mask=None if mask is None else mask.to(_dev())[:, :Cpad])
    got = out.cpu()
    mk = torch.ones(B, Cpad) if mask is None else mask[:, :Cpad]
    n_log = 1 + n_emb + n_cont
    assert torch.equal(got[..., 0], X * mk[:, 0, None, None])
    for j in range(n_cont):
        c = 1 + n_emb + j
        assert torch.equal(got[..., c], (cont[:, j:j + 1] * mk[:, c:c + 1])[:, :, None].expand(B, H, W))
    assert torch.equal(got[..., n_log:], torch.zeros(B, H, W, Cpad - n_log))
    with torch.no_grad():
        for j, (t, n) in enumerate(zip(tabs, rows)):
            _, seq = _plane_modules(t, H, W)
            ref = seq(idx[:, j].long())[:, 0] * mk[:, 1 + j, None, None].double()
            err = (got[..., 1 + j].double() - ref).abs()
            assert (err <= 4 * U * ref.abs()).all(), f"table {j}: worst {err.max().item():.3e}"


PTG = [(1, 28, 28, 10), (255, 28, 28, 10), (256, 28, 28, 3), (257, 28, 28, 10), (2048, 28, 28, 10),
       (3, 256, 256, 33), (2, 200, 512, 4)]


@pytest.mark.parametrize("B,H,W,n_rows", PTG)
def test_plane_table_grad_from_the_table(B, H, W, n_rows):
    """plane_table_grad(table=...) (the stepper's form, step.py: _plane_grads) == the x0 path on unmasked planes,
    bitwise, and float64 autograd through the module sequence.  Planes stored with a Dropout2d mask do not change it:
    tanh' comes from the table."""
    ops = _ops()
    g = torch.Generator().manual_seed(B + H * W + n_rows)
    tabs = [torch.randn(5, 256, generator=g), torch.randn(n_rows, 256, generator=g)]
    idx = torch.stack([torch.randint(0, 5, (B,), generator=g), torch.randint(0, n_rows, (B,), generator=g)],
                      dim=1).to(torch.int32)
    X = torch.randn(B, H, W, generator=g)
    Cpad = 4
    gp = torch.randn(B, H, W, Cpad, generator=g)
    Xd, idxd, tabd = X.to(_dev()), idx.to(_dev()), [t.to(_dev()) for t in tabs]
    x0 = ops.assemble_planes(Xd, idxd, tabd, None, B, H, W, Cpad)
    mask = (torch.rand(B, Cpad, generator=g) > 0.5).float().to(_dev()) * 2.0
    x0m = ops.assemble_planes(Xd, idxd, tabd, None, B, H, W, Cpad, mask=mask)
    gd = gp.to(_dev())
    via_x0 = ops.plane_table_grad(gd, 2, x0, 2, idxd, 1, n_rows)
    via_tab = ops.plane_table_grad(gd, 2, None, 2, idxd, 1, n_rows, table=tabd[1])
    assert torch.equal(via_tab, via_x0)
    if B > 8:                       # the masked planes would give another tanh' (where the mask zeroes a plane)
        assert not torch.equal(ops.plane_table_grad(gd, 2, x0m, 2, idxd, 1, n_rows), via_tab)
    # float64 autograd through Embedding -> Unflatten -> Upsample -> Tanh
    emb, seq = _plane_modules(tabs[1], H, W)
    planes = seq(idx[:, 1].long())[:, 0]
    (planes * gp[..., 2].double()).sum().backward()
    ref = emb.weight.grad
    # per (class, cell): a sum over the samples of the class and the pixels of the cell, each term g * (1 - tanh^2)
    with torch.no_grad():
        pt = planes.detach()
        mag = ((gp[..., 2].double() * (1 - pt * pt)).abs())
        oh = F.one_hot(idx[:, 1].long(), n_rows).double()                              # [B, n_rows]
        hh = (torch.arange(H) * 16) // H
        ww = (torch.arange(W) * 16) // W
        cell = (hh[:, None] * 16 + ww[None, :]).reshape(-1)
        per_cell = torch.zeros(B, 256, dtype=torch.float64).index_add_(1, cell, mag.reshape(B, -1))
        terms = oh.t() @ per_cell                                                        # sum |terms| per output
        gabs = oh.t() @ torch.zeros(B, 256, dtype=torch.float64).index_add_(1, cell, gp[..., 2].double().abs().reshape(B, -1))
        n_terms = B * ((H + 15) // 16 + 1) * ((W + 15) // 16 + 1)
        # the summation, plus 1 - p^2 from the fp32 tanh: an absolute error of a few u per term (cancels near |p| = 1)
        bound = (n_terms + 8) * U * terms + 8 * U * gabs
        s = int(idx[:, 1].long().bincount(minlength=n_rows).argmax())
        b = int((idx[:, 1] == s).nonzero()[0])                                           # one sample of that class
        contrib = torch.zeros(B, 256, dtype=torch.float64).index_add_(
            1, cell, (gp[..., 2].double() * (1 - pt * pt)).reshape(B, -1))
        buggy = ref.clone()
        buggy[s] -= contrib[b]
    assert_within(via_tab, ref, bound, buggy, "plane table grad")
