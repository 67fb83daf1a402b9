"""The two pertinent-positive kernels of the contrastive family alone, through ``ali_hip.ops`` (csrc/contrast.hip):
``ct_pp_attack`` and ``ct_pp_update``; the method of test_gpu_contrast_kernels.py.

Reference: the statement of each kernel (``ali_hip.contrast.attack_pp_statement``, ``pp_update_statement``) in fp64 on
the fp32 inputs; yardstick: the same statement in CPU fp32 (``_check`` of test_gpu_xent.py; per-row scalars pooled with
``_check_pooled`` of test_gpu_explain.py).  Logits, gradients and states are given, so every discrete outcome is
compared exactly: arg-max, success flags (pred == t0), the seed (+-c or 0) with its zero columns and padding, the
pixels at the background b, the pixels at x0 (both as the fp64 reference rounded to fp32 has them), the box
[min(b, x0), max(b, x0)], the reset to b bit for bit, the counters, the distances of the iterate as stored, and every
call against its own repetition.

Shapes: N = 35 (less than a block), 784 (the 16-byte path) and 4099 (odd, more than one pass of the block over the
row); C = 2, 3, 10; B = 1 and 3 with the rows at k = 1, 0, K (K = 3); gx_stride 1 and 4; the clip on and off;
b = 0.0 and -1.0 with x0 in [-1, 1] and some pixels of x0 exactly b.
"""
import pytest
import torch

from test_gpu_explain import _check_pooled
from test_gpu_xent import _check

gpu = pytest.mark.gpu

NS = (35, 784, 4099)
K = 3
ITS = (1, 0, K)                  # the rows' iteration counters: a momentum step, the first step, the end of a round
BGS = (0.0, -1.0)


# ------------------------------------------------------------------------------------------------ ct_pp_attack
def _attack_inputs(B, C, variant):
    g = torch.Generator().manual_seed(100 * B + C + 1)
    z = torch.randn(2 * B, C, generator=g)                         # rows [0, B): evaluated; rows [B, 2B): attacked
    t0 = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    c = torch.rand(B, generator=g) * 20 + 0.5
    kappa = 0.75
    rows = torch.arange(B)
    if variant == "ties":
        for r in range(2 * B):
            top = z[r].max().item() + 1.0
            z[r, [(3 * r) % C, (3 * r + 64) % C, (3 * r + 7) % C]] = top
    elif variant == "own_label":                                   # t0 is the arg-max of the evaluated row: a success
        t0 = z[:B].argmax(1).to(torch.int32)
    elif variant == "active":                                      # own far below the others: the hinge is on
        z[B + rows, t0.long()] = -50.0
    elif variant == "inactive":                                    # own far above the others: the hinge is off
        z[B + rows, t0.long()] = 50.0
    elif variant == "zero_margin":                                 # other - own + kappa == 0 exactly: off
        z[B:] = -3.0
        z[B + rows, t0.long()] = 2.0
        z[B + rows, (t0.long() + 1) % C] = 1.25
    return z.contiguous(), t0, c, kappa


@gpu
@pytest.mark.parametrize("C", [2, 3, 10])
@pytest.mark.parametrize("B", [1, 3])
def test_pp_attack_seed_argmax_and_flags(B, C):
    from ali_hip import ops
    from ali_hip.contrast import attack_pp_statement
    triples = []
    for variant in ("normal", "ties", "own_label", "active", "inactive", "zero_margin"):
        z, t0, c, kappa = _attack_inputs(B, C, variant)
        label = f"B={B} C={C} {variant}"
        A64, seed64, other = attack_pp_statement(z[B:].double(), t0, c.double(), kappa)
        A32, _, _ = attack_pp_statement(z[B:], t0, c, kappa)
        ld = C + 3
        got = ops.ct_pp_attack(z.cuda(), B, t0.cuda(), c.cuda(), kappa, 0, B, seed_ld=ld)
        again = ops.ct_pp_attack(z.cuda(), B, t0.cuda(), c.cuda(), kappa, 0, B, seed_ld=ld)
        seed, A, pred, succ = got
        assert all(torch.equal(a, b) for a, b in zip(got, again)), label
        want_pred = z[:B].argmax(1)
        assert torch.equal(pred.cpu().long(), want_pred), label
        assert torch.equal(succ.cpu().bool(), want_pred == t0.long()), label
        assert seed.shape == (B, ld) and not seed[:, C:].any(), label              # the padding is exactly 0
        assert torch.equal(seed[:, :C].cpu().double(), seed64), label              # +-c or 0: no rounding in it
        active = A64 > 0
        assert torch.equal(seed[:, :C].cpu().ne(0).sum(1), 2 * active.long()), label
        rows = torch.arange(B)
        sc = seed[:, :C].cpu()
        assert torch.equal(sc[rows, t0.long()], torch.where(active, -c, torch.zeros_like(c))), label  # -c on t0
        assert torch.equal(sc[rows, other], torch.where(active, c, torch.zeros_like(c))), label       # +c on other
        if variant in ("inactive", "zero_margin"):
            assert not active.any() and not A.any() and not seed.any(), label
        if variant == "active":
            assert active.all(), label
        if variant == "own_label":
            assert succ.all(), label
        if variant == "ties":                                                      # the first of the tied others
            tied = z[B:][rows, other]
            for r in range(B):
                first = [j for j in range(C) if j != t0[r] and z[B + r, j] == tied[r]][0]
                assert other[r] == first, label
        triples.append((A, A64, A32))
        # one set of rows for both roles: the same kernel with both offsets 0
        s1, A1, p1, u1 = ops.ct_pp_attack(z[B:].contiguous().cuda(), B, t0.cuda(), c.cuda(), kappa)
        assert torch.equal(s1, seed[:, :C]) and torch.equal(A1, A), label
        assert torch.equal(p1.cpu().long(), z[B:].argmax(1)), label
        assert torch.equal(u1.cpu().bool(), z[B:].argmax(1) == t0.long()), label
    _check_pooled(f"ct_pp_attack A B={B} C={C}", triples)


@gpu
def test_pp_attack_refuses_rows_outside_the_logits():
    from ali_hip import ops
    z = torch.zeros(4, 3, device="cuda")
    t0, c = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    for kw in (dict(eval_off=3), dict(grad_off=3), dict(seed_ld=2)):
        with pytest.raises(RuntimeError):
            ops.ct_pp_attack(z, 2, t0, c, 1.0, **kw)
    with pytest.raises(RuntimeError):
        ops.ct_pp_attack(torch.zeros(4, 1, device="cuda"), 2, t0, c, 1.0)         # one class: nothing to attack


# ------------------------------------------------------------------------------------------------ ct_pp_update
def _rows_ref(fn, it, parts):
    """``fn(row tensors..., k)`` row by row (every row has its own iteration counter), stacked"""
    outs = [fn(*[p[r:r + 1] for p in parts], int(it[r])) for r in range(len(it))]
    return [torch.cat([o[i] for o in outs]) for i in range(len(outs[0]))]


def _pp_inputs(B, N, gs, bg):
    g = torch.Generator().manual_seed(13 * B + N + (0 if bg == 0.0 else 5000))
    x0 = torch.rand(B, N, generator=g) * 2 - 1
    x0[:, 2::9] = bg                                               # x0 == b: the box is one point
    lo, hi = torch.minimum(x0, torch.full_like(x0, bg)), torch.maximum(x0, torch.full_like(x0, bg))
    inside = lambda p: torch.minimum(torch.maximum(  # noqa: E731
        bg + torch.rand(B, N, generator=g) * (torch.rand(B, N, generator=g) < p) * (x0 - bg), lo), hi)
    v, y = inside(0.6), inside(0.6)
    gx = torch.randn(B, N, gs, generator=g)
    gx[:, ::5, 0] *= 40.0                                          # far steps: both ends of the box
    gx[:, 1::7, 0] = 0.0
    y[:, 1::7] = bg                                                # g == 0 there: u == b, the pixel shrinks to b
    it = torch.tensor(ITS[:B], dtype=torch.int32)
    return x0, v, y, gx.contiguous(), it, lo, hi


@gpu
@pytest.mark.parametrize("bg", BGS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("clip", [1e4, 2.0], ids=["clip_off", "clip_on"])
def test_pp_update(B, N, clip, bg):
    from ali_hip import ops
    from ali_hip.contrast import pp_update_statement
    lr, beta = 0.05, 0.1
    gs = 4 if N != 35 else 1
    x0, v, y, gx, it, lo, hi = _pp_inputs(B, N, gs, bg)
    label = f"pp B={B} N={N} clip={clip} b={bg}"

    def ref(dt):
        def one(v_, y_, x_, g_, k):
            if k >= K:
                z = torch.zeros(1, dtype=dt)
                return torch.full_like(x_, bg), torch.full_like(x_, bg), z, z, z
            return pp_update_statement(v_, y_, x_, g_, k, K, lr, beta, clip, bg)
        return _rows_ref(one, it, [t.to(dt) for t in (v, y, x0, gx[:, :, 0])])
    (v64, y64, l1_64, l2_64, n64), (v32, y32, l1_32, l2_32, n32) = ref(torch.float64), ref(torch.float32)
    live = it < K
    assert ((n64[live] > clip).all() if clip < 10 else (n64[live] < clip).all()), label     # the clip is on / off

    def call():
        d = lambda t: t.clone().cuda()  # noqa: E731
        st = dict(v=d(v), y=d(y), it=d(it), rnd=torch.full((B,), 5, dtype=torch.int32, device="cuda"))
        for n in ("l1", "l2", "dist", "gnorm"):
            st[n] = torch.full((B,), -1.0, device="cuda")
        ops.ct_pp_update(gx.cuda(), st["v"], st["y"], x0.cuda(), bg, st["it"], st["rnd"], K, lr, beta, clip,
                         st["l1"], st["l2"], st["dist"], st["gnorm"])
        return st
    st, again = call(), call()
    assert all(torch.equal(st[n], again[n]) for n in st), label
    gv, gy = st["v"].cpu(), st["y"].cpu()
    # counters: a step counts the iteration, the end of a round starts the next one from b
    assert torch.equal(st["it"].cpu(), torch.where(live, it + 1, torch.zeros_like(it))), label
    assert torch.equal(st["rnd"].cpu(), 5 + (~live).int()), label
    for r in range(B):
        if not live[r]:
            assert torch.equal(gv[r], torch.full((N,), bg)) and torch.equal(gy[r], torch.full((N,), bg)), label
            assert st["l1"][r] == 0 and st["l2"][r] == 0 and st["dist"][r] == 0, label
    # discrete outcomes, exactly: pixels at b (shrink or an end of the box), pixels at x0, the box
    for got, r64 in ((gv, v64), (gy, y64)):
        assert torch.equal(got == bg, r64.float() == bg), label
        assert torch.equal(got == x0, r64.float() == x0), label
        assert ((got >= lo) & (got <= hi)).all(), label
    lv = live.unsqueeze(1)
    off = x0 != bg
    assert ((gv == bg) & off & lv).any() and ((gv != bg) & (gv != x0) & lv).any(), label
    if clip > 10:                                                  # (clipped to a norm of 2, no step reaches x0)
        for side in (x0 > bg, x0 < bg):                            # the x0 end above b and below it (b = 0 only:
            if (side & lv).any():                                  # no x0 in [-1, 1] lies below b = -1)
                assert ((gv == x0) & side & lv).any(), label
    _check(label + " v", st["v"], v64, v32)
    _check(label + " y", st["y"], y64, y32)
    lr_ = live.nonzero().reshape(-1)
    dist64, dist32 = l2_64 + beta * l1_64, l2_32 + beta * l1_32
    _check_pooled(label + " scalars", [(st["l1"][lr_], l1_64[lr_], l1_32[lr_]), (st["l2"][lr_], l2_64[lr_], l2_32[lr_]),
                                       (st["dist"][lr_], dist64[lr_], dist32[lr_]),
                                       (st["gnorm"][lr_], n64[lr_], n32[lr_])])
    # the distances are those of the iterate as stored, from b
    d = gv.double() - bg
    assert torch.allclose(st["l1"].cpu().double(), d.abs().sum(1), rtol=1e-6, atol=0), label
    assert torch.allclose(st["l2"].cpu().double(), d.pow(2).sum(1), rtol=1e-6, atol=0), label
