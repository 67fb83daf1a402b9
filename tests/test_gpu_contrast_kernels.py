"""The kernels of the contrastive family alone, through ``ali_hip.ops`` (csrc/contrast.hip): ``ct_attack``, ``ct_book``,
``ct_cem_update`` and ``ct_ce_update``.

Reference: the statement of each kernel (``ali_hip.contrast``: ``attack_statement``, ``cem_update_statement``,
``ce_update_statement``, ``c_table_statement``) in fp64 on the fp32 inputs; yardstick: the same statement in CPU fp32
(``_check`` of test_gpu_xent.py: e(device) <= YARD * e(cpu fp32) and <= RTOL * max|ref64|).  Per-row scalars of a call
are a handful of numbers and are pooled as test_gpu_explain.py pools small tensors.  Logits, gradients and states are
given, not computed on the device, so every discrete outcome is compared exactly: arg-max, success flags, the seed (its
values are +-c or 0) with its zero columns and padding, which rows went into the best, ``found``, the c table on
exactly representable inputs, the pixels the projections put back to x0, the clamped pixels (both as the fp64
reference rounded to fp32 has them), the counters, and every call against its own repetition.

Shapes: N = 35 (less than a block), 784 (a multiple of four: the 16-byte path) and 4099 (odd, more than one pass of
the block over the row); C = 2, 3, 10; B = 1 and 3.  Rows of a call sit at different iterations of their round (the
counters are per row), the last of three at k == K, where the kernels start the next round instead.
"""
import pytest
import torch

from test_gpu_explain import _check_pooled
from test_gpu_xent import _check

gpu = pytest.mark.gpu

NS = (35, 784, 4099)
K = 3
ITS = (1, 0, K)                  # the rows' iteration counters: a momentum step, the first step, the end of a round


# ------------------------------------------------------------------------------------------------ ct_attack
def _attack_inputs(B, C, variant):
    g = torch.Generator().manual_seed(100 * B + C)
    z = torch.randn(2 * B, C, generator=g)                         # rows [0, B): evaluated; rows [B, 2B): attacked
    t0 = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    c = torch.rand(B, generator=g) * 20 + 0.5
    kappa = 0.75
    if variant == "ties":
        for r in range(2 * B):
            top = z[r].max().item() + 1.0
            z[r, [(3 * r) % C, (3 * r + 64) % C, (3 * r + 7) % C]] = top
    elif variant == "own_label":                                   # t0 is the arg-max of both rows: no success, hinge on
        t0 = z[:B].argmax(1).to(torch.int32)
        z[B:] = z[:B]
    elif variant == "inactive":                                    # own far below the others: the hinge is off
        z[B + torch.arange(B), t0.long()] = -50.0
    elif variant == "zero_margin":                                 # own - other + kappa == 0 exactly: off
        z[B:] = -3.0
        z[B + torch.arange(B), t0.long()] = 1.25
        z[B + torch.arange(B), (t0.long() + 1) % C] = 2.0
    return z.contiguous(), t0, c, kappa


@gpu
@pytest.mark.parametrize("C", [2, 3, 10])
@pytest.mark.parametrize("B", [1, 3])
def test_attack_seed_argmax_and_flags(B, C):
    from ali_hip import ops
    from ali_hip.contrast import attack_statement
    triples = []
    for variant in ("normal", "ties", "own_label", "inactive", "zero_margin"):
        z, t0, c, kappa = _attack_inputs(B, C, variant)
        label = f"B={B} C={C} {variant}"
        A64, seed64, other = attack_statement(z[B:].double(), t0, c.double(), kappa)
        A32, _, _ = attack_statement(z[B:], t0, c, kappa)
        ld = C + 3
        got = ops.ct_attack(z.cuda(), B, t0.cuda(), c.cuda(), kappa, 0, B, seed_ld=ld)
        again = ops.ct_attack(z.cuda(), B, t0.cuda(), c.cuda(), kappa, 0, B, seed_ld=ld)
        seed, A, pred, succ = got
        assert all(torch.equal(a, b) for a, b in zip(got, again)), label
        want_pred = z[:B].argmax(1)
        assert torch.equal(pred.cpu().long(), want_pred), label
        assert torch.equal(succ.cpu().bool(), want_pred != t0.long()), label
        assert seed.shape == (B, ld) and not seed[:, C:].any(), label              # the padding is exactly 0
        assert torch.equal(seed[:, :C].cpu().double(), seed64), label              # +-c or 0: no rounding in it
        active = A64 > 0
        assert torch.equal(seed[:, :C].cpu().ne(0).sum(1), 2 * active.long()), label
        if variant in ("inactive", "zero_margin"):
            assert not active.any() and not A.any() and not seed.any(), label
        if variant == "own_label":
            assert active.all(), label
        if variant == "ties":                                                      # the first of the tied others
            rows = torch.arange(B)
            tied = z[B:][rows, other]
            for r in range(B):
                first = [j for j in range(C) if j != t0[r] and z[B + r, j] == tied[r]][0]
                assert other[r] == first, label
                assert seed[r, first].item() == (-c[r].item() if active[r] else 0.0), label
        triples.append((A, A64, A32))
        # one set of rows for both roles (the counterfactual search): the same kernel with both offsets 0
        s1, A1, p1, u1 = ops.ct_attack(z[B:].contiguous().cuda(), B, t0.cuda(), c.cuda(), kappa)
        assert torch.equal(s1, seed[:, :C]) and torch.equal(A1, A), label
        assert torch.equal(p1.cpu().long(), z[B:].argmax(1)), label
        # without labels: the arg-max alone
        none_s, none_a, p0, none_u = ops.ct_attack(z.cuda(), 2 * B)
        assert none_s is None and none_a is None and none_u is None and torch.equal(p0.cpu().long(), z.argmax(1)), label
    _check_pooled(f"ct_attack A B={B} C={C}", triples)


@gpu
def test_attack_refuses_rows_outside_the_logits():
    from ali_hip import ops
    z = torch.zeros(4, 3, device="cuda")
    t0, c = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    for kw in (dict(eval_off=3), dict(grad_off=3), dict(seed_ld=2)):
        with pytest.raises(RuntimeError):
            ops.ct_attack(z, 2, t0, c, 1.0, **kw)
    with pytest.raises(RuntimeError):
        ops.ct_attack(torch.zeros(4, 1, device="cuda"), 2, t0, c, 1.0)            # one class: nothing to attack


# ------------------------------------------------------------------------------------------------ ct_cem_update
def _rows_ref(fn, it, parts):
    """``fn(row tensors..., k)`` row by row (every row has its own iteration counter), stacked"""
    outs = [fn(*[p[r:r + 1] for p in parts], int(it[r])) for r in range(len(it))]
    return [torch.cat([o[i] for o in outs]) for i in range(len(outs[0]))]


def _cem_inputs(B, N, gs):
    g = torch.Generator().manual_seed(7 * B + N)
    x0 = torch.rand(B, N, generator=g) * 2 - 1
    up = lambda p: torch.rand(B, N, generator=g) * 0.4 * (torch.rand(B, N, generator=g) < p)  # noqa: E731
    v, y = x0 + up(0.6), x0 + up(0.6)
    gx = torch.randn(B, N, gs, generator=g)
    gx[:, ::5, 0] *= 40.0                                          # far steps: both clamps and the far side of x0
    gx[:, 1::7, 0] = 0.0
    y[:, 1::7] = x0[:, 1::7]                                       # g == 0 there: |d| <= beta, the pixel stays x0
    it = torch.tensor(ITS[:B], dtype=torch.int32)
    return x0, v, y, gx.contiguous(), it, x0.amin(1), x0.amax(1)


@gpu
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("clip", [1e4, 2.0], ids=["clip_off", "clip_on"])
def test_cem_update(B, N, clip):
    from ali_hip import ops
    from ali_hip.contrast import cem_update_statement
    lr, beta = 0.05, 0.1
    gs = 4 if N != 35 else 1
    x0, v, y, gx, it, lo, hi = _cem_inputs(B, N, gs)
    label = f"cem B={B} N={N} clip={clip}"

    def ref(dt):
        def one(v_, y_, x_, g_, lo_, hi_, k):
            if k >= K:
                z = torch.zeros(1, dtype=dt)
                return x_.clone(), x_.clone(), z, z, z
            return cem_update_statement(v_, y_, x_, g_, k, K, lr, beta, clip, lo_, hi_)
        return _rows_ref(one, it, [t.to(dt) for t in (v, y, x0, gx[:, :, 0], lo, hi)])
    (v64, y64, l1_64, l2_64, n64), (v32, y32, l1_32, l2_32, n32) = ref(torch.float64), ref(torch.float32)
    live = it < K
    assert ((n64[live] > clip).all() if clip < 10 else (n64[live] < clip).all()), label     # the clip is on / off

    def call():
        d = lambda t: t.clone().cuda()  # noqa: E731
        st = dict(v=d(v), y=d(y), it=d(it), rnd=torch.full((B,), 5, dtype=torch.int32, device="cuda"))
        for n in ("l1", "l2", "dist", "gnorm"):
            st[n] = torch.full((B,), -1.0, device="cuda")
        ops.ct_cem_update(gx.cuda(), st["v"], st["y"], x0.cuda(), lo.cuda(), hi.cuda(), st["it"], st["rnd"], K, lr,
                          beta, clip, st["l1"], st["l2"], st["dist"], st["gnorm"])
        return st
    st, again = call(), call()
    assert all(torch.equal(st[n], again[n]) for n in st), label
    gv, gy = st["v"].cpu(), st["y"].cpu()
    # counters: a step counts the iteration, the end of a round starts the next one
    assert torch.equal(st["it"].cpu(), torch.where(live, it + 1, torch.zeros_like(it))), label
    assert torch.equal(st["rnd"].cpu(), 5 + (~live).int()), label
    for r in range(B):
        if not live[r]:
            assert torch.equal(gv[r], x0[r]) and torch.equal(gy[r], x0[r]), label
            assert st["l1"][r] == 0 and st["l2"][r] == 0 and st["dist"][r] == 0, label
    # discrete outcomes, exactly: pixels back at x0 (shrink or projection) and pixels on a clamp
    # (of the reference rounded to fp32: a step of less than half an ulp above x0 is x0 in any fp32 result)
    x64 = x0.double()
    assert torch.equal(gv == x0, v64.float() == x0) and torch.equal(gy == x0, y64.float() == x0), label
    assert torch.equal(gv == hi.unsqueeze(1), v64.float() == hi.unsqueeze(1)), label
    assert (gv >= x0).all() and (gy >= x0).all() and (gv <= hi.unsqueeze(1)).all(), label
    lv = live.unsqueeze(1)
    assert ((gv == x0) & lv).any() and ((gv > x0) & lv).any(), label
    if clip > 10:                                                  # (clipped to a norm of 2, no step reaches a clamp)
        assert ((gv == hi.unsqueeze(1)) & (gv != x0) & lv).any(), label
    _check(label + " v", st["v"], v64, v32)
    _check(label + " y", st["y"], y64, y32)
    lr_ = live.nonzero().reshape(-1)
    dist64, dist32 = l2_64 + beta * l1_64, l2_32 + beta * l1_32
    _check_pooled(label + " scalars", [(st["l1"][lr_], l1_64[lr_], l1_32[lr_]), (st["l2"][lr_], l2_64[lr_], l2_32[lr_]),
                                       (st["dist"][lr_], dist64[lr_], dist32[lr_]),
                                       (st["gnorm"][lr_], n64[lr_], n32[lr_])])
    # the distances are those of the iterate as stored
    d = (gv.double() - x64)
    assert torch.allclose(st["l1"].cpu().double(), d.abs().sum(1), rtol=1e-6, atol=0), label
    assert torch.allclose(st["l2"].cpu().double(), d.pow(2).sum(1), rtol=1e-6, atol=0), label


# ------------------------------------------------------------------------------------------------ ct_ce_update
def _ce_inputs(B, N, gs):
    g = torch.Generator().manual_seed(11 * B + N)
    x0 = torch.rand(B, N, generator=g) * 2 - 1
    v = x0 + torch.randn(B, N, generator=g) * 0.2
    v[:, ::3] = x0[:, ::3]                                         # sign(0) pixels
    lo, hi = x0.amin(1), x0.amax(1)
    v = torch.minimum(torch.maximum(v, lo.unsqueeze(1)), hi.unsqueeze(1))
    gx = torch.randn(B, N, gs, generator=g)
    m = torch.randn(B, N, generator=g) * 0.3
    v2 = torch.rand(B, N, generator=g) * 0.1
    it = torch.tensor(ITS[:B], dtype=torch.int32)
    return x0, v, gx.contiguous(), m, v2, it, lo, hi


@gpu
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("clip", [1e3, 2.0], ids=["clip_off", "clip_on"])
def test_ce_update(B, N, clip):
    from ali_hip import ops
    from ali_hip.contrast import ce_update_statement
    lr, gamma = 0.05, 1.0
    gs = 4 if N != 35 else 1
    x0, v, gx, m, v2, it, lo, hi = _ce_inputs(B, N, gs)
    label = f"ce B={B} N={N} clip={clip}"

    def ref(dt):
        def one(v_, x_, g_, m_, s_, lo_, hi_, k):
            if k >= K:
                z = torch.zeros(1, dtype=dt)
                return x_.clone(), torch.zeros_like(x_), torch.zeros_like(x_), z, z
            return ce_update_statement(v_, x_, g_, m_, s_, k + 1, lr, gamma, clip, lo_, hi_)
        return _rows_ref(one, it, [t.to(dt) for t in (v, x0, gx[:, :, 0], m, v2, lo, hi)])
    (v64, m64, s64, l1_64, n64), (v32, m32, s32, l1_32, n32) = ref(torch.float64), ref(torch.float32)
    live = it < K
    assert ((n64[live] > clip).all() if clip < 10 else (n64[live] < clip).all()), label

    def call():
        d = lambda t: t.clone().cuda()  # noqa: E731
        st = dict(v=d(v), m=d(m), v2=d(v2), it=d(it), rnd=torch.full((B,), 5, dtype=torch.int32, device="cuda"),
                  l1=torch.full((B,), -1.0, device="cuda"), gnorm=torch.full((B,), -1.0, device="cuda"))
        ops.ct_ce_update(gx.cuda(), st["v"], x0.cuda(), lo.cuda(), hi.cuda(), st["m"], st["v2"], st["it"], st["rnd"], K,
                         lr, gamma, clip, st["l1"], st["gnorm"])
        return st
    st, again = call(), call()
    assert all(torch.equal(st[n], again[n]) for n in st), label
    gv = st["v"].cpu()
    assert torch.equal(st["it"].cpu(), torch.where(live, it + 1, torch.zeros_like(it))), label
    assert torch.equal(st["rnd"].cpu(), 5 + (~live).int()), label
    for r in range(B):
        if not live[r]:
            assert torch.equal(gv[r], x0[r]) and not st["m"][r].any() and not st["v2"][r].any(), label
            assert st["l1"][r] == 0, label
    lo1, hi1 = lo.unsqueeze(1), hi.unsqueeze(1)
    lv = live.unsqueeze(1)
    assert torch.equal((gv == lo1) & lv, (v64.float() == lo1) & lv), label        # clamped pixels, exactly (of the
    assert torch.equal((gv == hi1) & lv, (v64.float() == hi1) & lv), label        # reference rounded to fp32)
    assert (((gv == lo1) | (gv == hi1)) & lv).any() and (gv >= lo1).all() and (gv <= hi1).all(), label
    _check(label + " v", st["v"], v64, v32)
    _check(label + " m", st["m"], m64, m32)
    _check(label + " v2", st["v2"], s64, s32)
    lr_ = live.nonzero().reshape(-1)
    _check_pooled(label + " scalars", [(st["l1"][lr_], l1_64[lr_], l1_32[lr_]), (st["gnorm"][lr_], n64[lr_], n32[lr_])])
    assert torch.allclose(st["l1"].cpu().double(), (gv.double() - x0.double()).abs().sum(1), rtol=1e-6, atol=0), label


@gpu
def test_ce_update_sign_of_zero():
    """v == x0 everywhere with no classifier gradient and no momentum: g = gamma * sign(0) = 0, nothing moves"""
    from ali_hip import ops
    B, N = 2, 784
    x0 = (torch.rand(B, N, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    z = lambda: torch.zeros(B, N, device="cuda")  # noqa: E731
    v, m, v2 = x0.clone(), z(), z()
    it, rnd = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    l1, gn = torch.ones(B, device="cuda"), torch.ones(B, device="cuda")
    ops.ct_ce_update(z(), v, x0, x0.amin(1), x0.amax(1), m, v2, it, rnd, K, 0.1, 1.0, 1e3, l1, gn)
    assert torch.equal(v, x0) and not m.any() and not v2.any() and not l1.any() and not gn.any()
    assert it.tolist() == [1, 1] and rnd.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ ct_book
def _book_case(N):
    """six rows, each with its own story; run as one call of B = 6 ... no: as two calls of B = 3 and six of B = 1"""
    g = torch.Generator().manual_seed(N)
    rows = 6
    v = torch.randn(rows, N, generator=g)
    best = torch.randn(rows, N, generator=g)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    f32 = lambda *a: torch.tensor(a, dtype=torch.float32)  # noqa: E731
    #            improves   ties the best   no success   k == 0    round ends    round ends     (the last two at k == K)
    it = i32(1, 2, 2, 0, K, K)
    succ = i32(1, 1, 0, 1, 0, 1)
    dist = f32(0.5, 0.75, 0.1, 0.1, 0.1, 3.0)
    best_dist = f32(float("inf"), 0.75, 1.0, 1.0, 2.0, 2.0)
    pred = i32(7, 3, 4, 5, 6, 8)
    best_label = i32(1, 1, 1, 1, 2, 2)
    found = i32(0, 1, 0, 0, 1, 1)
    round_succ = i32(0, 0, 0, 0, 0, 0)
    ctab = torch.stack([f32(10, 10, 10, 10, 10, 5), f32(0, 0, 0, 0, 0, 0), f32(1e10, 1e10, 1e10, 1e10, 1e10, 10)])
    return dict(v=v, dist=dist, succ=succ, pred=pred, it=it, best=best, best_dist=best_dist, best_label=best_label,
                found=found, round_succ=round_succ, ctab=ctab)


def _book_expect(c):
    from ali_hip.contrast import c_table_statement
    hit = (c["it"] >= 1) & (c["succ"] != 0)
    better = hit & (c["dist"] < c["best_dist"])
    rs = (c["round_succ"] != 0) | hit
    end = c["it"] >= K
    c2, lo2, hi2 = c_table_statement(c["ctab"][0].double(), c["ctab"][1].double(), c["ctab"][2].double(), rs)
    ctab = torch.where(end.unsqueeze(0), torch.stack([c2, lo2, hi2]).float(), c["ctab"])
    return dict(copied=better.int(), best=torch.where(better.unsqueeze(1), c["v"], c["best"]),
                best_dist=torch.where(better, c["dist"], c["best_dist"]),
                best_label=torch.where(better, c["pred"], c["best_label"]), found=torch.where(better, 1, c["found"]).int(),
                round_succ=torch.where(end, 0, rs.int()).int(), ctab=ctab)


@gpu
@pytest.mark.parametrize("N", NS)
def test_book_best_so_far_and_the_c_table(N):
    from ali_hip import ops
    case = _book_case(N)
    want = _book_expect(case)
    assert want["copied"].tolist() == [1, 0, 0, 0, 0, 0] and want["found"].tolist() == [1, 1, 0, 0, 1, 1]
    # the table: failure with c_hi open -> c * 10; success (this very iterate) with c_hi = 10 -> c_hi = 5, c = 2.5
    assert want["ctab"][:, 4].tolist() == [100.0, 10.0, 1e10] and want["ctab"][:, 5].tolist() == [2.5, 0.0, 5.0]
    for sel in ([0, 1, 2], [3, 4, 5]) + tuple([r] for r in range(6)):
        def call():
            st = {k: (t[:, sel] if k == "ctab" else t[sel]).clone().contiguous().cuda() for k, t in case.items()}
            st["copied"] = ops.ct_book(st["v"], st["dist"], st["succ"], st["pred"], st["it"], K, st["best"],
                                       st["best_dist"], st["best_label"], st["found"], st["round_succ"], st["ctab"])
            return st
        st, again = call(), call()
        assert all(torch.equal(st[k], again[k]) for k in st), sel
        for k, t in want.items():
            w = t[:, sel] if k == "ctab" else t[sel]
            assert torch.equal(st[k].cpu(), w), (sel, k)
        for k in ("v", "dist", "succ", "pred", "it"):                             # the inputs are inputs
            assert torch.equal(st[k].cpu(), case[k][sel]), (sel, k)


@gpu
def test_book_c_table_over_rounds():
    """the round's success flag is carried from an earlier iterate to the end of the round; a failed round after a
    successful one bisects upwards"""
    from ali_hip import ops
    N, B = 35, 2
    dev = dict(device="cuda")
    v, best = torch.zeros(B, N, **dev), torch.zeros(B, N, **dev)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, **dev)  # noqa: E731
    best_dist, best_label, found, rs = torch.full((B,), float("inf"), **dev), i32(0, 0), i32(0, 0), i32(0, 0)
    ctab = torch.tensor([[8.0, 8.0], [0.0, 0.0], [1e10, 1e10]], **dev)
    dist, pred = torch.ones(B, **dev), i32(1, 1)
    steps = [(1, (1, 0)), (2, (0, 0)), (K, (0, 0)),          # round 0: row 0 succeeded at k = 1 -> c = 4; row 1 -> 80
             (1, (0, 0)), (K, (0, 0))]                       # round 1: both fail -> row 0 (4 + 8) / 2 = 6; row 1 -> 800
    for k, succ in steps:
        ops.ct_book(v, dist, i32(*succ), pred, i32(k, k), K, best, best_dist, best_label, found, rs, ctab)
    assert ctab.cpu().tolist() == [[6.0, 800.0], [4.0, 80.0], [8.0, 1e10]]
    assert found.tolist() == [1, 0] and rs.tolist() == [0, 0]
