"""Every launch route of the stand-alone BatchNorm passes, ali_colsum and ali_act_bwd (csrc/elementwise.hip).

The entry points choose between float4 kernels (rowreduce_vec_kernel<0|1|2>, bn_apply_vec_kernel,
bn_bwd_apply_vec_kernel) and scalar ones by C, row count and the 16-byte alignment of the operands they name, and size a
reduction grid (capped at 512 blocks) and an element-wise grid (capped at 2048 blocks, then grid-strided).  The cases
of tests/bn_cases.py are the smallest shapes that take each route; ``ops.ew_plan`` -- the launches' own plan -- is
asserted for every case first (without a GPU), so a later change of the dispatch cannot move a case silently.  The
``rows * C >= 2^31`` arm of ``vec_ok`` needs an 8 GB operand and stays untested.

Reference: a plain fp64 restatement of the formulas on the CPU (not nn.BatchNorm2d, which refuses count = 1 and hides
the per-group order).  Two legs:

- exact (every case, the capped ones included): x and g are integers in [-3, 3], masks in {0, 2}, the planted
  statistics of the backward integer means and invstd in {0.5, 1, 2}.  Every per-channel sum of |terms| stays below
  2^23 (asserted), so each product and partial sum is exact in fp32 in any order, with or without contraction: mean,
  dgamma, dbeta and colsum are compared with torch.equal, leaky / none act_bwd too (one multiply).  The unbiased running
  variance is held to 1 ulp (momentum 0.5 from zero running stats: the first pass stores exactly half of it);
- float (cases with 8 to 600 rows; at count = 1, L = rows cannot absorb the three roundings of one g~ * xhat term):
  LeakyReLU(2 randn + 0.5) inputs.  Reductions are held to ``L * 2^-24 * sum|terms|`` with L = rows (every summation
  tree of the kernels is shallower than rows minus the roundings of one term), propagated through mean^2 for the
  variance, and a reference with one row of an unmasked image dropped must violate that bound (checked on the CPU,
  without a GPU, for every case).

Derived values (invstd, sc, sh, running-stat blends) and element-wise outputs (bn_apply, gx, tanh act_bwd) are held to
``k * 2^-24 * sum|terms of their formula|`` plus the propagated error of their inputs, k the fp32 roundings counted in
the kernel's expression (written next to each bound, one spare).  Never relative to a tensor maximum.

Every output lives inside a larger NaN-filled buffer and starts NaN; the margins must still be NaN afterwards.
DESIGN.md 4 has the route table and the measured worst err / bound per leg."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import bn_cases as bc

gpu = pytest.mark.gpu

U = 2.0 ** -24          # unit round-off of fp32
UD = 2.0 ** -53         # ... of fp64 (the finals sum and divide in double)
PAD = 64                # floats of NaN margin on each side of every output (256 bytes: keeps 16-byte alignment)
EPS = float(np.float32(1e-5))
LEAKY, TANH, NONE = 1, 2, 0
ROW_IDS = [c.id for c in bc.ROW_CASES]
FLOAT_IDS = [c.id for c in bc.ROW_CASES if c.float_leg]
WIDE_IDS = [c.id for c in bc.WIDE_CASES]
# mask variants: ("in", "out") = (mask_in, mask_post) for bn_apply, (mask_in, mask_pre) for bn_bwd, mask for bn_stats
MASKS = {"none": (False, False), "in": (True, False), "out": (False, True), "both": (True, True)}
SLOPE = {"none": -1.0, "in": 0.0, "out": 0.1, "both": 0.1}   # leaky' of bn_bwd per mask variant (-1: none)


def _ops():
    from ali_hip import ops
    return ops


def _lib():
    from ali_hip import _lib
    return _lib


def f32(v):
    return float(np.float32(v))


def mask_variants(c):
    return ("both",) if c.capped else tuple(MASKS)


# ----------------------------------------------------------------------------------------------------------------------
# host side (no GPU)

@pytest.mark.parametrize("cid", ROW_IDS + WIDE_IDS)
def test_case_takes_its_route(cid):
    """ops.ew_plan names the case's route and the block counts the formulas give, for every entry the case feeds; the
    capped cases sit above both caps; misaligned operands take the scalar route"""
    ops, c = _ops(), bc.ALL[cid]
    ents = ("bn_apply", "bn_bwd_from_partials") + (("bn_stats", "bn_bwd") if c.C <= 256 else ())
    for op in ents:
        g = c.groups if op in ("bn_stats", "bn_apply") else 1
        rows = c.rows if g > 1 else c.B * c.rpi
        got = ops.ew_plan(op, rows, c.rpi, c.C, groups=g)
        assert got == bc.plan(op, rows, c.rpi, c.C, groups=g), (cid, op, got)
        assert got[0] == c.route, (cid, op, got)
        assert ops.ew_plan(op, rows, c.rpi, c.C, groups=g, aligned=False)[0] == "scalar", (cid, op)
    for op in ("bn_stats", "bn_bwd"):
        if c.C > 256:
            assert ops.ew_plan(op, c.B * c.rpi, c.rpi, c.C) is None, (cid, op)
    if c.capped:
        vec = c.route == "vec"
        assert bc.raw_reduce_blocks(c.rows, c.C, vec) > bc.REDUCE_CAP
        assert ops.ew_plan("bn_stats", c.rows, c.rpi, c.C)[1] == bc.REDUCE_CAP
        assert bc.raw_ew_blocks(c.rows * c.C, vec) > bc.EW_GRID_CAP
        assert ops.ew_plan("bn_apply", c.rows, c.rpi, c.C)[2] == bc.EW_GRID_CAP
        if vec:     # several trips of the four-rows-in-flight loop, the last one ragged
            stride = 512 * bc.lanes_r(c.C, True)
            assert c.rows > 4 * stride and c.rows % (4 * stride) != 0 and c.rpi % 2 == 1
    else:
        for op in ents:
            _, nb, ew = ops.ew_plan(op, c.rows, c.rpi, c.C, groups=c.groups if op in ("bn_stats", "bn_apply") else 1)
            assert nb < bc.REDUCE_CAP and ew < bc.EW_GRID_CAP, (cid, op)
    lr = {"v-c8": 128, "v-c12": 85, "v-c256": 4, "s-c6": 32, "s-c1": 256, "s-c255": 1, "w-c768": 1, "w-c1024": 1}
    if cid in lr:
        assert bc.lanes_r(c.C, c.route == "vec") == lr[cid], cid


@pytest.mark.parametrize("case", bc.COLSUM_CASES, ids=[k[0] for k in bc.COLSUM_CASES])
def test_colsum_case_takes_its_route(case):
    cid, rows, C, ld, aligned, route = case
    got = _ops().ew_plan("colsum", rows, 1, C, ld=ld, aligned=aligned)
    assert got == bc.plan("colsum", rows, 1, C, ld=ld, aligned=aligned) and got[0] == route, (cid, got)
    assert got[2] == 0 and (got[1] == bc.REDUCE_CAP) == cid.startswith("c-cap"), (cid, got)
    if cid.startswith("c-cap"):
        assert bc.raw_reduce_blocks(rows, C, route == "vec") > bc.REDUCE_CAP


def test_act_bwd_and_refusals():
    ops = _ops()
    for n in bc.ACT_N:
        assert ops.ew_plan("act_bwd", n, 1, 1) == bc.plan("act_bwd", n, 1, 1), n
    assert ops.ew_plan("act_bwd", bc.EW_CAP + 3, 1, 1)[2] == bc.EW_GRID_CAP
    assert ops.ew_plan("bn_stats", 10, 1, 257) is None and ops.ew_plan("bn_bwd", 10, 1, 260) is None
    assert ops.ew_plan("bn_apply", 10, 1, 1028) == ("scalar", 0, 41)
    assert ops.ew_plan("colsum", 10, 1, 8, ld=7) is None
    assert ops.ew_plan("bn_bwd", 10, 1, 8, groups=2) is None          # groups are for stats and apply only
    assert ops.ew_plan("bn_stats", 0, 1, 8) is None


# ----------------------------------------------------------------------------------------------------------------------
# inputs and fp64 references (CPU)

def int_inputs(c, seed, masks=(True, True)):
    """exact leg: x, g integers in [-3, 3], per-image masks in {0, 2} (per group: [B, C]), planted integer means and
    invstd in {0.5, 1, 2}, power-of-two gamma / sc, integer beta / sh"""
    gen = torch.Generator().manual_seed(seed)
    n = c.B * c.rpi
    x = torch.randint(-3, 4, (n, c.C), generator=gen).float()
    g = torch.randint(-3, 4, (n, c.C), generator=gen).float()
    m1 = (torch.randint(0, 2, (c.B, c.C), generator=gen) * 2).float() if masks[0] else None
    m2 = (torch.randint(0, 2, (c.B, c.C), generator=gen) * 2).float() if masks[1] else None
    p2 = torch.tensor([0.5, 1.0, 2.0])
    d = dict(x=x, g=g, m_in=m1, m_out=m2,
             mean=torch.randint(-2, 3, (c.C,), generator=gen).float(),
             invstd=p2[torch.randint(0, 3, (c.C,), generator=gen)],
             gamma=p2[torch.randint(0, 3, (c.C,), generator=gen)]
             * (torch.randint(0, 2, (c.C,), generator=gen) * 2 - 1),
             beta=torch.randint(-3, 4, (c.C,), generator=gen).float())
    d["sc"] = p2[torch.randint(0, 3, (c.groups, c.C), generator=gen)]
    d["sh"] = torch.randint(-3, 4, (c.groups, c.C), generator=gen).float()
    return d


def float_inputs(c, seed, masks=(True, True)):
    """float leg, as the older test: LeakyReLU(2 randn + 0.5), masks in {0, 2}, random gamma, beta, running stats; the
    backward's statistics are the batch's own"""
    gen = torch.Generator().manual_seed(seed)
    n = c.B * c.rpi
    x = torch.nn.functional.leaky_relu(torch.randn(n, c.C, generator=gen) * 2 + 0.5, 0.1)
    g = torch.randn(n, c.C, generator=gen)
    m1 = (torch.rand(c.B, c.C, generator=gen) > 0.5).float() * 2 if masks[0] else None
    m2 = (torch.rand(c.B, c.C, generator=gen) > 0.5).float() * 2 if masks[1] else None
    xm = x.double() * (m1.double().repeat_interleave(c.rpi, 0) if m1 is not None else 1)
    mu, var = xm.mean(0), xm.var(0, unbiased=False)
    d = dict(x=x, g=g, m_in=m1, m_out=m2, mean=mu.float(), invstd=(1 / torch.sqrt(var + EPS)).float(),
             gamma=torch.rand(c.C, generator=gen) + 0.5, beta=torch.randn(c.C, generator=gen),
             rm=torch.randn(c.C, generator=gen), rv=torch.rand(c.C, generator=gen) * 1.5 + 0.5,
             sc=torch.randn(c.groups, c.C, generator=gen), sh=torch.randn(c.groups, c.C, generator=gen))
    return d


def per_row(mask, rpi):
    """[B, C] image mask -> [B * rpi, C] fp64 (1 where absent)"""
    return None if mask is None else mask.double().repeat_interleave(rpi, 0)


def stat_sums(c, x, m_in, drop=False):
    """per group and channel: (s1, s2, sum|x~|) of x~ = x * mask in fp64; ``drop``: the planted bug -- row rpi // 2 of
    the first image of group 0 left out"""
    xm = x.double() * (per_row(m_in, c.rpi) if m_in is not None else 1)
    xm = xm.view(c.groups, c.rows, c.C)
    if drop:
        xm = xm.clone()
        xm[0, c.rpi // 2] = 0
    return xm.sum(1), (xm * xm).sum(1), xm.abs().sum(1)


def stats_ref(c, s1, s2, e1, e2, gamma, beta, rm, rv, mom, training=True):
    """fp64 statement of bn_stats_final_kernel per group (running stats in group order) with error bounds: e1, e2 the
    bounds of the sums s1, s2 (0 in the exact leg).  Returns dict of [groups, C] references and bounds."""
    G, C, count = c.groups, c.C, c.rows
    one = torch.ones(C, dtype=torch.float64)
    gm = gamma.double() if gamma is not None else one
    bt = beta.double() if beta is not None else 0 * one
    out = {k: [] for k in ("mean", "e_mean", "var", "e_var", "unb", "e_unb", "invstd", "e_invstd", "sc", "e_sc", "sh",
                           "e_sh", "rm", "e_rm", "rv", "e_rv")}
    rmr = rm.double() if rm is not None else None
    rvr = rv.double() if rv is not None else None
    erm = ervs = 0 * one
    for gi in range(G):
        if training:
            m = s1[gi] / count
            em_d = e1[gi] / count + 2 * UD * m.abs()                        # double divide
            v_raw = s2[gi] / count - m * m
            ev_d = e2[gi] / count + (2 * m.abs() + em_d) * em_d + 4 * UD * (s2[gi] / count + m * m)
            v = v_raw.clamp(min=0)
            unb = v * count / (count - 1) if count > 1 else v
            eunb = ev_d * (count / (count - 1) if count > 1 else 1) + U * unb.abs()   # (float)unb in the blend
            em = em_d + U * m.abs()                                           # (float)mean
            ev = ev_d + U * v.abs()                                           # (float)var
        else:
            m, v, em, ev, unb, eunb = rm.double(), rv.double(), 0 * one, 0 * one, rv.double(), 0 * one
        out["mean"].append(m), out["e_mean"].append(em), out["var"].append(v), out["e_var"].append(ev)
        out["unb"].append(unb), out["e_unb"].append(eunb)
        # invstd = 1 / sqrtf(var + eps): the add, the sqrt, the divide: k = 3, one spare; plus the var error propagated
        # (d invstd / d var = -invstd / (2 (var + eps)); second order: var's bound is far below var + eps here)
        ist = 1 / torch.sqrt(v + EPS)
        eis = 0.5 * ist * ev / (v + EPS) * 1.01 + 4 * U * ist
        # sc = g * invstd: one multiply, k = 1 + 1
        sc = gm * ist
        esc = gm.abs() * eis + 2 * U * sc.abs()
        # sh = b - mean * g * invstd: two multiplies and the subtract, k = 3 + 1
        t = m * gm * ist
        sh = bt - t
        esh = gm.abs() * (ist * em + m.abs() * eis) + 4 * U * (bt.abs() + t.abs())
        out["invstd"].append(ist), out["e_invstd"].append(eis), out["sc"].append(sc), out["e_sc"].append(esc)
        out["sh"].append(sh), out["e_sh"].append(esh)
        if training and rmr is not None:
            # r = (1 - mom) * r + mom * new: 1 - mom, two multiplies, the add: k = 4 + 1; the previous pass's error
            # carries with weight 1 - mom
            a = 1 - mom
            erm = a * erm + mom * em + 5 * U * (abs(a) * rmr.abs() + mom * m.abs())
            ervs = a * ervs + mom * eunb + 5 * U * (abs(a) * rvr.abs() + mom * unb.abs())
            rmr = a * rmr + mom * m
            rvr = a * rvr + mom * unb
        out["rm"].append(rmr if rmr is not None else 0 * one), out["e_rm"].append(erm)
        out["rv"].append(rvr if rvr is not None else 0 * one), out["e_rv"].append(ervs)
    return {k: torch.stack(v) for k, v in out.items()}


def bwd_sums(c, x, g, m_in, m_pre, mean, invstd, drop=False):
    """(sum g~ * xhat, sum g~, sum |g~ * xhat|, sum |g~|) per channel in fp64 (one group)"""
    mi, mp = per_row(m_in, c.rpi), per_row(m_pre, c.rpi)
    xv = x.double() * (mi if mi is not None else 1)
    gv = g.double() * (mp if mp is not None else 1)
    if drop:
        gv = gv.clone()
        gv[c.rpi // 2] = 0
    t = gv * (xv - mean.double()) * invstd.double()
    return t.sum(0), gv.sum(0), t.abs().sum(0), gv.abs().sum(0)


def gx_ref(c, x, g, m_in, m_pre, mean, invstd, gamma, dgamma, dbeta, batch_stats, slope):
    """fp64 statement of bn_bwd_apply_kernel from the device's own dgamma / dbeta, with its bound.  Roundings counted in
    r = (g~ - (db + (x~ - mu) * is * dg) * ic) * (gm * is) * mi * leaky': ic = 1 / rows, the subtract, two multiplies,
    the add, * ic, g~ -, gm * is, the product, * slope: k = 10, one spare; eval: gm * is, the product, * slope:
    k = 3 + 1"""
    rows = c.B * c.rpi
    mi, mp = per_row(m_in, c.rpi), per_row(m_pre, c.rpi)
    xr = x.double()
    xv = xr * (mi if mi is not None else 1)
    gv = g.double() * (mp if mp is not None else 1)
    is_, mu, dg, db = invstd.double(), mean.double(), dgamma.double().cpu(), dbeta.double().cpu()
    gm = gamma.double() if gamma is not None else torch.ones(c.C, dtype=torch.float64)
    ic = 1.0 / rows
    if batch_stats:
        a = (xv - mu) * is_ * dg
        r = gv - (db + a) * ic
        terms = gv.abs() + (db.abs() + a.abs()) * ic
        k = 11
    else:
        r, terms, k = gv, gv.abs(), 4
    scale = gm * is_ * (mi if mi is not None else 1)
    if slope >= 0:
        scale = scale * torch.where(xr > 0, torch.ones_like(xr), torch.full_like(xr, f32(slope)))
    return r * scale, k * U * terms * scale.abs()


# ----------------------------------------------------------------------------------------------------------------------
# device calls: every output inside a NaN-filled buffer

def _dev():
    return torch.device("cuda")


class Slot:
    """``n`` floats at ``PAD + shift`` of a NaN-filled buffer; ``margins_nan()`` after the launch"""

    def __init__(self, shape, shift=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD + 4,), float("nan"), device=_dev())
        self.lo, self.n = PAD + shift, n
        self.t = self.buf[self.lo:self.lo + n].view(*shape)

    def margins_nan(self):
        b = self.buf.cpu()
        return bool(torch.isnan(b[:self.lo]).all() and torch.isnan(b[self.lo + self.n:]).all())


_KEEP = []      # device copies handed to the library as raw pointers: alive until call() has synchronised


def dev_in(t, shift=0):
    """a contiguous device copy of ``t`` starting ``shift`` floats into a larger buffer (shift 1: 4 bytes off 16)"""
    if t is None:
        return None
    buf = torch.zeros(t.numel() + PAD, device=_dev())
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    _KEEP.append(v)
    return v


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def call(name, *args):
    lib = _lib().load()
    _lib().check(getattr(lib, name)(*args), name)
    torch.cuda.synchronize()
    _KEEP.clear()


def ws():
    w = _ops().workspace(_dev())
    return c_void_p(w.data_ptr()), w.numel()


def stream():
    return _ops()._stream()


def run_stats(c, d, masked, training=True, mom=0.5, affine=True, running=True, rm0=None, rv0=None, shift=0):
    """ali_bn_stats on a case: returns (st [groups, 4, C] cpu, rm, rv cpu or None); outputs' margins checked"""
    st = Slot((c.groups, 4, c.C))
    x = dev_in(d["x"], shift)
    mask = dev_in(d["m_in"]) if masked else None
    rm = Slot((c.C,)) if running else None
    rv = Slot((c.C,)) if running else None
    if running:
        rm.t.copy_(rm0 if rm0 is not None else torch.zeros(c.C))
        rv.t.copy_(rv0 if rv0 is not None else torch.zeros(c.C))
    gam, bet = (dev_in(d["gamma"]), dev_in(d["beta"])) if affine else (None, None)
    call("ali_bn_stats", P(x), P(mask), c.B, c.rpi, c.C, P(gam), P(bet), P(rm and rm.t), P(rv and rv.t), f32(mom), EPS,
         int(training), P(st.t[0, 0]), P(st.t[0, 1]), P(st.t[0, 2]), P(st.t[0, 3]), c.groups, 4 * c.C, *ws(), stream())
    torch.cuda.synchronize()
    assert st.margins_nan() and (not running or (rm.margins_nan() and rv.margins_nan())), "write outside the outputs"
    return st.t.cpu(), (rm.t.cpu() if running else None), (rv.t.cpu() if running else None)


def run_apply(c, x, sc, sh, m_in, m_post, shift=(0, 0, 0)):
    """ali_bn_apply with [groups, 4, C] statistics (sc, sh in rows 2, 3); shift = (x, mask_in, out) in floats"""
    st = torch.full((c.groups, 4, c.C), float("nan"))
    st[:, 2], st[:, 3] = sc, sh
    st = st.to(_dev())
    out = Slot(tuple(x.shape), shift[2])
    call("ali_bn_apply", P(dev_in(x, shift[0])), P(st[0, 2]), P(st[0, 3]), P(dev_in(m_in, shift[1])), P(dev_in(m_post)),
         P(out.t), c.B, c.rpi, c.C, c.groups, 4 * c.C, stream())
    torch.cuda.synchronize()
    assert out.margins_nan(), "bn_apply wrote outside its output"
    return out.t.cpu()


def run_bwd(c, d, m_in, m_pre, batch_stats, slope, want_gx=True, affine=True, shift=(0, 0, 0), part=None, slots=0):
    """ali_bn_bwd (or, with ``part``, ali_bn_bwd_from_partials): (dgamma, dbeta, gx or None) on the CPU"""
    dg, db = Slot((c.C,)), Slot((c.C,))
    gx = Slot(tuple(d["x"].shape), shift[2]) if want_gx else None
    gam = dev_in(d["gamma"]) if affine else None
    args = (P(dev_in(d["x"], shift[0])), P(dev_in(d["g"])), P(dev_in(m_in, shift[1])), P(dev_in(m_pre)),
            P(dev_in(d["mean"])), P(dev_in(d["invstd"])), P(gam), c.B, c.rpi, c.C, int(batch_stats), f32(slope),
            P(dg.t), P(db.t), P(gx and gx.t))
    if part is None:
        call("ali_bn_bwd", *args, *ws(), stream())
    else:
        call("ali_bn_bwd_from_partials", P(part), slots, *args, stream())
    torch.cuda.synchronize()
    assert dg.margins_nan() and db.margins_nan() and (gx is None or gx.margins_nan()), "write outside the outputs"
    return dg.t.cpu(), db.t.cpu(), (gx.t.cpu() if want_gx else None)


def within(got, ref, bound, what):
    err = (got.double() - ref.double()).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"err/bound {what}: {ratio:.3e}")
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} out of bound, worst excess "
                           f"{(err - bound)[bad].max().item():.3e}")
    return ratio


def assert_within(got, ref, bound, buggy, what):
    """within(), after asserting on the CPU that the planted-bug reference violates the same bound somewhere"""
    assert ((buggy.double() - ref.double()).abs() > bound).any(), \
        f"{what}: the bound does not tell the planted bug apart"
    return within(got, ref, bound, what)


def ulp1(got, ref, what):
    r32 = ref.float().numpy()
    sp = torch.from_numpy(np.spacing(np.abs(r32)).astype(np.float64))
    within(got, ref, sp, what)


def exact_sum_guard(*abs_sums):
    for a in abs_sums:
        assert float(a.max()) < 2 ** 23, "the exact leg's inputs would round"


# ----------------------------------------------------------------------------------------------------------------------
# bn_stats

def check_stats_exact(c, d, st, rm, rv, masked, mom=0.5):
    s1, s2, a1 = stat_sums(c, d["x"], d["m_in"] if masked else None)
    exact_sum_guard(a1, s2)
    z = torch.zeros(c.C)
    r = stats_ref(c, s1, s2, 0 * s1, 0 * s2, d["gamma"], d["beta"], z, z, f32(mom))
    assert torch.equal(st[:, 0], r["mean"].float()), f"{c.id}: mean"
    within(st[:, 1], r["invstd"], r["e_invstd"], f"{c.id}: invstd")
    within(st[:, 2], r["sc"], r["e_sc"], f"{c.id}: sc")
    within(st[:, 3], r["sh"], r["e_sh"], f"{c.id}: sh")
    if rm is not None:
        # the first pass blends into zeros with momentum 0.5: it stores exactly half of (float)mean and (float)unb
        if c.groups == 1:
            assert torch.equal(rm, 0.5 * r["mean"][0].float()), f"{c.id}: running_mean"
            ulp1(2 * rv, r["unb"][0], f"{c.id}: unbiased running_var")
        within(rm, r["rm"][-1], r["e_rm"][-1], f"{c.id}: running_mean after {c.groups} passes")
        within(rv, r["rv"][-1], r["e_rv"][-1], f"{c.id}: running_var after {c.groups} passes")


@gpu
@pytest.mark.parametrize("cid,masked",
                         [(i, m) for i in ROW_IDS for m in ((True,) if bc.ALL[i].capped else (False, True))])
def test_bn_stats_exact(cid, masked):
    c = bc.ALL[cid]
    d = int_inputs(c, 11)
    st, rm, rv = run_stats(c, d, masked)
    check_stats_exact(c, d, st, rm, rv, masked)


def float_stats_refs(c, d, masked, mom):
    m_in = d["m_in"] if masked else None
    s1, s2, a1 = stat_sums(c, d["x"], m_in)
    b1, b2, _ = stat_sums(c, d["x"], m_in, drop=True)
    L = c.rows
    e1, e2 = L * U * a1, L * U * s2
    args = (d["gamma"], d["beta"], d["rm"], d["rv"], f32(mom))
    return stats_ref(c, s1, s2, e1, e2, *args), stats_ref(c, b1, b2, e1, e2, *args)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("cid", FLOAT_IDS)
def test_float_bounds_catch_the_planted_bug(cid, masked):
    """host side of the float leg: one row of an unmasked image dropped moves mean and invstd (bn_stats) and dgamma and
    dbeta (bn_bwd) out of their bounds -- the bounds can fail"""
    c = bc.ALL[cid]
    d = float_inputs(c, 5)
    r, b = float_stats_refs(c, d, masked, 0.1)
    for k in ("mean", "invstd"):
        assert ((b[k] - r[k]).abs() > r["e_" + k]).any(), (cid, k)
    if c.groups == 1:
        m_in, m_pre = (d["m_in"], d["m_out"]) if masked else (None, None)
        t1, t2, a1, a2 = bwd_sums(c, d["x"], d["g"], m_in, m_pre, d["mean"], d["invstd"])
        u1, u2, _, _ = bwd_sums(c, d["x"], d["g"], m_in, m_pre, d["mean"], d["invstd"], drop=True)
        L = c.rows
        assert ((u1 - t1).abs() > L * U * a1).any() and ((u2 - t2).abs() > L * U * a2).any(), cid


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("cid", FLOAT_IDS)
def test_bn_stats_float(cid, masked):
    c = bc.ALL[cid]
    d = float_inputs(c, 5)
    r, b = float_stats_refs(c, d, masked, 0.1)
    st, rm, rv = run_stats(c, d, masked, mom=0.1, rm0=d["rm"], rv0=d["rv"])
    assert_within(st[:, 0], r["mean"], r["e_mean"], b["mean"], f"{cid}: mean")
    assert_within(st[:, 1], r["invstd"], r["e_invstd"], b["invstd"], f"{cid}: invstd")
    within(st[:, 2], r["sc"], r["e_sc"], f"{cid}: sc")
    within(st[:, 3], r["sh"], r["e_sh"], f"{cid}: sh")
    within(rm, r["rm"][-1], r["e_rm"][-1], f"{cid}: running_mean")
    within(rv, r["rv"][-1], r["e_rv"][-1], f"{cid}: running_var")


@gpu
@pytest.mark.parametrize("variant", ["eval", "no-affine", "no-running", "count1-eval"])
def test_bn_stats_corners(variant):
    """training = 0 (running stats in, nothing reduced or updated), gamma and beta absent, running stats absent in
    training"""
    c = bc.ALL["n1-s3" if variant == "count1-eval" else "v-c64"]
    d = int_inputs(c, 12)
    if variant in ("eval", "count1-eval"):
        rm0, rv0 = d["mean"], d["invstd"] * 3               # integers and 1.5, 3, 6: exact inputs
        st, rm, rv = run_stats(c, d, True, training=False, rm0=rm0, rv0=rv0)
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0), "eval mode changed the running stats"
        r = stats_ref(c, None, None, None, None, d["gamma"], d["beta"], rm0, rv0, 0.5, training=False)
        assert torch.equal(st[:, 0], rm0[None]), "eval mean"
        within(st[:, 1], r["invstd"], r["e_invstd"], "eval invstd")
        within(st[:, 2], r["sc"], r["e_sc"], "eval sc")
        within(st[:, 3], r["sh"], r["e_sh"], "eval sh")
        return
    affine = variant != "no-affine"
    st, rm, rv = run_stats(c, d, True, affine=affine, running=variant != "no-running")
    if not affine:
        d = dict(d, gamma=None, beta=None)
    check_stats_exact(c, d, st, rm, rv, True)


# ----------------------------------------------------------------------------------------------------------------------
# bn_apply

def apply_ref(c, x, sc, sh, m_in, m_post):
    """out = (x * mi * sc + sh) * mp per group; masks exact ({0, 2}); x~ * sc and + sh: k = 2 (contracted or not)"""
    G = c.groups
    xv = x.double() * (per_row(m_in, c.rpi) if m_in is not None else 1)
    mp = per_row(m_post, c.rpi) if m_post is not None else torch.ones_like(xv)
    scr = sc.double().repeat_interleave(c.rows, 0) if G > 1 else sc.double().expand(xv.shape[0], -1)
    shr = sh.double().repeat_interleave(c.rows, 0) if G > 1 else sh.double().expand(xv.shape[0], -1)
    return (xv * scr + shr) * mp, 2 * U * ((xv * scr).abs() + shr.abs()) * mp.abs()


@gpu
@pytest.mark.parametrize("cid,masks", [(i, m) for i in ROW_IDS + WIDE_IDS for m in mask_variants(bc.ALL[i])])
def test_bn_apply(cid, masks):
    c = bc.ALL[cid]
    mi, mo = MASKS[masks]
    d = int_inputs(c, 13, (mi, mo))
    ref, _ = apply_ref(c, d["x"], d["sc"], d["sh"], d["m_in"], d["m_out"])
    out = run_apply(c, d["x"], d["sc"], d["sh"], d["m_in"], d["m_out"])
    assert torch.equal(out, ref.float()), f"{cid}: exact bn_apply"
    if c.rows * c.groups <= 600:
        d = float_inputs(c, 14, (mi, mo))
        ref, bound = apply_ref(c, d["x"], d["sc"], d["sh"], d["m_in"], d["m_out"])
        within(run_apply(c, d["x"], d["sc"], d["sh"], d["m_in"], d["m_out"]), ref, bound, f"{cid}: float bn_apply")


# ----------------------------------------------------------------------------------------------------------------------
# bn_bwd

BWD_IDS = [i for i in ROW_IDS if bc.ALL[i].groups == 1]


@gpu
@pytest.mark.parametrize("cid,masks", [(i, m) for i in BWD_IDS for m in mask_variants(bc.ALL[i])])
def test_bn_bwd_exact(cid, masks):
    c = bc.ALL[cid]
    mi, mp = MASKS[masks]
    d = int_inputs(c, 15, (mi, mp))
    slope = SLOPE[masks]
    t1, t2, a1, a2 = bwd_sums(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"])
    exact_sum_guard(a1, a2)
    dg, db, gx = run_bwd(c, d, d["m_in"], d["m_out"], True, slope)
    assert torch.equal(dg, t1.float()) and torch.equal(db, t2.float()), f"{cid}: dgamma / dbeta"
    ref, bound = gx_ref(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"], d["gamma"], dg, db, True,
                        slope)
    within(gx, ref, bound, f"{cid}: gx")


@gpu
@pytest.mark.parametrize("masks", ["none", "both"])
@pytest.mark.parametrize("cid", [i for i in FLOAT_IDS if bc.ALL[i].groups == 1])
def test_bn_bwd_float(cid, masks):
    c = bc.ALL[cid]
    mi, mp = MASKS[masks]
    d = float_inputs(c, 16, (mi, mp))
    t1, t2, a1, a2 = bwd_sums(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"])
    u1, u2, _, _ = bwd_sums(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"], drop=True)
    dg, db, gx = run_bwd(c, d, d["m_in"], d["m_out"], True, 0.1)
    L = c.rows
    assert_within(dg, t1, L * U * a1, u1, f"{cid}: dgamma")
    assert_within(db, t2, L * U * a2, u2, f"{cid}: dbeta")
    ref, bound = gx_ref(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"], d["gamma"], dg, db, True, 0.1)
    within(gx, ref, bound, f"{cid}: gx")


@gpu
@pytest.mark.parametrize("variant", ["eval", "no-gx", "no-gamma", "count1"])
def test_bn_bwd_corners(variant):
    """batch_stats = 0, want_gx = False (nothing written), gamma absent, count = 1 on both routes"""
    for cid in (("n1-v4", "n1-s3") if variant == "count1" else ("v-c64", "s-c6")):
        c = bc.ALL[cid]
        d = int_inputs(c, 17)
        if variant == "no-gamma":
            d["gamma"] = None
        bs = variant != "eval"
        dg, db, gx = run_bwd(c, d, d["m_in"], d["m_out"], bs, 0.1, want_gx=variant != "no-gx",
                             affine=variant != "no-gamma")
        t1, t2, _, _ = bwd_sums(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"])
        assert torch.equal(dg, t1.float()) and torch.equal(db, t2.float()), f"{cid} {variant}: dgamma / dbeta"
        if gx is not None:
            ref, bound = gx_ref(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"], d["gamma"], dg, db,
                                bs, 0.1)
            within(gx, ref, bound, f"{cid} {variant}: gx")


# ----------------------------------------------------------------------------------------------------------------------
# alignment fallback: (7, 25, 64) with one operand 4 bytes off a 16-byte boundary

@gpu
@pytest.mark.parametrize("which", ["x", "mask", "out"])
def test_alignment_fallback(which):
    """the scalar kernels take over (ops.ew_plan with aligned=False says so) and give the exact leg's results bit for
    bit; gx holds its bound on both routes"""
    c = bc.ALL["v-c64"]
    ops = _ops()
    for op in ("bn_stats", "bn_apply", "bn_bwd"):
        assert ops.ew_plan(op, c.rows, c.rpi, c.C, aligned=False)[0] == "scalar"
    d = int_inputs(c, 18)
    sh = {"x": (1, 0, 0), "mask": (0, 1, 0), "out": (0, 0, 1)}[which]
    if which != "out":      # bn_stats names x and its mask only
        st_a, rm_a, rv_a = run_stats(c, d, True)
        if which == "x":
            st_m, rm_m, rv_m = run_stats(c, d, True, shift=1)
        else:
            st_m, rm_m, rv_m = _stats_mask_shifted(c, d)
        assert torch.equal(st_a, st_m) and torch.equal(rm_a, rm_m) and torch.equal(rv_a, rv_m), "bn_stats"
        check_stats_exact(c, d, st_m, rm_m, rv_m, True)
    a = run_apply(c, d["x"], d["sc"], d["sh"], d["m_in"], d["m_out"])
    m = run_apply(c, d["x"], d["sc"], d["sh"], d["m_in"], d["m_out"], shift=sh)
    assert torch.equal(a, m), "bn_apply"
    dga, dba, gxa = run_bwd(c, d, d["m_in"], d["m_out"], True, 0.1)
    dgm, dbm, gxm = run_bwd(c, d, d["m_in"], d["m_out"], True, 0.1, shift=sh)
    assert torch.equal(dga, dgm) and torch.equal(dba, dbm), "bn_bwd dgamma / dbeta"
    for gx, dg, db in ((gxa, dga, dba), (gxm, dgm, dbm)):
        ref, bound = gx_ref(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"], d["gamma"], dg, db, True,
                            0.1)
        within(gx, ref, bound, f"gx ({which} shifted)")


def _stats_mask_shifted(c, d):
    st = Slot((c.groups, 4, c.C))
    rm, rv = Slot((c.C,)), Slot((c.C,))
    rm.t.zero_(), rv.t.zero_()
    call("ali_bn_stats", P(dev_in(d["x"])), P(dev_in(d["m_in"], 1)), c.B, c.rpi, c.C, P(dev_in(d["gamma"])),
         P(dev_in(d["beta"])), P(rm.t), P(rv.t), 0.5, EPS, 1, P(st.t[0, 0]), P(st.t[0, 1]), P(st.t[0, 2]),
         P(st.t[0, 3]), 1, 4 * c.C, *ws(), stream())
    torch.cuda.synchronize()
    assert st.margins_nan() and rm.margins_nan() and rv.margins_nan()
    return st.t.cpu(), rm.t.cpu(), rv.t.cpu()


# ----------------------------------------------------------------------------------------------------------------------
# the two finals fed by [2][C][slots] partials

def partials(slots, C, seed):
    """integer partials: s1 in [-20, 20], s2 >= s1^2 in [0, 420]: exact in any order"""
    gen = torch.Generator().manual_seed(seed)
    s1 = torch.randint(-20, 21, (C, slots), generator=gen).float()
    s2 = s1 * s1 + torch.randint(0, 21, (C, slots), generator=gen).float()
    return torch.stack([s1, s2])


@gpu
@pytest.mark.parametrize("slots", bc.FROM_PARTIALS_SLOTS)
def test_bn_stats_from_partials(slots):
    C = 6
    for groups in (1, 2, 3):
        if slots % groups:
            continue
        per = slots // groups
        c = bc.Case("part", groups * 4 * per, 1, C, "scalar", groups=groups)   # count = 4 rows per slot of a group
        part = partials(slots, C, slots + groups)
        s1 = part[0].double().view(C, groups, per).sum(2).T
        s2 = part[1].double().view(C, groups, per).sum(2).T
        d = int_inputs(c, 19)
        st = Slot((groups, 4, C))
        rm, rv = Slot((C,)), Slot((C,))
        rm.t.zero_(), rv.t.zero_()
        call("ali_bn_stats_from_partials", P(dev_in(part)), slots, groups, C, c.rows, P(dev_in(d["gamma"])),
             P(dev_in(d["beta"])), P(rm.t), P(rv.t), 0.5, EPS, P(st.t[0, 0]), P(st.t[0, 1]), P(st.t[0, 2]),
             P(st.t[0, 3]), 4 * C, stream())
        torch.cuda.synchronize()
        assert st.margins_nan() and rm.margins_nan() and rv.margins_nan(), "write outside the outputs"
        z = torch.zeros(C)
        r = stats_ref(c, s1, s2, 0 * s1, 0 * s2, d["gamma"], d["beta"], z, z, 0.5)
        got = st.t.cpu()
        what = f"slots {slots} groups {groups}"
        assert torch.equal(got[:, 0], r["mean"].float()), what + ": mean"
        within(got[:, 1], r["invstd"], r["e_invstd"], what + ": invstd")
        within(got[:, 2], r["sc"], r["e_sc"], what + ": sc")
        within(got[:, 3], r["sh"], r["e_sh"], what + ": sh")
        if groups == 1:
            ulp1(2 * rv.t.cpu(), r["unb"][0], what + ": unbiased running_var")
        within(rm.t.cpu(), r["rm"][-1], r["e_rm"][-1], what + ": running_mean")
        within(rv.t.cpu(), r["rv"][-1], r["e_rv"][-1], what + ": running_var")


@gpu
@pytest.mark.parametrize("slots", bc.FROM_PARTIALS_SLOTS)
def test_bn_bwd_from_partials(slots):
    """dgamma / dbeta are the exact sums of the slots at C = 512 (vec gx pass); gx holds its bound"""
    c = bc.Case("part", 5, 8, 512, "vec")
    part = partials(slots, c.C, 100 + slots)
    d = int_inputs(c, 20)
    dg, db, gx = run_bwd(c, d, d["m_in"], d["m_out"], True, 0.1, part=dev_in(part), slots=slots)
    assert torch.equal(dg, part[0].double().sum(1).float()) and torch.equal(db, part[1].double().sum(1).float())
    ref, bound = gx_ref(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"], d["gamma"], dg, db, True, 0.1)
    within(gx, ref, bound, f"slots {slots}: gx")


@gpu
@pytest.mark.parametrize("cid", WIDE_IDS)
def test_bn_bwd_from_partials_wide(cid):
    """the gx pass of ali_bn_bwd_from_partials beyond 256 channels, both routes, exact and float inputs"""
    c = bc.ALL[cid]
    for leg in ("exact", "float"):
        d = int_inputs(c, 21) if leg == "exact" else float_inputs(c, 22)
        part = partials(257, c.C, 23)
        dg, db, gx = run_bwd(c, d, d["m_in"], d["m_out"], True, 0.1, part=dev_in(part), slots=257)
        assert torch.equal(dg, part[0].double().sum(1).float()) and torch.equal(db, part[1].double().sum(1).float())
        ref, bound = gx_ref(c, d["x"], d["g"], d["m_in"], d["m_out"], d["mean"], d["invstd"], d["gamma"], dg, db, True,
                            0.1)
        within(gx, ref, bound, f"{cid} {leg}: gx")


# ----------------------------------------------------------------------------------------------------------------------
# ali_colsum, ali_act_bwd

@gpu
@pytest.mark.parametrize("case", bc.COLSUM_CASES, ids=[k[0] for k in bc.COLSUM_CASES])
def test_colsum(case):
    cid, rows, C, ld, aligned, _ = case
    gen = torch.Generator().manual_seed(rows + C)
    x = torch.randint(-3, 4, (rows, ld), generator=gen).float()
    x[:, C:] = float("nan")                       # the columns beyond C must not be read
    exact_sum_guard(x[:, :C].abs().sum(0))
    out = Slot((C,))
    xd = dev_in(x.reshape(-1), 0 if aligned else 1)
    call("ali_colsum", P(xd), rows, C, ld, P(out.t), *ws(), stream())
    torch.cuda.synchronize()
    assert out.margins_nan()
    assert torch.equal(out.t.cpu(), x[:, :C].double().sum(0).float()), cid


@gpu
@pytest.mark.parametrize("n", bc.ACT_N)
def test_act_bwd(n):
    gen = torch.Generator().manual_seed(n)
    gy = torch.randn(n, generator=gen)
    y = torch.randn(n, generator=gen)
    y[::7] = 0
    gyd, yd = dev_in(gy), dev_in(y)
    for act in (LEAKY, TANH, NONE):
        out = Slot((n,))
        call("ali_act_bwd", P(gyd), P(yd), P(out.t), n, act, f32(0.1), stream())
        torch.cuda.synchronize()
        assert out.margins_nan(), act
        got = out.t.cpu()
        if act == LEAKY:
            assert torch.equal(got, gy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, f32(0.1))))
        elif act == NONE:
            assert torch.equal(got, gy)
        else:   # gy * (1 - y * y): y * y, the subtract, the multiply: k = 3 + 1
            yd64, g64 = y.double(), gy.double()
            within(got, g64 * (1 - yd64 * yd64), 4 * U * g64.abs() * (1 + yd64 * yd64), "tanh act_bwd")
