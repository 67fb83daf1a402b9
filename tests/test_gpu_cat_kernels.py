"""ali_cat_nll and ali_cat_map (csrc/cat.hip) against the statement of attribute_scms/audio_mnist.py.

Continuous results (lp, out3, every gradient tensor, logits, noise) by the yardstick of tests/cat_cases.py: the fp64
statement on the CPU is the reference, the fp32 statement on the CPU the yardstick.  Discrete results (drawn, predicted
and differing classes, statuses) exactly, against the statement continued from the device's own stored logits, draws and
noise."""
import pytest
import torch

import cat_cases as cc

pytestmark = pytest.mark.gpu
_GRAPHS = {}


def _ops():
    from ali_hip import ops
    return ops


def _graphs(name):
    """(sizes, the fp32 CPU graph, its fp64 twin, theta and towers on the device), built once per name"""
    if name not in _GRAPHS:
        sizes = cc.CORNER if name == "corner" else cc.SIZES[name.replace("branchy-", "")]
        g32 = cc.branchy_graph(sizes) if name.startswith("branchy") else cc.new_graph(sizes, seed=len(name))
        g64 = cc.twin(g32, sizes, torch.float64)
        theta = torch.cat([p.detach().reshape(-1) for p in cc.trained_params(g32)]).cuda()
        towers = torch.cat([p.detach().reshape(-1) for m in cc.linears(g32)[4:12] for p in (m.weight, m.bias)]).cuda()
        _GRAPHS[name] = (sizes, g32, g64, theta, towers)
    return _GRAPHS[name]


def _dev(v):
    """a CPU tensor on the device; a column range of a wider table stays one"""
    if v._base is None:
        return v.cuda()
    off = v.storage_offset()
    return v._base.cuda()[:, off:off + v.shape[1]]


def _two_tile_rows():
    """the smallest N at which a block takes more than one row tile, read from the plan"""
    ops = _ops()
    big = ops.cat_plan(1 << 20, 13, 2, 17)
    n = big.grid * big.tile_rows + 1
    assert ops.cat_plan(n, 13, 2, 17).tiles_per_block == 2 and ops.cat_plan(n - 1, 13, 2, 17).tiles_per_block == 1
    return n


def _tile():
    return _ops().cat_plan(1, 5, 2, 6).tile_rows


NLL_CASES = [  # graph, contexts, rows ("tile-1" ...), wgt given, index given
    ("small", "onehot", 1, False, False),
    ("small", "dense", "tile-1", True, False),
    ("small", "strided", "tile+1", False, False),
    ("wide", "dense", 257, True, False),
    ("wide", "onehot", "two-tiles", False, False),
    ("wide", "strided", 257, True, True),
    ("small", "onehot", 70, False, True),
    ("corner", "onehot", "tile+1", True, False),
    ("branchy-small", "dense", 257, True, False),
    ("branchy-wide", "onehot", "tile+1", False, False),
]


@pytest.mark.parametrize("name,kind,rows,with_wgt,with_index", NLL_CASES)
def test_nll_against_the_statement(name, kind, rows, with_wgt, with_index):
    ops = _ops()
    sizes, g32, g64, theta, towers = _graphs(name)
    R = {"tile-1": _tile() - 1, "tile+1": _tile() + 1, "two-tiles": None}.get(rows, rows)
    R = _two_tile_rows() if R is None else R
    ctx = cc.contexts(sizes, R, kind)
    gen = torch.Generator().manual_seed(R)
    index = torch.randint(0, R, (R + 3,), generator=gen) if with_index else None           # repeats, another length
    N = R if index is None else index.numel()
    wgt = torch.randn(N, 2, generator=gen) if with_wgt else None
    gscale = -0.75
    w_stmt = gscale * (wgt.double() if with_wgt else torch.full((N, 2), 1.0 / N, dtype=torch.float64))   # as the kernel forms it
    rows_of = (lambda t: t if index is None else t[index])
    lp64, g64s = cc.statement_nll(g64, [rows_of(t) for t in ctx], w_stmt, torch.float64)
    lp32, g32s = cc.statement_nll(g32, [rows_of(t) for t in ctx], w_stmt, torch.float32)

    dctx = [_dev(t) for t in ctx]
    if kind == "strided":
        assert not dctx[0].is_contiguous()
    towers_before = towers.clone()
    kw = dict(index=None if index is None else index.cuda(), wgt=None if wgt is None else wgt.cuda(), gscale=gscale,
              want_grad=True)
    lp, out3, gth = ops.cat_nll(theta, towers, *dctx, **kw)
    tag = f"{name}/{kind}/N={N}"
    cc.within_yardstick(f"{tag} lp_native", lp[:, 0], lp64[:, 0], lp32[:, 0])
    cc.within_yardstick(f"{tag} lp_accent", lp[:, 1], lp64[:, 1], lp32[:, 1])
    o64 = torch.stack([-(lp64.sum(1)).mean(), lp64[:, 0].mean(), lp64[:, 1].mean()])
    o32 = torch.stack([-(lp32.sum(1)).mean(), lp32[:, 0].mean(), lp32[:, 1].mean()])
    cc.within_yardstick(f"{tag} out3", out3, o64, o32)
    off, parts = 0, []
    for i, (p, a, b) in enumerate(zip(cc.trained_params(g32), g64s, g32s)):
        parts.append(gth[off:off + p.numel()].view(p.shape))
        cc.within_yardstick(f"{tag} grad[{i}] {tuple(p.shape)}", parts[-1], a, b)
        off += p.numel()
    assert off == gth.numel()

    # exact properties
    assert torch.equal(towers, towers_before)                                   # the frozen towers are read only
    lp2, out3b, gth2 = ops.cat_nll(theta, towers, *dctx, **kw)
    assert torch.equal(lp, lp2) and torch.equal(out3, out3b) and torch.equal(gth, gth2)      # the same bits again
    lp_only, _, _ = ops.cat_nll(theta, towers, *dctx, index=kw["index"], want_out3=False)
    assert torch.equal(lp_only, lp)                                             # forward alone, the same rows
    if with_index:
        gathered = [t[index.cuda()].contiguous() for t in dctx]
        lp3, out3c, gth3 = ops.cat_nll(theta, towers, *gathered, wgt=kw["wgt"], gscale=gscale, want_grad=True)
        assert torch.equal(lp, lp3) and torch.equal(out3, out3c) and torch.equal(gth, gth3)
    if name == "corner":
        assert torch.equal(lp[:, 1], torch.zeros(N, device="cuda"))            # a one-class node: lp exactly 0
        assert torch.equal(parts[10], torch.zeros_like(parts[10])) and torch.equal(parts[11], torch.zeros_like(parts[11]))
    if name.startswith("branchy"):
        w1, b1, w2, b2, w3, b3, w4, b4, v1, c1, v2, c2 = parts
        for w, b, nxt in ((w1, b1, w2), (w2, b2, w3), (w3, b3, w4), (v1, c1, v2)):
            assert not w[0].any() and b[0] == 0 and not nxt[:, 0].any()         # the dead unit, and what it feeds
        for t in (w1, b1, w2, b2, w3):                                          # behind and at the all-zero layer: the
            assert not t.any()                                                  # gate is closed at pre-activation 0
        assert b3.any() and w4.any() and v1.any()


def _stored_argmax(z, e):
    """the first maximum of the fp64 sums of stored fp32 values"""
    return (z.double() + e.double()).argmax(dim=-1)


MAP_CASES = [("small", 1), ("small", "tile+1"), ("wide", 257), ("branchy-small", 70), ("corner", "tile-1")]


def _map_setup(name, rows, seed=0):
    sizes, g32, g64, theta, towers = _graphs(name)
    N = {"tile-1": _tile() - 1, "tile+1": _tile() + 1}.get(rows, rows)
    gen = torch.Generator().manual_seed(N + seed)
    lab = [torch.randint(0, c, (N,), generator=gen) for c in sizes]
    country = torch.eye(sizes[0])[lab[0]]
    return sizes, g32, g64, theta, towers, N, gen, lab, country


def _check_logits(tag, g32, g64, country, native_rows, logits, Cn):
    zn64, za64 = cc.statement_logits(g64, country, native_rows, torch.float64)
    zn32, za32 = cc.statement_logits(g32, country, native_rows, torch.float32)
    cc.within_yardstick(f"{tag} logits native", logits[:, :Cn], zn64, zn32)
    cc.within_yardstick(f"{tag} logits accent", logits[:, Cn:], za64, za32)


@pytest.mark.parametrize("name,rows", MAP_CASES)
def test_map_logits_and_sample(name, rows):
    ops = _ops()
    from ali_hip import source
    sizes, g32, g64, theta, towers, N, gen, lab, country = _map_setup(name, rows)
    Cc, Cn, Ca = sizes
    Ct = Cn + Ca
    dense = torch.rand(N, Cn, generator=gen)
    r = ops.cat_map(ops.CAT_LOGITS, theta, towers, country.cuda(), Cn, Ca, native_rows=dense.cuda())
    _check_logits(f"{name}/N={N} dense", g32, g64, country, dense, r["logits"].cpu(), Cn)
    r = ops.cat_map(ops.CAT_LOGITS, theta, towers, country.cuda(), Cn, Ca, y=(lab[1].cuda(), None))
    _check_logits(f"{name}/N={N} labels", g32, g64, country, torch.eye(Cn)[lab[1]], r["logits"].cpu(), Cn)

    r = ops.cat_map(ops.CAT_SAMPLE, theta, towers, country.cuda(), Cn, Ca, seed=5, offset=11, want_logits=True, want_g=True)
    z, g = r["logits"].cpu(), r["g"].cpu()
    ref = source.gumbel_reference(5, 0, N * Ct, offset=11).reshape(N, Ct)
    assert (g.double() - ref).abs().max() <= 2 * cc.EPS32 * ref.abs().max()
    native, accent = (t.cpu() for t in r["out"])
    assert native.dtype == torch.int64 and native.shape == (N,)
    assert torch.equal(native, _stored_argmax(z[:, :Cn], g[:, :Cn]))
    assert torch.equal(accent, _stored_argmax(z[:, Cn:], g[:, Cn:]))
    _check_logits(f"{name}/N={N} drawn", g32, g64, country, torch.eye(Cn)[native], z, Cn)     # accent saw the draw
    again = ops.cat_map(ops.CAT_SAMPLE, theta, towers, country.cuda(), Cn, Ca, seed=5, offset=11)
    assert all(torch.equal(a, b) for a, b in zip(again["out"], r["out"]))
    moved = ops.cat_map(ops.CAT_SAMPLE, theta, towers, country.cuda(), Cn, Ca, seed=5, offset=11 + N * Ct, want_g=True)
    assert N * Ct < 4 or not torch.equal(moved["g"], r["g"])
    # held nodes: native_speaker given, accent drawn under it; both given: nothing left to draw
    h = ops.cat_map(ops.CAT_SAMPLE, theta, towers, country.cuda(), Cn, Ca, y=(lab[1].cuda(), None), seed=5, offset=11,
                    want_logits=True, want_g=True)
    assert h["out"][0] is None
    zh = h["logits"].cpu()
    assert torch.equal(h["out"][1].cpu(), _stored_argmax(zh[:, Cn:], h["g"].cpu()[:, Cn:]))
    _check_logits(f"{name}/N={N} held", g32, g64, country, torch.eye(Cn)[lab[1]], zh, Cn)


@pytest.mark.parametrize("name,rows", MAP_CASES)
def test_map_differ(name, rows):
    ops = _ops()
    from ali_hip import source
    sizes, g32, g64, theta, towers, N, gen, lab, country = _map_setup(name, rows, seed=1)
    Cc, Cn, Ca = sizes
    for node, C in ((0, Cn), (1, Ca)):
        v = [None, None]
        v[node] = lab[1 + node].cuda()                          # forbid a random class per row
        y = (None, None) if node == 0 else (lab[1].cuda(), None)
        kw = dict(y=y, v=v, node=node, seed=9, offset=3)
        r = ops.cat_map(ops.CAT_DIFFER, theta, towers, country.cuda(), Cn, Ca, want_logits=True, want_g=True, **kw)
        z = r["logits"].cpu()[:, Cn:] if node else r["logits"].cpu()[:, :Cn]
        g = r["g"].cpu()
        assert g.shape == (ops.CAT_TRIES, N, C)
        ref = source.gumbel_reference(9, 0, ops.CAT_TRIES * N * C, offset=3).reshape(ops.CAT_TRIES, N, C)
        assert (g.double() - ref).abs().max() <= 2 * cc.EPS32 * ref.abs().max()
        tries = _stored_argmax(z[None], g)                       # [tries, N]: the statement's loop, every try
        differs = tries != lab[1 + node][None]
        found = differs.any(0)
        first = differs.int().argmax(0)                          # the first try that differs
        want = torch.where(found, tries[first, torch.arange(N)], tries[-1])
        assert torch.equal(r["out"][node].cpu(), want)
        assert torch.equal(r["status"].cpu(), (~found).int())
        assert C > 1 or not found.any()                          # a one-class node fails all 64 tries on every row
        quick = ops.cat_map(ops.CAT_DIFFER, theta, towers, country.cuda(), Cn, Ca, **kw)       # stops at the kept try
        assert torch.equal(quick["out"][node], r["out"][node]) and torch.equal(quick["status"], r["status"])
        if node == 0:                                            # accent drawn once, behind the tries, under the kept value
            zs = ops.cat_map(ops.CAT_SAMPLE, theta, towers, country.cuda(), Cn, Ca, y=(r["out"][0], None), seed=9,
                             offset=3 + ops.CAT_TRIES * N * Cn, want_logits=True, want_g=True)
            assert torch.equal(zs["out"][1], r["out"][1])


def test_map_differ_rows_forced_to_fail():
    """class 0 of native_speaker made certain: rows that forbid it use all 64 tries and report it, the others keep try 0"""
    ops = _ops()
    sizes, g32, _, theta, towers = _graphs("small")
    Cc, Cn, Ca = sizes
    th = theta.clone()
    off = sum(p.numel() for p in cc.trained_params(g32)[:7])       # b4
    th[off] += 1000.0
    N = 40
    country = torch.eye(Cc)[torch.arange(N) % Cc].cuda()
    forb = (torch.arange(N) % 3 != 0).long().cuda()                # rows 0, 3, ... forbid class 0
    r = ops.cat_map(ops.CAT_DIFFER, th, towers, country, Cn, Ca, v=(forb, None), node=0, seed=1, want_g=True,
                    want_logits=True)
    tries = _stored_argmax(r["logits"][None, :, :Cn], r["g"])
    assert not tries.any()                                          # every try of every row is class 0
    assert torch.equal(r["status"].cpu(), (forb == 0).int().cpu())
    assert torch.equal(r["out"][0].cpu(), torch.zeros(N, dtype=torch.int64))


@pytest.mark.parametrize("name,rows", MAP_CASES)
def test_map_abduct_and_cf(name, rows):
    ops = _ops()
    from attribute_scms.causal_module import gumbel_posterior
    sizes, g32, g64, theta, towers, N, gen, lab, country = _map_setup(name, rows, seed=2)
    Cc, Cn, Ca = sizes
    y = (lab[1].cuda(), lab[2].cuda())
    r = ops.cat_map(ops.CAT_ABDUCT, theta, towers, country.cuda(), Cn, Ca, y=y, seed=4, offset=100, want_logits=True,
                    want_g=True)
    z, g, noise = (r[k].cpu() for k in ("logits", "g", "noise"))
    _check_logits(f"{name}/N={N} abduct", g32, g64, country, torch.eye(Cn)[lab[1]], z, Cn)
    for tag, sl, yy in (("native", slice(0, Cn), lab[1]), ("accent", slice(Cn, Cn + Ca), lab[2])):
        cc.within_yardstick(f"{name}/N={N} noise {tag}", noise[:, sl], gumbel_posterior(z[:, sl].double(), yy, g[:, sl].double()),
                            gumbel_posterior(z[:, sl], yy, g[:, sl]))
        assert torch.equal(_stored_argmax(z[:, sl], noise[:, sl]), yy)           # the noise regenerates the observation

    country_cf = torch.eye(Cc)[(lab[0] + 1) % Cc]
    v = ((lab[1] + 1) % Cn, (lab[2] + 1) % Ca)
    for moved in (False, True):
        for mask in range(4):
            c = ops.cat_map(ops.CAT_CF, theta, towers, country.cuda(), Cn, Ca, country_cf=country_cf.cuda() if moved else None,
                            y=y, v=tuple(v[j].cuda() if (mask >> j) & 1 else None for j in range(2)), cf_mask=mask, seed=4,
                            offset=100, want_logits=True, want_noise=True)
            assert torch.equal(c["noise"], r["noise"]) and torch.equal(c["logits"][0], r["logits"])     # the same abduction
            z1, native, accent = c["logits"][1].cpu(), c["out"][0].cpu(), c["out"][1].cpu()
            assert torch.equal(native, v[0] if mask & 1 else _stored_argmax(z1[:, :Cn], noise[:, :Cn])), (moved, mask)
            assert torch.equal(accent, v[1] if mask & 2 else _stored_argmax(z1[:, Cn:], noise[:, Cn:])), (moved, mask)
            _check_logits(f"{name}/N={N} cf moved={moved} mask={mask}", g32, g64, country_cf if moved else country,
                          torch.eye(Cn)[native], z1, Cn)
            if not moved and mask == 0:
                assert torch.equal(native, lab[1]) and torch.equal(accent, lab[2])   # nothing intervened on: the observation
            if not moved and mask == 1 and Cn > 1:
                assert torch.equal(native, v[0])


def test_bad_arguments_are_refused_before_any_launch():
    ops = _ops()
    sizes, _, _, theta, towers = _graphs("small")
    Cc, Cn, Ca = sizes
    country = torch.eye(Cc)[torch.zeros(4, dtype=torch.int64)].cuda()
    y = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="mode"):
        ops.cat_map(9, theta, towers, country, Cn, Ca)
    with pytest.raises(RuntimeError, match="cf_mask"):
        ops.cat_map(ops.CAT_CF, theta, towers, country, Cn, Ca, y=(y, y), cf_mask=4)
    with pytest.raises(RuntimeError, match="cf_mask"):
        ops.cat_map(ops.CAT_CF, theta, towers, country, Cn, Ca, y=(y, y), cf_mask=1)           # intervened on without a value
    with pytest.raises(RuntimeError, match="observed"):
        ops.cat_map(ops.CAT_ABDUCT, theta, towers, country, Cn, Ca, y=(y, None))
    with pytest.raises(RuntimeError, match="forbidden"):
        ops.cat_map(ops.CAT_DIFFER, theta, towers, country, Cn, Ca, node=1)
    with pytest.raises(ValueError, match="class counts"):
        ops.cat_map(ops.CAT_SAMPLE, theta, towers, torch.zeros(4, 65, device="cuda"), Cn, Ca)
    with pytest.raises(ValueError):
        ops.cat_map(ops.CAT_SAMPLE, theta[:-1], towers, country, Cn, Ca)
    with pytest.raises(ValueError):
        ops.cat_map(ops.CAT_SAMPLE, theta, towers, country.double(), Cn, Ca)
    native, accent = torch.eye(Cn)[[0] * 4].cuda(), torch.eye(Ca)[[0] * 4].cuda()
    with pytest.raises(ValueError):
        ops.cat_nll(theta, towers, country, native[:3], accent)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        ops.cat_nll(theta, towers, country, native, accent, want_lp=False, want_out3=False)
    with pytest.raises(ValueError):
        ops.cat_nll(theta, towers, country, native, accent, wgt=torch.zeros(4, 3, device="cuda"))
