"""The three kernels of csrc/attrib.hip on their own, through ``ops``.

Reference: this file's torch statement of each kernel in fp64 on the fp32 inputs; yardstick: the same statement in CPU
fp32 (``_check`` of test_gpu_xent.py: at most YARD times the CPU-fp32 error and at most RTOL of max|ref64|).  What the
header states exactly is compared exactly: the attribute part of a row at t == 0 and t == 1, delta (one fp32
subtraction), the padding columns, the drawn background rows and mixing weights against ``ali_hip.rng``, a reduction over
rows whose delta is zero, the classes ``ali_eg_reduce`` does not write, and every call against its own repetition."""
import numpy as np
import pytest
import torch

from test_gpu_xent import _check

gpu = pytest.mark.gpu

L, EMB, A = 512, 256, 13
N_LOG, LD = L + EMB + 3, 800
# attribute columns [digit (10) | thickness | intensity | slant] -> row [z | digit @ table | intensity | slant | thickness]
SEGS = [(0, 10, 0, L, 0, 0), (0, 1, 10, L + EMB + 2, -1, 10), (0, 1, 11, L + EMB, -1, 11), (0, 1, 12, L + EMB + 1, -1, 12)]
CONT = [(10, L + EMB + 2), (11, L + EMB), (12, L + EMB + 1)]


def _layout(table):
    from ali_hip import ops
    return ops.CfLayout(SEGS, [table], N_LOG, LD)


def _inputs(R, S, nd, Nb, seed):
    g = torch.Generator().manual_seed(seed)
    x, bg = torch.randn(R, A, generator=g), torch.randn(Nb, A, generator=g)
    idx = torch.randint(0, Nb, (R, S), generator=g, dtype=torch.int32)
    t = torch.rand(R, S, generator=g)
    z = torch.randn(R, S, nd, L, generator=g)
    table = torch.randn(10, EMB, generator=g)
    return x, bg, idx, t, z, table


def input_statement(x, bg, idx, t, z, table, dt):
    """rows [R*S*nd, LD] and delta of ali_eg_input in dtype ``dt``"""
    R, S, nd = z.shape[:3]
    x, bg, t, table = x.to(dt), bg.to(dt), t.to(dt).unsqueeze(-1), table.to(dt)
    b = bg[idx.long()]
    a = t * x.unsqueeze(1) + (1 - t) * b
    rep = a.unsqueeze(2).expand(R, S, nd, A).reshape(-1, A)
    rows = torch.zeros(R * S * nd, LD, dtype=dt)
    rows[:, :L] = z.to(dt).reshape(-1, L)
    rows[:, L:L + EMB] = rep[:, :10] @ table
    for src, dst in CONT:
        rows[:, dst] = rep[:, src]
    return rows, x.unsqueeze(1) - b


@gpu
@pytest.mark.parametrize("R,S,nd", [(2, 3, 2), (1, 1, 1)])
def test_eg_input_rows_delta_ends_and_padding(R, S, nd):
    from ali_hip import ops
    Nb = 5
    x, bg, idx, t, z, table = _inputs(R, S, nd, Nb, seed=10 * R + S)
    idx.reshape(-1)[0], t.reshape(-1)[0] = 0, 0.0                      # the first background row, t exactly 0
    idx.reshape(-1)[-1] = Nb - 1                                        # the last background row ...
    if R * S > 1:
        t.reshape(-1)[-1] = 1.0                                         # ... and t exactly 1
        x[0] = bg[idx[0, 1]]                                            # x == bg[idx]: delta exactly 0
    lay = _layout(table.cuda())
    args = (lay, L, x.cuda(), bg.cuda(), S, nd, idx.cuda(), t.cuda(), z.cuda())
    rows, delta, idx_used, t_used = ops.eg_input(*args, want_draws=True)
    again = ops.eg_input(*args, want_draws=True)
    assert all(torch.equal(u, v) for u, v in zip((rows, delta, idx_used, t_used), again))
    assert rows.shape == (R * S * nd, LD) and delta.shape == (R, S, A)
    assert torch.equal(idx_used.cpu(), idx) and torch.equal(t_used.cpu(), t)
    r64, d64 = input_statement(x, bg, idx, t, z, table, torch.float64)
    r32, d32 = input_statement(x, bg, idx, t, z, table, torch.float32)
    label = f"eg_input R={R} S={S} nd={nd}"
    rows_c = rows.cpu()
    assert torch.equal(rows_c[:, :L], z.reshape(-1, L))                 # z is copied
    assert not rows_c[:, N_LOG:].any()                                   # padding columns are exactly 0
    assert torch.equal(delta.cpu(), d32)                                 # one fp32 subtraction
    _check(label + " table product", rows[:, L:L + EMB], r64[:, L:L + EMB], r32[:, L:L + EMB])
    _check(label + " continuous", rows[:, L + EMB:N_LOG], r64[:, L + EMB:N_LOG], r32[:, L + EMB:N_LOG])
    # t == 0: the attribute part is bg[idx], t == 1: it is x, bit for bit -- the continuous columns directly, the table
    # columns as the product of exactly that row
    ends = [(0, bg[idx.reshape(-1)[0].item()])] + ([(R * S - 1, x[R - 1])] if R * S > 1 else [])
    for rk, want in ends:
        for s in range(nd):
            row = rows_c[rk * nd + s]
            for src, dst in CONT:
                assert row[dst].item() == want[src].item(), (label, rk, s, src)
        exact = ops.eg_input(lay, L, want.reshape(1, A).cuda(), want.reshape(1, A).cuda(), 1, 1,
                             torch.zeros(1, 1, dtype=torch.int32, device="cuda"), torch.full((1, 1), 0.5, device="cuda"),
                             torch.zeros(1, 1, 1, L, device="cuda"))[0]
        assert torch.equal(rows[rk * nd, L:L + EMB], exact[0, L:L + EMB]), (label, rk)
    if R * S > 1:
        assert not delta[0, 1].any()


@gpu
def test_eg_input_device_draws_follow_the_host_references():
    from ali_hip import ops, rng
    R, S, nd, Nb, seed, counter, offset = 2, 3, 2, 5, 0x5EED, 3, 4
    x, bg, _, _, _, table = _inputs(R, S, nd, Nb, seed=7)
    lay = _layout(table.cuda())
    ctr = torch.full((1,), counter, dtype=torch.int64, device="cuda")
    rows, delta, idx, t = ops.eg_input(lay, L, x.cuda(), bg.cuda(), S, nd, seed=seed, dev_counter=ctr, offset=offset,
                                       want_draws=True)
    want_i = torch.from_numpy(rng.eg_index_reference(seed, counter, R * S, Nb, offset * S)).reshape(R, S)
    want_t = rng.eg_t_reference(seed, counter, R * S, offset * S).reshape(R, S)
    assert torch.equal(idx.cpu().long(), want_i) and torch.equal(t.cpu(), want_t)
    # z: ali_normal_fill's stream bit for bit, and within the bound test_gpu_vae_kernels.py holds that stream to (four
    # times what the recipe evaluated in numpy fp32 deviates from the fp64 reference)
    n, zoff = R * S * nd * L, offset * S * nd * L
    fill = ops.normal_fill(seed, torch.empty(n, device="cuda"), dev_counter=ctr, offset=zoff)
    assert torch.equal(rows[:, :L].reshape(-1), fill)
    ref = rng.normal_reference(seed, counter, n, zoff).numpy()
    k1, k2, odd = rng.latent_bits(seed, counter, n, zoff)
    u1, u2 = k1.astype(np.float32) * np.float32(2.0 ** -24), k2.astype(np.float32) * np.float32(2.0 ** -24)
    f32 = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.where(odd, np.sin(np.float32(2.0 * np.pi) * u2),
                                                            np.cos(np.float32(2.0 * np.pi) * u2))
    dev, bound = np.abs(fill.cpu().numpy() - ref).max(), 4 * np.abs(f32.astype(np.float64) - ref).max()
    print(f"ATTRIB eg_input drawn z: device max |dev| {dev:.3e}, numpy-f32 max |dev| {bound / 4:.3e}")
    assert dev <= bound, (dev, bound)
    # what it drew is what it used: the same call with the draws handed in gives the same bits
    given = ops.eg_input(lay, L, x.cuda(), bg.cuda(), S, nd, idx, t, rows[:, :L].reshape(R, S, nd, L).contiguous())
    assert torch.equal(given[0], rows) and torch.equal(given[1], delta)
    # a call split into row ranges draws what the whole call draws
    tail = ops.eg_input(lay, L, x[1:].cuda(), bg.cuda(), S, nd, seed=seed, dev_counter=ctr, offset=offset + 1)
    assert torch.equal(tail[0], rows[S * nd:]) and torch.equal(tail[1], delta[1:])


def seed_statement(z, c, scale, dt):
    p = z.to(dt).softmax(1)
    onehot = torch.zeros_like(p)
    onehot[:, c] = 1
    g = scale * p[:, c:c + 1] * (onehot - p)
    # the outputs are fp32: what lies below half its smallest subnormal (the +-80 rows' e^-160) is 0 there
    tiny = 2.0 ** -150
    return torch.where(g.abs() < tiny, torch.zeros_like(g), g), torch.where(p < tiny, torch.zeros_like(p), p)


@gpu
@pytest.mark.parametrize("K", [10, 2])
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_eg_seed(N, K):
    from ali_hip import ops
    g = torch.Generator().manual_seed(100 * N + K)
    z = torch.randn(N, K, generator=g)
    z[N // 2] = torch.where(torch.arange(K) % 2 == 0, 80.0, -80.0)     # exp overflows without the max shift
    scale = 1.0 / (200 * 4)
    for c in (0, K - 1):
        gl, p = ops.eg_seed(z.cuda(), c, scale, want_p=True)
        gl2, none = ops.eg_seed(z.cuda(), c, scale)
        assert none is None and torch.equal(gl, gl2)
        g64, p64 = seed_statement(z, c, scale, torch.float64)
        g32, p32 = seed_statement(z, c, scale, torch.float32)
        label = f"eg_seed N={N} K={K} c={c}"
        assert torch.isfinite(gl).all() and torch.isfinite(p).all()
        _check(label + " glogit", gl, g64, g32)
        _check(label + " p", p, p64, p32)
        row = N // 2                                     # the +-80 row on its own scale (all zeros when p_c = e^-160)
        _check(label + " +-80 row", gl[row:row + 1], g64[row:row + 1], g32[row:row + 1])
        # every row of the seed sums to zero within the yardstick: the sums are pooled with the entries, as
        # test_gpu_explain.py pools small tensors, so that their error is held to the bounds of the entries' scale
        sums = lambda v: torch.cat([v.double().cpu().reshape(-1), v.double().cpu().sum(dim=1)])  # noqa: E731
        _check(label + " entries and row sums", sums(gl), sums(g64), sums(g32))


def reduce_statement(g_rows, delta, table, nd, dt):
    """phi[r, :] of one class: [R, A]"""
    R, S, _ = delta.shape
    g = g_rows.to(dt)
    ga = torch.zeros(g.shape[0], A, dtype=dt)
    ga[:, :10] = g[:, L:L + EMB] @ table.to(dt).T
    for src, dst in CONT:
        ga[:, src] = g[:, dst]
    return (delta.to(dt).unsqueeze(2) * ga.reshape(R, S, nd, A)).sum(dim=(1, 2))


@gpu
@pytest.mark.parametrize("R,S,nd", [(2, 3, 2), (1, 67, 3)])
def test_eg_reduce(R, S, nd):
    from ali_hip import ops
    g = torch.Generator().manual_seed(1000 * R + S)
    C = 4
    g_rows = torch.randn(R * S * nd, LD, generator=g)
    delta = torch.randn(R, S, A, generator=g)
    table = torch.randn(10, EMB, generator=g)
    lay = _layout(table.cuda())
    label = f"eg_reduce R={R} S={S} nd={nd}"
    for c in (0, C - 1):
        phi = torch.full((R, C, A), float("nan"), device="cuda")
        ops.eg_reduce(lay, g_rows.cuda(), delta.cuda(), nd, phi, c)
        phi2 = torch.full((R, C, A), float("nan"), device="cuda")
        ops.eg_reduce(lay, g_rows.cuda(), delta.cuda(), nd, phi2, c)
        assert torch.equal(phi[:, c], phi2[:, c])                                      # equal bits
        others = [k for k in range(C) if k != c]
        assert torch.isnan(phi[:, others]).all()                                        # untouched
        _check(f"{label} c={c}", phi[:, c], reduce_statement(g_rows, delta, table, nd, torch.float64),
               reduce_statement(g_rows, delta, table, nd, torch.float32))
    # an explained row whose delta is zero gives exactly zero
    zero = delta.clone()
    zero[R - 1] = 0
    phi = torch.full((R, C, A), float("nan"), device="cuda")
    ops.eg_reduce(lay, g_rows.cuda(), zero.cuda(), nd, phi, 1)
    assert not phi[R - 1, 1].any() and not torch.isnan(phi[R - 1, 1]).any()
    if R > 1:
        assert phi[0, 1].abs().max().item() > 0
    # a row's bits do not depend on the rows next to it
    alone = torch.full((1, C, A), float("nan"), device="cuda")
    ops.eg_reduce(lay, g_rows[:S * nd].cuda(), delta[:1].cuda(), nd, alone, 1)
    full = torch.full((R, C, A), float("nan"), device="cuda")
    ops.eg_reduce(lay, g_rows.cuda(), delta.cuda(), nd, full, 1)
    assert torch.equal(alone[0, 1], full[0, 1])


@gpu
def test_argument_checks():
    from ali_hip import ops
    x, bg, idx, t, z, table = _inputs(1, 2, 1, 3, seed=1)
    lay = _layout(table.cuda())
    with pytest.raises(ValueError):
        ops.eg_input(lay, L, x.cuda(), bg[:, :12].cuda(), 2, 1)
    with pytest.raises(ValueError):
        ops.eg_input(lay, L, x.cuda(), bg.cuda(), 2, 1, idx=idx[:, :1].cuda())
    with pytest.raises(RuntimeError, match="ali_eg_input"):
        ops.eg_input(ops.CfLayout(SEGS[:3], [table.cuda()], N_LOG, LD), L, x.cuda(), bg.cuda(), 2, 1)   # a column unwritten
    with pytest.raises(RuntimeError, match="ali_eg_seed"):
        ops.eg_seed(torch.zeros(2, 3, device="cuda"), 3, 1.0)
    with pytest.raises(RuntimeError, match="ali_eg_reduce"):
        ops.eg_reduce(lay, torch.zeros(2, LD, device="cuda"), torch.zeros(1, 2, A, device="cuda"), 1,
                      torch.zeros(1, 4, A, device="cuda"), 4)
