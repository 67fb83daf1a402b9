"""The two kernels of csrc/cfeval.hip on the device: ``ops.group_moments`` and ``ops.manifold_err``.

Reference: the pairwise statement of audiomnist_cf_eval.py:93-131 on the CPU in fp64 (``ManifoldBank`` on CPU tensors;
for the moments an fp64 ``index_add`` over the same row order); yardstick: the same statement in CPU fp32, which is what
the scripts compute; bound: ``flow_cases.within_yardstick`` entry by entry (MULT = 4, floor FLOOR_ULPS = 4).  Every test
prints its worst ratio.  Every call is made twice and must give the same bits, and leaves the workspace's reserved head
at zero."""
import pytest
import torch

from flow_cases import within_yardstick
from test_cfeval_cpu import corner_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from ali_hip import ops
    return ops


def _head_is_zero():
    assert int(_ops().workspace(torch.device(DEV))[:4096].count_nonzero()) == 0


def _bank_rows(N, D, O, C, seed):
    """rows in [-1, 1]; cells dealt round-robin (every cell is hit once N >= O * C) except that the last class belongs
    to owner 0 alone"""
    g = torch.Generator().manual_seed(seed + 13 * N + D + 101 * O + C)
    rows = torch.rand(N, D, generator=g) * 2 - 1
    cell = torch.arange(N) % (O * C)
    owner, cls = cell // C, cell % C
    owner = torch.where(cls == C - 1, torch.zeros_like(owner), owner)
    return rows, owner, cls


def _csr(owner, cls, O, C):
    cell = owner * C + cls
    order = torch.argsort(cell, stable=True).to(torch.int32)
    cnt = torch.bincount(cell, minlength=O * C)
    start = torch.cat([cnt.new_zeros(1), cnt.cumsum(0)]).to(torch.int32)
    return cell, order, start, cnt


# ------------------------------------------------------------------------------------------------------ group_moments
@pytest.mark.parametrize("O,C", [(1, 1), (3, 2), (5, 10)])
@pytest.mark.parametrize("D", [1, 3, 63, 784, 785, 4097])
def test_group_moments(D, O, C):
    ops = _ops()
    worst = 0.0
    for N in (1, 7, 130):
        rows, owner, cls = _bank_rows(N, D, O, C, 1)
        cell, order, start, cnt = _csr(owner, cls, O, C)
        got = ops.group_moments(rows.to(DEV), order.to(DEV), start.to(DEV), O, C)
        again = ops.group_moments(rows.to(DEV), order.to(DEV), start.to(DEV), O, C)
        for a, b in zip(got, again):
            assert a.dtype == torch.float64 and torch.equal(a, b)
        S, Q, TS, TQ = (t.cpu() for t in got)
        assert S.shape == Q.shape == (O * C, D) and TS.shape == TQ.shape == (C, D)
        ref, yard = {}, {}
        for dt, out in ((torch.float64, ref), (torch.float32, yard)):
            r = rows.to(dt)
            out["S"] = torch.zeros(O * C, D, dtype=dt).index_add_(0, cell, r)
            out["Q"] = torch.zeros(O * C, D, dtype=dt).index_add_(0, cell, r * r)
            out["TS"] = torch.zeros(C, D, dtype=dt).index_add_(0, cls, r)
            out["TQ"] = torch.zeros(C, D, dtype=dt).index_add_(0, cls, r * r)
        for k, v in (("S", S), ("Q", Q), ("TS", TS), ("TQ", TQ)):
            worst = max(worst, within_yardstick(f"group_moments {k} D={D} N={N} O={O} C={C}", v, ref[k], yard[k]))
        empty = cnt == 0
        assert torch.equal(S[empty], torch.zeros(int(empty.sum()), D, dtype=torch.float64))
        assert torch.equal(Q[empty], torch.zeros(int(empty.sum()), D, dtype=torch.float64))
        # the last class is owner 0's alone: its totals are that cell's sums, bit for bit
        assert torch.equal(TS[C - 1], S[C - 1]) and torch.equal(TQ[C - 1], Q[C - 1])
        # a pitched view 4 bytes off a 16-byte boundary: the element-wise path, the same bits
        ld = D + 3
        buf = torch.zeros(N * ld + 4, device=DEV)
        view = buf[1:1 + N * ld].view(N, ld)[:, :D]
        view.copy_(rows)
        assert view.data_ptr() % 16 == 4 and view.stride(0) == ld
        for a, b in zip(got, ops.group_moments(view, order.to(DEV), start.to(DEV), O, C)):
            assert torch.equal(a, b)
    print(f"group_moments D={D} O={O} C={C}: worst yardstick ratio {worst:.3g}")
    _head_is_zero()


def test_group_moments_skips_what_the_csr_leaves_out_and_checks_its_arguments():
    ops = _ops()
    rows, owner, cls = _bank_rows(20, 12, 2, 2, 3)
    keep = torch.arange(20) % 5 != 0                                    # rows 0, 5, 10, 15 belong to no cell
    cell = torch.where(keep, owner * 2 + cls, torch.full_like(owner, 4))
    order = torch.argsort(cell, stable=True).to(torch.int32)
    cnt = torch.bincount(cell, minlength=5)[:4]
    start = torch.cat([cnt.new_zeros(1), cnt.cumsum(0)]).to(torch.int32)
    S, Q, TS, TQ = ops.group_moments(rows.to(DEV), order.to(DEV), start.to(DEV), 2, 2)
    _, order2, start2, _ = _csr(owner[keep], cls[keep], 2, 2)
    S2, Q2, TS2, TQ2 = ops.group_moments(rows[keep].to(DEV), order2.to(DEV), start2.to(DEV), 2, 2)
    assert torch.equal(S, S2) and torch.equal(Q, Q2) and torch.equal(TS, TS2) and torch.equal(TQ, TQ2)
    with pytest.raises(RuntimeError, match="O \\* C"):
        ops.group_moments(rows.to(DEV), order.to(DEV), torch.zeros(70001, dtype=torch.int32, device=DEV), 70000, 1)
    with pytest.raises(ValueError, match="int32"):
        ops.group_moments(rows.to(DEV), order.long().to(DEV), start.to(DEV), 2, 2)


# ------------------------------------------------------------------------------------------------------- manifold_err
def _errors_on_device(rows, owner, cls, O, C, cf, cf_owner, cf_cls):
    """ManifoldBank on the device, called twice; [M, 3] on the host"""
    from ali_hip.cfeval import ManifoldBank
    bank = ManifoldBank(rows.to(DEV), owner.to(DEV), cls.to(DEV), O, C)
    out = []
    for _ in range(2):
        e = bank.errors(cf.to(DEV), cf_owner.to(DEV), cf_cls.to(DEV))
        out.append(torch.stack([e["same"], e["other"], e["ratio"]], dim=1).cpu())
    assert torch.equal(torch.isnan(out[0]), torch.isnan(out[1]))
    assert torch.equal(out[0].nan_to_num(7.0), out[1].nan_to_num(7.0))
    _head_is_zero()
    return out[0]


def _statement(rows, owner, cls, O, C, cf, cf_owner, cf_cls, dtype):
    from ali_hip.cfeval import ManifoldBank
    e = ManifoldBank(rows.to(dtype), owner, cls, O, C).errors(cf.to(dtype), cf_owner, cf_cls)
    return torch.stack([e["same"], e["other"], e["ratio"]], dim=1)


def _check(name, got, ref64, f32):
    worst = 0.0
    for j, col in enumerate(("same", "other", "ratio")):
        worst = max(worst, within_yardstick(f"{name} {col}", got[:, j], ref64[:, j], f32[:, j]))
    print(f"{name}: worst yardstick ratio {worst:.3g}")
    return worst


_MANIFOLD = [(D, M, 40, 3, 2) for D in (1, 3, 63, 784, 785, 4097, 16384) for M in (1, 5, 257)]
_MANIFOLD.append((64 * 4096 + 5, 2, 3, 3, 1))                  # 65 chunks of 4096: the 64-block cap is reached and passed


@pytest.mark.parametrize("D,M,N,O,C", _MANIFOLD)
def test_manifold_err(D, M, N, O, C):
    rows, owner, cls = _bank_rows(N, D, O, C, 2)
    if C == 1:
        owner = torch.arange(N) % O                                # (one class: every owner keeps its rows)
    g = torch.Generator().manual_seed(D + M)
    cf = torch.rand(M, D, generator=g) * 2 - 1
    cf_cls = torch.randint(0, max(C - 1, 1), (M,), generator=g)     # the classes every owner holds
    cf_owner = torch.randint(0, O, (M,), generator=g)
    got = _errors_on_device(rows, owner, cls, O, C, cf, cf_owner, cf_cls)
    _check(f"manifold_err D={D} M={M}", got, _statement(rows, owner, cls, O, C, cf, cf_owner, cf_cls, torch.float64),
           _statement(rows, owner, cls, O, C, cf, cf_owner, cf_cls, torch.float32))


@pytest.mark.parametrize("D", [63, 784, 16384])
def test_manifold_err_near_and_equal_rows(D):
    """rows within 1e-3 of a bank row of their own cell are a tensor of their own: their small ``same`` values set
    their own scale.  A row EQUAL to the only bank row of its cell has same == 0.0 exactly."""
    O, C = 4, 2
    rows, owner, cls = _bank_rows(41, D, 3, C, 4)
    owner[-1], cls[-1] = 3, 0                                       # cell (3, 0): this one row
    g = torch.Generator().manual_seed(D)
    at = torch.tensor([0, 8, 12, 40, 40, 4])                         # rows of class 0, which every owner holds
    near = rows[at] + 1e-3 * (torch.rand(len(at), D, generator=g) * 2 - 1)
    got = _errors_on_device(rows, owner, cls, O, C, near, owner[at], cls[at])
    ref64 = _statement(rows, owner, cls, O, C, near, owner[at], cls[at], torch.float64)
    _check(f"manifold_err near rows D={D}", got, ref64, _statement(rows, owner, cls, O, C, near, owner[at], cls[at],
                                                                   torch.float32))
    assert ref64[3, 0] < 1e-6 * D                                  # (the one-row cell: the distance to that row alone)
    equal = _errors_on_device(rows, owner, cls, O, C, rows[40:41], owner[40:41], cls[40:41])
    assert equal[0, 0].item() == 0.0 and equal[0, 2].item() == 0.0 and equal[0, 1].item() > 0


def test_manifold_err_nan_corners_and_device_indices():
    from ali_hip.cfeval import ManifoldBank
    ops = _ops()
    rows, ro, rc, cf, o, c, nan = corner_case(torch.float32)
    ref64 = _statement(rows, ro, rc, 3, 3, cf, o, c, torch.float64)
    f32 = _statement(rows, ro, rc, 3, 3, cf, o, c, torch.float32)
    assert torch.equal(torch.isnan(ref64), nan)
    got = _errors_on_device(rows, ro, rc, 3, 3, cf, o, c)
    assert torch.equal(torch.isnan(got), nan)                      # NaN exactly where the CPU statement has it
    within_yardstick("manifold_err corners", got[~nan], ref64[~nan], f32[~nan])
    # the indices are read on the device: changed in place between two calls, they change the result
    bank = ManifoldBank(rows.to(DEV), ro.to(DEV), rc.to(DEV), 3, 3)
    od, cd = o.to(DEV).to(torch.int32), c.to(DEV).to(torch.int32)
    cfd = cf.to(DEV)
    first = ops.manifold_err(cfd, od, cd, bank.S, bank.Q, bank.TS, bank.TQ, bank.cnt, bank.tcnt).clone()
    assert torch.equal(first.cpu().nan_to_num(7.0), got.nan_to_num(7.0))
    o2, c2 = o.flip(0).clone(), c.flip(0).clone()
    od.copy_(o2)
    cd.copy_(c2)
    second = ops.manifold_err(cfd, od, cd, bank.S, bank.Q, bank.TS, bank.TQ, bank.cnt, bank.tcnt).cpu()
    ref2 = _statement(rows, ro, rc, 3, 3, cf, o2, c2, torch.float64)
    assert torch.equal(torch.isnan(second), torch.isnan(ref2)) and not torch.equal(torch.isnan(second), nan)
    ok = ~torch.isnan(ref2)
    within_yardstick("manifold_err after an in-place index change", second[ok], ref2[ok],
                     _statement(rows, ro, rc, 3, 3, cf, o2, c2, torch.float32)[ok])
    _head_is_zero()
    with pytest.raises(ValueError, match="int32"):
        ops.manifold_err(cfd, od.long(), cd, bank.S, bank.Q, bank.TS, bank.TQ, bank.cnt, bank.tcnt)
    with pytest.raises(ValueError, match="float64"):
        ops.manifold_err(cfd, od, cd, bank.S.float(), bank.Q, bank.TS, bank.TQ, bank.cnt, bank.tcnt)
