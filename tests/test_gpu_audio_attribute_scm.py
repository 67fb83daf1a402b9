"""The AudioMNIST attribute SCM on the device through its family interface: ``graph.log_prob`` under autograd,
``CatStepper`` (one step taken apart; captured against eager), ``train``, and the sampling entries of the graph."""
import numpy as np
import pytest
import torch

import cat_cases as cc

pytestmark = pytest.mark.gpu
SIZES = cc.SIZES["small"]


def _pair(seed=3, sizes=SIZES):
    """(the device graph, its fp32 and fp64 CPU statements) on the same weights"""
    g32 = cc.new_graph(sizes, seed)
    return cc.twin(g32, sizes, torch.float32, device="cuda"), g32, cc.twin(g32, sizes, torch.float64)


def _obs(ctx, dev=None, dtype=None):
    return {k: (v if dev is None else v.to(dev)) if dtype is None else v.to(dtype) for k, v in zip(cc.TRIO, ctx)}


def test_log_prob_under_autograd():
    gd, g32, g64 = _pair()
    assert gd._cat is not None and gd._cat.matches(gd)
    assert all(a is b for a, b in zip(gd._cat.params, cc.trained_params(gd)))
    ctx = cc.contexts(SIZES, 97, "onehot")
    wgt = torch.randn(97, 2, generator=torch.Generator().manual_seed(1))
    lp64, gr64 = cc.statement_nll(g64, ctx, wgt, torch.float64)
    lp32, gr32 = cc.statement_nll(g32, ctx, wgt, torch.float32)
    lp = gd.log_prob(_obs(ctx, "cuda"))
    assert set(lp) == set(cc.TRIO) and all(v.shape == (97,) and v.is_cuda for v in lp.values())
    cc.within_yardstick("family lp_native", lp["native_speaker"], lp64[:, 0], lp32[:, 0])
    cc.within_yardstick("family lp_accent", lp["accent"], lp64[:, 1], lp32[:, 1])
    w = wgt.cuda()
    (lp["native_speaker"] * w[:, 0] + lp["accent"] * w[:, 1]).sum().backward()
    for i, (p, a, b) in enumerate(zip(cc.trained_params(gd), gr64, gr32)):
        cc.within_yardstick(f"family grad[{i}]", p.grad, a, b)
    tower = cc.linears(gd)[4]
    assert tower.weight.grad is None


def test_one_stepper_step_taken_apart():
    """The parameter check: fp32 Adam forms p - step with |step| ~ lr on the first step, so its rounding is an ulp32 at
    the size of the larger operand, max(|p|, lr), not at the size of a parameter that happens to lie near zero."""
    from ali_hip.cat import CatStepper
    gd, g32, g64 = _pair(seed=4)
    ctx = cc.contexts(SIZES, 150, "onehot")
    before = gd._cat.theta.detach().clone()
    stepper = CatStepper(gd, lr=1e-2, capture=False)
    out = stepper.step(*[t.cuda() for t in ctx])
    # the gradient of the loss by the yardstick
    wgt = torch.full((150, 2), -1.0 / 150, dtype=torch.float64)
    lp64, gr64 = cc.statement_nll(g64, ctx, wgt, torch.float64)
    lp32, gr32 = cc.statement_nll(g32, ctx, wgt, torch.float32)
    cc.within_yardstick("stepper gradient", stepper.g, torch.cat([x.reshape(-1) for x in gr64]),
                        torch.cat([x.reshape(-1) for x in gr32]))
    cc.within_yardstick("stepper loss", out["loss"], -lp64.sum(1).mean(), -lp32.sum(1).mean())
    cc.within_yardstick("stepper lp_accent", out["lp_accent"], lp64[:, 1].mean(), lp32[:, 1].mean())
    # the parameters: torch's Adam in fp64 on the DEVICE's gradient, so Adam's g / sqrt(v) amplifies nothing
    p = before.double().cpu().requires_grad_(True)
    p.grad = stepper.g.double().cpu()
    torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8).step()
    got = gd._cat.theta.double().cpu()
    err = (got - p.detach()).abs()
    ulp = cc.EPS32 * torch.maximum(p.detach().abs(), before.double().cpu().abs()).clamp(min=1e-2)
    print("Adam: worst error in ulp32", float((err / ulp).max()))
    assert (err <= 4 * ulp).all()
    assert int(stepper.dev_step) == 1


def test_captured_steps_are_eager_steps_bit_for_bit():
    from ali_hip.cat import CatStepper
    runs = {}
    for capture in (False, True):
        gd, _, _ = _pair(seed=5)
        stepper = CatStepper(gd, capture=capture)
        losses = []
        for step in range(3):
            for n in (128, 45):                                  # a full and a ragged last batch: two graphs
                ctx = [t.cuda() for t in cc.contexts(SIZES, n, "onehot", seed=step)]
                losses.append(stepper.step(*ctx)["loss"].clone())
        # the epoch form: rows of one table through an index
        table = [t.cuda() for t in cc.contexts(SIZES, 200, "onehot", seed=9)]
        idx = torch.randperm(200, generator=torch.Generator().manual_seed(2)).cuda()
        for s in (0, 128):
            losses.append(stepper.step(*table, index=idx[s:s + 128])["loss"].clone())
        runs[capture] = (torch.stack(losses), gd._cat.theta.clone(), stepper.m.clone(), stepper.v.clone())
        if capture:
            assert len(stepper.graphs) == 4
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(a, b)
    assert int(torch.isfinite(runs[True][0]).all())


def test_train_lowers_the_loss_and_its_state_loads_on_the_cpu():
    import attribute_scms.audio_mnist as aa
    ds = cc.onehot_ds(SIZES, 300, seed=6)
    torch.manual_seed(0)
    np.random.seed(0)
    g = aa.train({k: v.cuda() for k, v in ds.items()}, steps=3, device="cuda")
    assert g._cat is not None and len(g.train_losses) == 3 and g.train_losses[2] < g.train_losses[0]
    cpu = aa.AudioMNISTCausalGraph(ds, device="cpu")
    for k in ("native_speaker", "accent"):
        cpu.get_module(k).load_state_dict({n: t.cpu() for n, t in g.get_module(k).state_dict().items()})
    for a, b in zip(cc.linears(g)[4:12], cc.linears(cpu)[4:12]):              # the towers are not in any state_dict
        b.weight.data.copy_(a.weight.data.cpu())
        b.bias.data.copy_(a.bias.data.cpu())
    obs = {k: ds[k] for k in cc.TRIO}
    want = cpu.log_prob(obs)
    got = g.log_prob({k: v.cuda() for k, v in obs.items()})
    for k in ("native_speaker", "accent"):
        assert torch.allclose(got[k].detach().cpu(), want[k].detach(), rtol=1e-5, atol=1e-5)


def _fresh(seed):
    torch.manual_seed(seed)
    return cc.new_graph(SIZES, seed=8, device="cuda")


def test_sampling_entries_of_the_graph():
    n = 50
    gen = torch.Generator().manual_seed(0)
    country = torch.randint(0, SIZES[0], (n,), generator=gen).cuda()
    forb = torch.randint(0, SIZES[2], (n,), generator=gen).cuda()

    def run(g):
        s = g.sample({"country_of_origin": country})
        s2 = g.sample({"country_of_origin": country})
        d, status = g.sample_differing({"country_of_origin": country, "native_speaker": s["native_speaker"]}, "accent", forb)
        cf = g.sample_cf(s, {"native_speaker": 1 - s["native_speaker"]})
        return s, s2, d, status, cf

    g = _fresh(21)
    s, s2, d, status, cf = run(g)
    for out in (s, s2, d, cf):
        assert set(out) == set(g.modules)
        assert all(v.shape == (n,) and v.dtype == torch.int64 and v.is_cuda for v in out.values())
    assert all(int(s[k].max()) < c for k, c in zip(cc.TRIO, SIZES))
    assert status.shape == (n,) and status.dtype == torch.int32 and not status.any()
    assert not (d["accent"] == forb).any() and d["native_speaker"] is s["native_speaker"]
    assert torch.equal(cf["native_speaker"], 1 - s["native_speaker"]) and torch.equal(cf["digit"], s["digit"])
    # the stream's offset advances between calls: the second sample is another draw
    assert g._cat.offset == n * sum(SIZES[1:]) * 4 + n * 64 * SIZES[2]
    same = g.sample_cf(s, {})
    assert all(torch.equal(same[k], s[k]) for k in g.modules)
    assert not (torch.equal(s["native_speaker"], s2["native_speaker"]) and torch.equal(s["accent"], s2["accent"]))
    # a fresh graph with the same seed repeats everything
    again = run(_fresh(21))
    for a, b in zip((s, s2, d, cf), (again[0], again[1], again[2], again[4])):
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(status, again[3])
    # no draw of its own when nothing is held
    free = g.sample(n=33)
    assert all(v.shape == (33,) and v.is_cuda for v in free.values())
    noise = g.recover_noise(s)
    assert noise["native_speaker"].shape == (n, SIZES[1]) and noise["accent"].shape == (n, SIZES[2])
    assert torch.equal((g.get_module("native_speaker").model(torch.eye(SIZES[0], device="cuda")[country])
                        + noise["native_speaker"]).argmax(1), s["native_speaker"])


def test_a_changed_graph_runs_the_statement():
    g = _fresh(22)
    n = 20
    country = torch.zeros(n, dtype=torch.int64, device="cuda")
    g.sample({"country_of_origin": country})
    used = g._cat.offset
    assert used > 0
    g.add_edge("age", "gender")
    assert not g._cat.matches(g)
    s = g.sample({"country_of_origin": country})                      # Categorical.sample: the stream does not move
    assert g._cat.offset == used and s["accent"].shape == (n,) and s["accent"].dtype == torch.int64
    d, status = g.sample_differing({"country_of_origin": country}, "accent", torch.zeros(n, dtype=torch.int64, device="cuda"))
    assert g._cat.offset == used and not (d["accent"] == 0).any() and not status.any()
    ds = cc.onehot_ds(SIZES, 64, 1)
    lp = g.log_prob({k: ds[k].cuda() for k in cc.TRIO})
    assert lp["accent"].shape == (64,) and lp["accent"].grad_fn is not None and "CatLogProb" not in type(lp["accent"].grad_fn).__name__
    g.remove_edge("age", "gender")
    assert g._cat.matches(g)
    g.sample({"country_of_origin": country})
    assert g._cat.offset > used
