"""The cf_metrics family on the device: ReLU stages and the large ``Flatten -> Linear`` of ``ali_hip.chain``, the
drop-in ``Encoder`` / ``Decoder``, ``AeStepper`` and ``CfMetrics``.

Reference: the stock modules under autograd on the CPU in fp64 (CPU inputs never touch the kernels); yardstick: the same
in CPU fp32; bounds: ``_check`` of test_gpu_xent.py (YARD x the CPU-fp32 error and RTOL of max|ref64|, both from
test_gpu_conv_geometry.py).  Sign ties: the ``TieWatch`` criterion of test_gpu_modules.py, applied to the inputs of the
``nn.ReLU`` modules -- a pre-activation within fp32 summation noise of zero (4e-7 of the largest) switches the
derivative between 1 and 0 with the summation order, so inputs are re-seeded until the fp64 forward has none.  A
pre-activation of EXACTLY zero is no tie: every evaluation agrees on it, and its derivative is 0, as torch's.

One stepper step is taken apart as in test_gpu_classifiers.py: loss and every gradient by both bounds, the updated
weights against an fp64 Adam step at the device's gradient (1e-6 * lr + 6e-8 * max|w|), and against the fp64
restatement's weights by the statistics of ``_check_encoder_update``.
"""
import copy

import pytest
import torch
import torch.nn as nn

from test_cfmetrics_cpu import metrics_case
from test_gpu_callers import _check_encoder_update
from test_gpu_classifier_chain import autograd_pass, compare_with_autograd
from test_gpu_xent import _check

gpu = pytest.mark.gpu
LR = 1e-4


class ReluWatch:
    """``TieWatch`` for nn.ReLU inputs; exact zeros are not counted (see the module docstring)"""

    def __init__(self, *mods):
        self.ties = 0
        self.hooks = [m.register_forward_hook(self._hook) for mod in mods for m in mod.modules()
                      if isinstance(m, nn.ReLU)]

    def _hook(self, mod, inp, out):
        x = inp[0].detach().abs()
        self.ties += int(((x > 0) & (x <= 4e-7 * x.max())).sum())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()


def relu_tie_free(mods, make, run, tries=24):
    for v in range(tries):
        args = make(v)
        with ReluWatch(*mods) as tw, torch.no_grad():
            run(*args)
        if tw.ties == 0:
            return args
    pytest.fail(f"no tie-free case in {tries} draws")


class NhwcStack(nn.Sequential):
    """a conv stack whose CUDA batches run on ``ali_hip.chain`` and come back as [B,C,H,W]"""

    def forward(self, x):
        if not x.is_cuda:
            return super().forward(x)
        from ali_hip.chain import run_chain
        from ali_hip.classify import nhwc_input
        return run_chain(self, nhwc_input(x), x.shape[1]).permute(0, 3, 1, 2)


def _stack_case(model, in_shape, seed):
    ref64 = copy.deepcopy(model).double()
    with torch.no_grad():
        out_shape = tuple(ref64(torch.zeros(in_shape, dtype=torch.float64)).shape)

    def make(v):
        g = torch.Generator().manual_seed(seed + v)
        return torch.randn(in_shape, generator=g), torch.randn(out_shape, generator=g)
    return relu_tie_free([ref64], make, lambda x, cot: ref64(x.double()))


# ------------------------------------------------------------------------------------------------------- ReLU stages
@gpu
def test_conv_relu_conv_chain_vs_fp64_autograd():
    torch.manual_seed(41)
    model = NhwcStack(nn.Conv2d(1, 8, 3), nn.ReLU(), nn.Conv2d(8, 6, 3, 2, 1))
    x, cot = _stack_case(model, (3, 1, 9, 11), 400)
    compare_with_autograd(model, x, cot, "conv-relu-conv")


@gpu
def test_conv_transpose_relu_chain_vs_fp64_autograd():
    torch.manual_seed(42)
    model = NhwcStack(nn.ConvTranspose2d(8, 12, 4, 2, 1), nn.ReLU())
    x, cot = _stack_case(model, (3, 8, 5, 7), 410)
    compare_with_autograd(model, x, cot, "convT-relu")


@gpu
def test_pre_activations_of_exactly_zero_get_gradient_zero():
    torch.manual_seed(43)
    model = NhwcStack(nn.Conv2d(1, 8, 3), nn.ReLU(), nn.Conv2d(8, 4, 3))
    with torch.no_grad():
        model[0].weight[3].zero_()                 # channel 3: 0 * x + 0 on every device
        model[0].bias[3] = 0.0
    x, cot = _stack_case(model, (2, 1, 8, 8), 420)
    compare_with_autograd(model, x, cot, "zero channel")
    yd, gxd, gpd = autograd_pass(model, x, cot, device="cuda")
    _, _, gp64 = autograd_pass(model, x, cot, torch.float64)
    assert torch.equal(gp64["0.weight"][3], torch.zeros(1, 3, 3, dtype=torch.float64)) and gp64["0.bias"][3] == 0
    assert torch.equal(gpd["0.weight"][3].cpu(), torch.zeros(1, 3, 3)) and gpd["0.bias"][3].item() == 0.0


# --------------------------------------------------------------------------------------------------- the large flatten
@gpu
@pytest.mark.parametrize("C,O", [(8, 4), (8, 10), (128, 4), (128, 10)])
def test_flatten_linear_on_a_7x7_map(C, O):
    from ali_hip.chain import get_plan, trace
    from classifiers._stack import ClassifierStack
    torch.manual_seed(50 + C + O)
    model = ClassifierStack(nn.Flatten(), nn.Linear(49 * C, O))
    assert trace(get_plan(model), (3, 7, 7, C), C)[0][2].fwd == "flat_gemm"
    g = torch.Generator().manual_seed(C * O)
    x, cot = torch.randn(3, C, 7, 7, generator=g), torch.randn(3, O, generator=g)
    compare_with_autograd(model, x, cot, f"flatten 7x7 C={C} O={O}")


@gpu
def test_conv_relu_flatten_linear_end_to_end():
    """the flatten behind a conv stage: its data gradient carries the ReLU derivative in its epilogue"""
    from classifiers._stack import ClassifierStack
    torch.manual_seed(55)
    model = ClassifierStack(nn.Conv2d(1, 8, 4, 2, 1), nn.ReLU(), nn.Flatten(), nn.Linear(8 * 36, 5))
    x, cot = _stack_case(model, (3, 1, 12, 12), 430)
    compare_with_autograd(model, x, cot, "conv-relu-flatten-linear")


# ---------------------------------------------------------------------------------------------------- Encoder / Decoder
def _ae_case(c, latent, B, seed=60):
    """(E, G, x): fp32 CPU modules and a batch whose fp64 pass through both has no ReLU tie"""
    import train_morphomnist_ae as ae
    torch.manual_seed(seed + c)
    E, G = ae.Encoder(c, latent), ae.Decoder(c, latent)
    E64, G64 = copy.deepcopy(E).double().chain_view(), copy.deepcopy(G).double().chain_view()

    def make(v):
        return (torch.rand(B, 1, 28, 28, generator=torch.Generator().manual_seed(seed + 7 * v)) * 2 - 1,)
    (x,) = relu_tie_free([E64, G64], make, lambda x: G64(E64(x.double())))
    return E, G, x


@gpu
@pytest.mark.parametrize("c,latent,B", [(64, 10, 2), (8, 4, 5)])
def test_encoder_and_decoder_vs_the_fp64_modules(c, latent, B):
    E, G, x = _ae_case(c, latent, B)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        z = E(x)
    compare_with_autograd(E, x, torch.randn(B, latent, generator=g), f"Encoder({c},{latent})")
    compare_with_autograd(G, z, torch.randn(B, 1, 28, 28, generator=g), f"Decoder({c},{latent})")


def _loss_pass(E, G, x, dtype=None, device="cpu"):
    E, G = copy.deepcopy(E), copy.deepcopy(G)
    if dtype is not None:
        E, G, x = E.to(dtype), G.to(dtype), x.to(dtype)
    E, G, x = E.to(device), G.to(device), x.to(device)
    loss = (x - G(E(x))).square().mean()
    loss.backward()
    grads = {f"E.{k}": p.grad for k, p in E.named_parameters()}
    grads.update({f"G.{k}": p.grad for k, p in G.named_parameters()})
    return loss.detach(), grads


@gpu
def test_loss_backward_through_both_modules():
    E, G, x = _ae_case(8, 4, 5)
    l64, g64 = _loss_pass(E, G, x, torch.float64)
    l32, g32 = _loss_pass(E, G, x, torch.float32)
    ld, gd = _loss_pass(E, G, x, device="cuda")
    _check("ae loss", ld, l64, l32)
    for k in g64:
        _check(f"ae {k}.grad", gd[k], g64[k], g32[k])


# ------------------------------------------------------------------------------------------------------------ AeStepper
def _reference_step(E, G, x, dtype):
    E, G = copy.deepcopy(E).to(dtype), copy.deepcopy(G).to(dtype)
    opt = torch.optim.Adam(list(E.parameters()) + list(G.parameters()), lr=LR, betas=(0.5, 0.9))
    opt.zero_grad()
    loss = (x.to(dtype) - G(E(x.to(dtype)))).square().mean()
    loss.backward()
    grads = {("E", k): p.grad.clone() for k, p in E.named_parameters()}
    grads.update({("G", k): p.grad.clone() for k, p in G.named_parameters()})
    opt.step()
    return E, G, loss.detach(), grads


@gpu
@pytest.mark.parametrize("c,latent,B", [(64, 10, 2), (8, 4, 5)])
def test_one_stepper_step_taken_apart(c, latent, B):
    from ali_hip.cfmetrics import AeStepper
    E, G, x = _ae_case(c, latent, B)
    E64, G64, loss64, g64 = _reference_step(E, G, x, torch.float64)
    _, _, loss32, g32 = _reference_step(E, G, x, torch.float32)
    Ed, Gd = copy.deepcopy(E).cuda(), copy.deepcopy(G).cuda()
    before = {n: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for n, m in (("E", Ed), ("G", Gd))}
    stepper = AeStepper(Ed, Gd, lr=LR)
    r = stepper.step(x.cuda())
    assert r["loss"].dim() == 0
    _check(f"ae({c},{latent}) loss", r["loss"], loss64, loss32)
    for n, m in (("E", Ed), ("G", Gd)):
        for k, p in m.named_parameters():
            gd = stepper.opt.grad_views[id(p)].detach().cpu()
            _check(f"ae({c},{latent}) {n}.{k}.grad", gd, g64[(n, k)], g32[(n, k)])
            g = gd.double()
            want = before[n][k].double() - LR * (g / (g.abs() + 1e-8))     # Adam's first step at the device's gradient
            err = (p.detach().cpu().double() - want).abs().max().item()
            bound = 1e-6 * LR + 6e-8 * before[n][k].abs().max().item()
            print(f"AE {n}.{k} update err={err:.3e} bound={bound:.3e}")
            assert err <= bound, (n, k, err, bound)
    _check_encoder_update(E64.float(), Ed, before["E"], LR, 1)
    _check_encoder_update(G64.float(), Gd, before["G"], LR, 1)


@gpu
def test_captured_and_eager_steps_agree_bit_for_bit():
    from ali_hip.cfmetrics import AeStepper
    E, G, x = _ae_case(8, 4, 5)
    xs = [x.cuda(), (x * 0.5).cuda(), (-x).cuda()]
    out = []
    for capture in (False, True):
        Ed, Gd = copy.deepcopy(E).cuda(), copy.deepcopy(G).cuda()
        stepper = AeStepper(Ed, Gd, lr=LR, capture=capture)
        losses = [stepper.step(xi)["loss"].clone() for xi in xs]
        out.append((losses, [p.detach().clone() for p in list(Ed.parameters()) + list(Gd.parameters())],
                    int(stepper.opt.step_t.item())))
        if capture:
            assert len(stepper._graphs) == 1
    (l_e, w_e, n_e), (l_c, w_c, n_c) = out
    assert n_e == n_c == 3
    for a, b in zip(l_e + w_e, l_c + w_c):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------- checkpoints
@gpu
def test_checkpoint_saved_from_the_cpu_modules_runs_on_the_device(tmp_path):
    import train_morphomnist_ae as ae
    E, G, x = _ae_case(8, 4, 5)
    torch.save({"E": E, "G": G}, tmp_path / "ae.tar")
    back = torch.load(tmp_path / "ae.tar", map_location="cuda", weights_only=False)
    Ed, Gd = back["E"], back["G"]
    assert next(Ed.parameters()).is_cuda and next(Gd.parameters()).is_cuda
    E2, G2 = ae.Encoder(8, 4).cuda(), ae.Decoder(8, 4).cuda()          # the state_dict flavour
    E2.load_state_dict(E.state_dict())
    G2.load_state_dict(G.state_dict())
    with torch.no_grad():
        r64 = copy.deepcopy(G).double()(copy.deepcopy(E).double()(x.double()))
        r32 = G(E(x))
        _check("checkpoint pickle", Gd(Ed(x.cuda())), r64, r32)
        _check("checkpoint state_dict", G2(E2(x.cuda())), r64, r32)


# ------------------------------------------------------------------------------------------------------------ CfMetrics
def _to(mods, f):
    if isinstance(mods, dict):
        return {k: (f(copy.deepcopy(e)), f(copy.deepcopy(g))) for k, (e, g) in mods.items()}
    return [f(copy.deepcopy(m)) for m in mods]


@gpu
def test_cfmetrics_on_the_device():
    from ali_hip.cfmetrics import CfMetrics
    clf, aes, oracles, x, cf, orig = metrics_case(torch.float32)
    target = (orig + 3) % 10
    ref = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = CfMetrics(_to([clf], lambda t: t.to(dt))[0], _to(aes, lambda t: t.to(dt)), _to(oracles, lambda t: t.to(dt)))
        ref[name] = [m.add(x.to(dt), cf.to(dt), orig), m.add(x.to(dt), cf.to(dt), orig, target)]
        ref[name + "_logits"] = m.clf(cf.to(dt))
    dev = lambda t: t.cuda()       # noqa: E731
    clf_d, aes_d, or_d = _to([clf], dev)[0], _to(aes, dev), _to(oracles, dev)
    xd, cfd, od, td = x.cuda(), cf.cuda(), orig.cuda(), target.cuda()
    outs = {}
    for capture in (False, True):
        m = CfMetrics(clf_d, aes_d, or_d, capture=capture)
        got = [m.add(xd, cfd, od, t) for t in (None, td)]
        outs[capture] = got
        if capture:
            assert len(m._graphs) == 2                       # (target None / given: two signatures)
            # 2B rows in order
            t = m.table("cf")
            assert t["cf_label"].tolist() == got[0]["label"].tolist() + got[1]["label"].tolist()
            assert t["t_rec_cf"].tolist() == got[0]["t_rec"].tolist() + got[1]["t_rec"].tolist()
            assert t["cf_os_1"].tolist() == got[0]["os"][:, 1].tolist() + got[1]["os"][:, 1].tolist()
            assert t["cf_lvs_0"].tolist() == got[0]["lvs"][:, 0].tolist() + got[1]["lvs"][:, 0].tolist()
            # a second batch shape makes another graph; a changed weight drops them all
            m.add(xd[:3], cfd[:3], od[:3], td[:3])
            assert len(m._graphs) == 3 and len(m.table("cf")["cf_label"]) == 13
            # what add returned stays the caller's: a replay of the same graph on other data does not touch it
            held = {k: v.clone() for k, v in got[1].items()}
            other = m.add(xd, -cfd, od, td)
            assert len(m._graphs) == 3 and not torch.equal(other["o_rec"], held["o_rec"])
            for k in held:
                assert torch.equal(got[1][k], held[k]), k
            # a changed weight drops the graphs, and the new ones see it: the "all" autoencoder moves all_rec of every
            # row and nothing else
            with torch.no_grad():
                aes_d["all"][0].fc.bias.add_(0.125)
            again = m.add(xd, cfd, od, td)
            assert len(m._graphs) == 1
            for k in ("label", "l1", "o_rec", "t_rec", "os", "lvs"):
                assert torch.equal(again[k], held[k]), k
            assert bool((again["all_rec"] != held["all_rec"]).all())
    for a, b in zip(outs[False], outs[True]):                # captured and eager: the same bits
        for k in a:
            assert torch.equal(a[k], b[k]), k
    with torch.no_grad():
        logits_d = clf_d(cfd)
        _check("cfmetrics clf logits", logits_d, ref["f64_logits"], ref["f32_logits"])
        want_label = logits_d.argmax(1)
        oc = [o(cfd).argmax(1) for o in or_d]
    # the case is one whose labels no rounding moves (checked on the CPU: fp64 and fp32 agree), so target=None rows
    # read the same autoencoder in every evaluation
    assert torch.equal(ref["f64"][0]["label"], ref["f32"][0]["label"]), "pick another seed in metrics_case"
    assert torch.equal(want_label.cpu(), ref["f64"][0]["label"]), "pick another seed in metrics_case"
    for i, got in enumerate(outs[True]):
        assert torch.equal(got["label"].long(), want_label)
        assert torch.equal(got["os"].long(), torch.stack([(want_label == c).long() for c in oc], dim=1))
        for k in ("l1", "o_rec", "t_rec", "all_rec", "lvs"):
            _check(f"cfmetrics[{i}] {k}", got[k], ref["f64"][i][k], ref["f32"][i][k])
