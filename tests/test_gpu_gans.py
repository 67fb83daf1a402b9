"""The ``gans/`` family on the device: the drop-in modules under autograd, ``GradientPenaltyFn`` and ``GanStepper``.

Reference: the same computation with stock torch on the stock modules (CPU tensors never touch the kernels) in fp64,
``torch.optim.Adam`` with betas (0.5, 0.9) for the steps; yardstick: the same in CPU fp32.  With e(t) = max|t - ref64|
every device output is held to e(device) <= 4 * e(cpu fp32) and e(device) <= 2e-4 * max|ref64| (the bounds of
test_gpu_conv_geometry.py).  The Discriminator's geometry fixes the image at 128 x 128; the cases shrink width and
batch: d = 4 with B = 3 (odd: row / tile tails) or B = 2, and one d = 8, B = 4 case whose 32-channel-stride layers take
the GEMM's uniform-tap loop.

Sign ties.  A whole-network comparison breaks where a LeakyReLU input lies within rounding noise of zero.  Every case
therefore takes the first seed in range(20) for which every fp64 pre-activation of D (and of G, where G is part of the
case) on every input of the case is farther from zero than 100 x the fp32-vs-fp64 deviation of that layer's
pre-activations (the maximum over the layer), and asserts that there is one; no element is skipped.  The biases are
placed around 3 standard deviations of their channel's convolution term from its mean, with random signs: the density
of pre-activations near zero drops by e^-4.5, about one element in 700 still has the sign opposite to its channel's
(some forty per image, in every layer), so the masks depend on the data and differ from image to image, and an early
seed qualifies although a case holds up to a million activations -- the search runs the fp64 reference once per seed
it tries.

CAP_ONLY lists the outputs held by the 2e-4 cap alone, each with its reason and the measured ratio.
"""
import copy
import functools

import pytest
import torch
import torch.nn as nn

RTOL = 2e-4     # of max|ref64|
YARD = 4.0      # times the deviation of the CPU fp32 evaluation
LR, BETAS, LAM = 1e-4, (0.5, 0.9), 10.0

gpu = pytest.mark.gpu

# (case, output) -> reason and measured figures (MI355X against the fp32 host evaluation next to it).  These outputs are
# held by the 2e-4 cap alone; every other output meets both bounds (largest measured ratio among them: 3.74).
CAP_ONLY = {
    # Adam's first update is lr * g / (|g| + 1e-8): where |g| comes near 1e-8 it follows the rounding error of g.  One of
    # this weight's 12800 gradient elements is 4.7e-8 (median 1.8e-3); there d(update)/dg = 311, so the 1e-9 by which two
    # fp32 evaluations of g differ moves the update by 3e-7, 0.3 % of lr.  Device 3.17e-7; the host's fp32 evaluation of
    # the same element gave 1.5e-8 on one machine and 2.4e-7 on another (ratio 20.5 / 1.3); 1.4e-6 of max|ref|.
    ("stepper_gan", "step 1 G.layers.5.weight"): "Adam update of a gradient element within 5x of its epsilon",
    # One number: the sum of B * 128 * 128 = 32768 products gy * tanh'.  The device's column sum adds them in blocks of
    # rows, the host pairwise.  Device 5.2e-7 (1.4e-6 of the value, the level of a blocked fp32 sum of 3e4 terms), host
    # 1.1e-7: ratio 4.89.
    ("stepper_gan", "step 2 G.layers.11.bias.exp_avg"): "a single 32768-term sum in another order",
    # Eight numbers, squares of sums of B * 32 * 32 = 2048 terms each: device 1.6e-9 (1.0e-6 of max|ref|), host 3.1e-10,
    # ratio 5.14 -- summation order again, doubled by the square.
    ("stepper_wgan", "step 2 G.layers.7.bias.exp_avg_sq"): "squares of 2048-term sums in another order",
    # 64 numbers with a handful of roundings each; the host's land within 0.3 ulp (1.3e-11, 3e-8 of max|ref|), the
    # device's within 1.7 ulp (9.1e-11, 2e-7 of max|ref|): ratio 6.88 at the resolution of the format.
    ("stepper_wgan", "step 2 D.layers.8.bias.exp_avg_sq"): "host result within 0.3 ulp; device within 1.7 ulp",
}


def check(case, name, got, ref64, f32, fails=None):
    """both bounds for output ``name`` of ``case``; prints the figures before it asserts.  ``fails`` (a list): collect
    the failures instead of stopping at the first, for ``assert not fails`` at the end of the test"""
    try:
        _check(case, name, got, ref64, f32)
    except AssertionError as e:
        if fails is None:
            raise
        fails.append(str(e))


def _check(case, name, got, ref64, f32):
    got, ref64, f32 = got.detach().double().cpu().reshape(ref64.shape), ref64.detach().double(), f32.detach().double()
    scale = ref64.abs().max().item()
    e_dev, e_cpu = (got - ref64).abs().max().item(), (f32 - ref64).abs().max().item()
    print(f"{case} {name}: device {e_dev:.3e}, cpu fp32 {e_cpu:.3e} (ratio {e_dev / max(e_cpu, 1e-300):.2f}), "
          f"max|ref| {scale:.3e}")
    if scale == 0.0:
        assert e_dev == 0.0, f"{case} {name}: the reference is exactly zero, the device is not ({e_dev:.3e})"
        return
    assert e_dev <= RTOL * scale, f"{case} {name}: max err {e_dev:.3e} vs {RTOL} * {scale:.3e}"
    if (case, name) not in CAP_ONLY:
        assert e_dev <= YARD * e_cpu, f"{case} {name}: max err {e_dev:.3e} > {YARD} * {e_cpu:.3e} (CPU fp32)"


# ---------------------------------------------------------------------- models and the tie-free seed
BIAS_K = 3.0


def init_(model, seed, probe):
    """O(1) activations whatever the depth, layer by layer on the ``probe`` batch: weights N(0, 1), then every output
    channel (every feature of the Generator's Linear) is scaled to standard deviation 1 and centred, and its bias is
    moved to +-BIAS_K * (0.8 .. 1.2) with a random sign (module docstring).  The last layer (no LeakyReLU behind it:
    logits, tanh inputs) is scaled to root mean square 1 as a whole and keeps biases a tenth of that."""
    g = torch.Generator().manual_seed(seed)
    x = probe
    mods = list(model.layers)
    with torch.no_grad():
        for i, m in enumerate(mods):
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))
                m.bias.zero_()
                y = m(x)
                sign = torch.randint(0, 2, m.bias.shape, generator=g).float() * 2 - 1
                mag = BIAS_K * (0.8 + 0.4 * torch.rand(m.bias.shape, generator=g))
                if not any(isinstance(n, nn.LeakyReLU) for n in mods[i + 1:]):
                    m.weight.div_(y.square().mean().sqrt())
                    m.bias.copy_(0.1 * sign * mag)
                else:
                    dims = [k for k in range(y.dim()) if k != 1]
                    mean, std = y.mean(dims), y.std(dims)
                    shape = [1] * m.weight.dim()
                    shape[1 if isinstance(m, nn.ConvTranspose2d) else 0] = -1
                    m.weight.div_(std.reshape(shape))
                    m.bias.copy_(sign * mag - mean / std)
            x = m(x)
    return model


def models(d, seed):
    import gans.audio_mnist as gm
    g = torch.Generator().manual_seed(1000 + seed)
    G = init_(gm.Generator(d), 2 * seed, torch.randn(32, 100, generator=g))
    D = init_(gm.Discriminator(d), 2 * seed + 1, torch.rand(8, 1, 128, 128, generator=g) * 2 - 1)
    return G, D


def preacts(net, x):
    """the LeakyReLU inputs of a stock ``layers`` stack on input ``x``"""
    out = []
    mods = list(net.layers)
    with torch.no_grad():
        for i, m in enumerate(mods):
            x = m(x)
            if i + 1 < len(mods) and isinstance(mods[i + 1], nn.LeakyReLU):
                out.append(x)
    return out


def ties(net64, x64):
    """number of fp64 pre-activations of ``net64`` on ``x64`` within 100 x the layer's fp32-vs-fp64 deviation of zero"""
    net32 = copy.deepcopy(net64).float()
    n = 0
    for p64, p32 in zip(preacts(net64, x64), preacts(net32, x64.float())):
        dev = (p32.double() - p64).abs().max().item()
        n += int((p64.abs() <= 100 * dev).sum())
    return n


def first_seed(build):
    """``build(seed)`` -> (case, [(net64, x64), ...]): the case of the first seed in range(20) without a sign tie"""
    for seed in range(20):
        case, watched = build(seed)
        if sum(ties(net, x) for net, x in watched) == 0:
            print(f"tie-free seed: {seed}")
            return case
    raise AssertionError("no seed in range(20) gives a case without LeakyReLU sign ties")


def grads_of(model):
    return {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}


# ---------------------------------------------------------------------- modules under autograd
@functools.lru_cache(maxsize=None)
def module_case(which, d, B):
    """``which`` = "G" | "D": (net, input, cotangent of its output, fp64 results, CPU fp32 results); G and D are compared
    on their own, so each picks its own seed"""
    def build(seed):
        net = models(d, seed)[0 if which == "G" else 1]
        g = torch.Generator().manual_seed(100 + seed)
        if which == "G":
            x, cot = torch.randn(B, 100, generator=g), torch.randn(B, 1, 128, 128, generator=g)
        else:
            x, cot = torch.rand(B, 1, 128, 128, generator=g) * 2 - 1, torch.randn(B, 1, generator=g)
        return (net, x, cot), [(copy.deepcopy(net).double(), x.double())]
    net, x, cot = first_seed(build)
    ref = {dt: run_module(copy.deepcopy(net).to(dt), x.to(dt), cot.to(dt)) for dt in (torch.float64, torch.float32)}
    return net, x, cot, ref[torch.float64], ref[torch.float32]


def run_module(net, x, cot):
    xx = x.clone().requires_grad_(True)
    net.zero_grad()
    y = net(xx)
    (y * cot).sum().backward()
    out = {"output": y.detach(), "input.grad": xx.grad}
    out.update({f"{k}.grad": v for k, v in grads_of(net).items()})
    return out


@gpu
@pytest.mark.parametrize("d,B", [(4, 3), (8, 4)])
@pytest.mark.parametrize("which", ["G", "D"])
def test_modules_forward_and_gradients_vs_fp64(which, d, B):
    net, x, cot, r64, r32 = module_case(which, d, B)
    dev = copy.deepcopy(net).cuda()
    got = run_module(dev, x.cuda(), cot.cuda())
    assert got["output"].shape == ((B, 1, 128, 128) if which == "G" else (B, 1)) and dev.device.type == "cuda"
    fails = []
    for k in r64:
        check(f"{which}_d{d}_b{B}", k, got[k], r64[k], r32[k], fails)
    assert not fails, "\n".join(fails)
    with torch.no_grad():       # [B, 100, 1, 1] latents and [B, 128, 128] images, as the reference's reshapes take them
        alt = x.cuda().reshape((B, 100, 1, 1) if which == "G" else (B, 128, 128))
        assert torch.equal(dev(alt), got["output"])


# ---------------------------------------------------------------------- the gradient penalty
def penalty_torch(D, x):
    """value and gradients of the unweighted penalty by create_graph + backward on the stock modules"""
    import gans.audio_mnist as gm
    D.zero_grad()
    xx = x.clone().requires_grad_(True)
    pen = gm.compute_gradient_penalty(D, xx)
    pen.backward()
    return pen.detach(), grads_of(D), (xx.grad if xx.grad is not None else torch.zeros_like(xx))


@functools.lru_cache(maxsize=None)
def penalty_case(d, B):
    def build(seed):
        _, D = models(d, seed)
        x = torch.rand(B, 1, 128, 128, generator=torch.Generator().manual_seed(200 + seed)) * 2 - 1
        return (D, x), [(copy.deepcopy(D).double(), x.double())]
    D, x = first_seed(build)
    return D, x, penalty_torch(copy.deepcopy(D).double(), x.double()), penalty_torch(copy.deepcopy(D), x)


@gpu
def test_gradient_penalty_fn_vs_create_graph_backward():
    import gans.audio_mnist as gm
    from ali_hip.chain import get_plan
    from ali_hip.gan import GradientPenaltyFn
    d, B = 4, 3
    D, x, (p64, g64, gx64), (p32, g32, gx32) = penalty_case(d, B)
    assert float(gx64.abs().max()) == 0.0 and all(float(g64[k].abs().max()) == 0.0 for k in g64 if k.endswith("bias"))
    Dd = copy.deepcopy(D).cuda()
    plan = get_plan(Dd.layers)
    for how in ("GradientPenaltyFn", "compute_gradient_penalty"):
        Dd.zero_grad()
        xd = x.cuda().requires_grad_(True)
        pen = (GradientPenaltyFn.apply(plan, xd, *plan.params()) if how == "GradientPenaltyFn"
               else gm.compute_gradient_penalty(Dd, xd))
        assert pen.dim() == 0 and pen.requires_grad
        (pen * 1.5).backward()                  # an incoming gradient other than 1
        check(f"gp_d{d}_b{B}", f"{how} value", pen, p64, p32)
        got = grads_of(Dd)
        for k in g64:
            check(f"gp_d{d}_b{B}", f"{how} {k}.grad", got[k], 1.5 * g64[k], 1.5 * g32[k])
        assert xd.grad is None or float(xd.grad.abs().max()) == 0.0


@gpu
def test_wgan_loop_body_statement_runs_unchanged():
    """the reference's D-step statement on CUDA modules: loss, backward, torch.optim step"""
    import gans.audio_mnist as gm
    G, D = models(4, 0)
    G, D = G.cuda(), D.cuda()
    opt = torch.optim.Adam(D.parameters(), lr=LR, betas=BETAS)
    before = [p.detach().clone() for p in D.parameters()]
    images = torch.rand(2, 1, 128, 128, device="cuda") * 2 - 1
    opt.zero_grad()
    loss_D = gm.wgan_loss_it(D, images, G(torch.randn(2, 100, device="cuda"))).mean()
    loss_D.backward()
    opt.step()
    # every weight and conv bias moves; the head's bias does not: d/dc of D(x~) - D(x) is 1 - 1, the penalty's is zero
    moved = {k: not torch.equal(a, p) for a, (k, p) in zip(before, D.named_parameters())}
    assert torch.isfinite(loss_D) and not moved.pop("layers.11.bias") and all(moved.values()), moved


# ---------------------------------------------------------------------- the stepper
def loop_body(G, D, oG, oD, images, z_g, z_d, z_s, eps, mode, do_g=True, watch=None):
    """gans/audio_mnist.py:300-337 with given draws; ``watch`` collects (net, input) of every D / G forward"""
    bce = nn.BCEWithLogitsLoss()
    n = len(images)
    valid, fake = torch.ones(n, 1, dtype=images.dtype), torch.zeros(n, 1, dtype=images.dtype)
    out = {}

    def seen(net, x):
        if watch is not None:
            watch.append((copy.deepcopy(net), x.detach().clone()))

    if do_g:
        oG.zero_grad()
        seen(G, z_g)
        gen = G(z_g)
        seen(D, gen)
        loss_G = bce(D(gen), valid) if mode == "gan" else -D(gen).mean()
        loss_G.backward()
        oG.step()
        out["loss_G"] = loss_G.detach()
    oD.zero_grad()
    seen(G, z_d)
    gz = G(z_d)
    seen(D, gz)
    seen(D, images)
    if mode == "gan":
        loss_D = (bce(D(images), valid) + bce(D(gz), fake)) / 2
    else:
        e = eps.reshape(n, 1, 1, 1)
        xhat = e * images + (1 - e) * gz
        seen(D, xhat)
        gradients = torch.autograd.grad(D(xhat).sum(), xhat, create_graph=True)[0]
        pen = ((gradients.reshape(n, -1).norm(2, dim=1) - 1) ** 2).mean()
        loss_D = (D(gz) - D(images) + LAM * pen).mean()
    loss_D.backward()
    oD.step()
    out["loss_D"] = loss_D.detach()
    with torch.no_grad():
        seen(G, z_s)
        gs = G(z_s)
        seen(D, gs)
        seen(D, images)
        DG, DE = D(gs), D(images)
        if mode == "gan":
            DG, DE = DG.sigmoid(), DE.sigmoid()
        out["DG"], out["DE"] = DG.mean(), DE.mean()
    return out


def run_loop(G, D, draws, mode, dtype, steps=2, watch=None):
    G, D = copy.deepcopy(G).to(dtype), copy.deepcopy(D).to(dtype)
    oG = torch.optim.Adam(G.parameters(), lr=LR, betas=BETAS)
    oD = torch.optim.Adam(D.parameters(), lr=LR, betas=BETAS)
    hist = []
    for s in range(steps):
        images, z_g, z_d, z_s, eps = (t.to(dtype) for t in draws[s])
        r = loop_body(G, D, oG, oD, images, z_g, z_d, z_s, eps, mode, watch=watch)
        snap = {"scalars": r, "G": {k: v.detach().clone() for k, v in G.state_dict().items()},
                "D": {k: v.detach().clone() for k, v in D.state_dict().items()}}
        for nm, m, o in (("G", G, oG), ("D", D, oD)):
            for (k, p) in m.named_parameters():
                snap[f"{nm}.{k}.exp_avg"] = o.state[p]["exp_avg"].clone()
                snap[f"{nm}.{k}.exp_avg_sq"] = o.state[p]["exp_avg_sq"].clone()
        hist.append(snap)
    return hist


def make_draws(B, seed, steps=2):
    g = torch.Generator().manual_seed(300 + seed)
    return [(torch.rand(B, 1, 128, 128, generator=g) * 2 - 1, torch.randn(B, 100, generator=g),
             torch.randn(B, 100, generator=g), torch.randn(B, 100, generator=g), torch.rand(B, generator=g))
            for _ in range(steps)]


@functools.lru_cache(maxsize=None)
def stepper_case(mode, d=4, B=2):
    def build(seed):
        G, D = models(d, seed)
        draws = make_draws(B, seed)
        watch = []
        h64 = run_loop(G, D, draws, mode, torch.float64, watch=watch)
        return (G, D, draws, h64), watch
    G, D, draws, h64 = first_seed(build)
    return G, D, draws, h64, run_loop(G, D, draws, mode, torch.float32)


def dev_draws(step):
    return [t.cuda() for t in step]


@gpu
@pytest.mark.parametrize("mode", ["gan", "wgan"])
def test_stepper_two_steps_vs_the_fp64_loop(mode):
    from ali_hip.gan import GanStepper
    G, D, draws, h64, h32 = stepper_case(mode)
    Gd, Dd = copy.deepcopy(G).cuda(), copy.deepcopy(D).cuda()
    stepper = GanStepper(Gd, Dd, lr=LR, betas=BETAS, loss_mode=mode, penalty_weight=LAM)
    case = f"stepper_{mode}"
    r = stepper.step(*dev_draws(draws[0]))
    assert set(r) == {"loss_G", "loss_D", "DG", "DE"} and all(v.dim() == 0 and v.is_cuda for v in r.values())
    fails = []
    for k in ("loss_G", "loss_D", "DG", "DE"):
        check(case, f"step 1 {k}", r[k], h64[0]["scalars"][k], h32[0]["scalars"][k], fails)
    for nm, m in (("G", Gd), ("D", Dd)):
        for k, v in m.state_dict().items():
            check(case, f"step 1 {nm}.{k}", v, h64[0][nm][k], h32[0][nm][k], fails)
    stepper.step(*dev_draws(draws[1]))
    sd = stepper.state_dict()
    for nm, m in (("G", Gd), ("D", Dd)):
        opt = sd[f"optimizer_{nm}"]["state"]
        for i, (k, _) in enumerate(m.named_parameters()):
            assert float(opt[i]["step"]) == 2.0
            for mom in ("exp_avg", "exp_avg_sq"):
                check(case, f"step 2 {nm}.{k}.{mom}", opt[i][mom], h64[1][f"{nm}.{k}.{mom}"], h32[1][f"{nm}.{k}.{mom}"],
                      fails)
    assert sd["iteration"] == 2
    assert not fails, "\n".join(fails)


def _run_steps(mode, capture, n=3, k=1, seed=5, given=True):
    from ali_hip.gan import GanStepper
    G, D = models(4, 1)
    Gd, Dd = G.cuda(), D.cuda()
    stepper = GanStepper(Gd, Dd, lr=LR, betas=BETAS, loss_mode=mode, d_updates_per_g_update=k, capture=capture, seed=seed)
    draws = make_draws(2, 77, steps=n)
    res = []
    for s in range(n):
        r = stepper.step(*dev_draws(draws[s])) if given else stepper.step(draws[s][0].cuda())
        res.append({k_: v.clone() for k_, v in r.items()})
    return stepper, res


def _same_state(a, b):
    return all(torch.equal(p, q) for m, n in ((a.G, b.G), (a.D, b.D)) for p, q in zip(m.parameters(), n.parameters())) \
        and all(torch.equal(getattr(g, t), getattr(h, t)) for g, h in ((a.opt_g, b.opt_g), (a.opt_d, b.opt_d))
                for t in ("m", "v", "step_t"))


@gpu
@pytest.mark.parametrize("given", [True, False], ids=["given_draws", "device_draws"])
@pytest.mark.parametrize("mode", ["gan", "wgan"])
def test_captured_steps_replay_the_eager_ones_bit_for_bit(mode, given):
    eager, res_e = _run_steps(mode, False, given=given)
    graph, res_c = _run_steps(mode, True, given=given)
    assert len(graph._graphs) == 1
    for a, b in zip(res_e, res_c):
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert _same_state(eager, graph)
    assert int(graph.opt_d.step_t.item()) == 3 and int(graph.iter_t.item()) == 3
    if not given:                                       # the counter moved: other draws, other scores
        assert not torch.equal(res_e[0]["DG"], res_e[1]["DG"])


@gpu
def test_device_draws_are_the_counter_streams():
    """z_g / z_d / z_s and eps drawn on the device equal the host recipes keyed (seed, iteration)"""
    from ali_hip import source
    drawn, res_a = _run_steps("wgan", False, n=2, seed=9, given=False)
    B, draws = 2, make_draws(2, 77, steps=2)
    from ali_hip.gan import GanStepper
    G, D = models(4, 1)
    ref = GanStepper(G.cuda(), D.cuda(), lr=LR, betas=BETAS, loss_mode="wgan", seed=9)
    for it in range(2):
        z = source.normal_reference(9, it, 3 * B * 100).float().reshape(3, B, 100).cuda()
        e = source.uniform_reference(9, it, B).cuda()
        r = ref.step(draws[it][0].cuda(), z[0], z[1], z[2], e)
        # (the device's fp32 Box-Muller differs from the fp64 recipe by roundings: the scores agree to a few ulps)
        for k in r:
            assert float((r[k] - res_a[it][k]).abs()) <= 1e-4 * max(1.0, float(r[k].abs())), (it, k)


@gpu
def test_two_d_updates_per_g_update_leave_g_untouched_on_odd_iterations():
    stepper, res = _run_steps("gan", False, n=0, k=2)
    draws = make_draws(2, 77, steps=3)
    snaps = []
    for s in range(3):
        before = [p.detach().clone() for p in stepper.G.parameters()]
        d_before = [p.detach().clone() for p in stepper.D.parameters()]
        r = stepper.step(*dev_draws(draws[s]))
        same = all(torch.equal(a, p) for a, p in zip(before, stepper.G.parameters()))
        assert not any(torch.equal(a, p) for a, p in zip(d_before, stepper.D.parameters()))
        snaps.append(("loss_G" in r, same))
    assert snaps == [(True, False), (False, True), (True, False)]
    assert int(stepper.opt_g.step_t.item()) == 2 and int(stepper.opt_d.step_t.item()) == 3


@gpu
@pytest.mark.parametrize("mode", ["gan", "wgan"])
def test_state_dict_round_trip_resumes_bit_identically(mode):
    from ali_hip.gan import GanStepper
    full, res = _run_steps(mode, False, n=3, given=False)
    part, _ = _run_steps(mode, False, n=2, given=False)
    sd = part.state_dict()
    # the optimiser entries are torch.optim.Adam state dicts
    opt = torch.optim.Adam(part.D.parameters(), lr=LR, betas=BETAS)
    opt.load_state_dict(copy.deepcopy(sd["optimizer_D"]))
    assert float(opt.state[next(iter(part.D.parameters()))]["step"]) == 2.0
    G, D = models(4, 3)                               # other weights: everything comes from the checkpoint
    fresh = GanStepper(G.cuda(), D.cuda(), lr=LR, betas=BETAS, loss_mode=mode, seed=5)
    fresh.load_state_dict(sd)
    r = fresh.step(make_draws(2, 77, steps=3)[2][0].cuda())
    assert all(torch.equal(r[k], res[2][k]) for k in r)
    assert _same_state(full, fresh)


@gpu
def test_stepper_argument_errors():
    from ali_hip.gan import GanStepper
    G, D = models(4, 0)
    G, D = G.cuda(), D.cuda()
    with pytest.raises(NotImplementedError, match="weight_decay"):
        GanStepper(G, D, discriminator_weight_decay=0.1)
    with pytest.raises(ValueError):
        GanStepper(G, D).step(torch.zeros(2, 1, 128, 128))


@gpu
@pytest.mark.parametrize("mode", ["gan", "wgan"])
def test_train_runs_two_iterations_on_a_waveform_source(mode):
    import gans.audio_mnist as gm
    from ali_hip.step import FlatGroup
    from image_scms import _spect
    from image_scms.audio_mnist import STFT
    g = torch.Generator().manual_seed(0)
    data = _spect.WaveformData(torch.randn(4, 8000, generator=g) * 0.1, {}, **STFT, device="cuda")
    G, D, oD, oG = gm.train(data, n_epochs=1, device="cuda", batch_size=2, generator_size=4, discriminator_size=4,
                            loss_mode=mode, save_images_every=None)
    assert isinstance(G, gm.Generator) and isinstance(D, gm.Discriminator)
    assert isinstance(oD, FlatGroup) and isinstance(oG, FlatGroup)
    assert oD.state_dict()["step"] == 2 and oG.state_dict()["step"] == 2
    assert all(torch.isfinite(p).all() for m in (G, D) for p in m.parameters())
