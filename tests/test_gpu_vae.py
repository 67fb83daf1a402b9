"""The three conditional VAEs of ``deepscm_vae/`` and the executors of ``ali_hip.vae`` on the device.

Reference: the stock-torch statement of the same modules and weights in fp64 on the CPU (CPU inputs never touch the
kernels), ``torch.optim.Adam`` for the steps; yardstick: the same in CPU fp32; the two bounds of
test_gpu_conv_geometry.py through ``_check`` of test_gpu_vae_kernels.py.  MNIST at B = 4, S = 2; AudioMNIST and whale
at d = 8 (the smallest width the kernels' channel rules take), B = 2, S = 2.  Cases are re-seeded until the fp64 forward
has no LeakyReLU input within fp32 noise of zero (``tie_free`` of test_gpu_modules.py).

Three steps against the fp64 loop compare the three loss values only -- parameters after Adam are sign-sensitive at
noise level -- with the CPU-fp32 loop's own deviation from fp64 times YARD as the margin."""
import copy

import pytest
import torch

import ali_oracle as orc
from test_gpu_conv_geometry import RTOL, YARD
from test_gpu_modules import tie_free, to_dev
from test_gpu_vae_kernels import _check
from test_vae_cpu import build

gpu = pytest.mark.gpu
FAMILIES = {"mnist": ("mnist_b4", 1e-4), "audio": ("audio_d8_b2", 1e-3), "whale": ("whale_d8_b2", 1e-3)}
S, KLW = 2, 10.0
_CASES = {}


def dbl(c):
    return {k: v.double() for k, v in c.items()}


def case(name, golden_dir):
    """(vae fp32 on the CPU, its fp64 copy, x, c, eps): fixture weights rescaled to O(1) activations, tie free"""
    if name not in _CASES:
        fx_name, std = FAMILIES[name]
        _, vae, x0, c, _, _ = build(fx_name, golden_dir)
        orc.rescale_for_test_(vae.encoder, std, bias_seed=7), orc.rescale_for_test_(vae.decoder, std, bias_seed=8)
        with torch.no_grad():                      # log_var head: small outputs, so that exp() of it stays O(1)
            vae.encoder.log_var_head.weight.mul_(0.25)
        ref64 = copy.deepcopy(vae).double()
        B = x0.shape[0]

        def make(v):
            g = torch.Generator().manual_seed(40 + v)
            return torch.rand(x0.shape, generator=g) * 2 - 1, torch.randn(S, B, 512, 1, 1, generator=g)
        # (the whale case has 1.5 M LeakyReLU inputs, about three ties per draw: one draw in twenty-five is tie free)
        x, eps = tie_free([ref64], make, lambda x, e: ref64.elbo(x.double(), dbl(c), S, kl_weight=KLW, eps=e.double()),
                          tries=200)
        _CASES[name] = (vae, ref64, x, c, eps)
    return _CASES[name]


def _elbo_and_grads(vae, x, c, eps):
    vae.zero_grad()
    e = vae.elbo(x, c, num_samples=S, kl_weight=KLW, eps=eps)
    (-e).backward()
    return e.detach(), {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p))
                        for k, p in vae.named_parameters()}


@gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_modules_and_autograd_elbo_vs_fp64(name, golden_dir):
    vae, ref64, x, c, eps = case(name, golden_dir)
    dev = copy.deepcopy(vae).cuda()
    xd, cd, ed = x.cuda(), to_dev(c), eps.cuda()
    with torch.no_grad():
        m64, v64 = ref64.encoder(x.double(), dbl(c))
        m32, v32 = vae.encoder(x, c)
        md, vd = dev.encoder(xd, cd)
        _check(f"{name} mean", md, m64, m32)
        _check(f"{name} log_var", vd, v64, v32)
        s64 = ref64.encoder.sample(x.double(), dbl(c), eps=eps[0].double())
        _check(f"{name} sample", dev.encoder.sample(xd, cd, 'cuda', eps=ed[0]), s64, vae.encoder.sample(x, c, eps=eps[0]))
        _check(f"{name} decoder", dev.decoder(s64.float().cuda(), cd), ref64.decoder(s64.float().double(), dbl(c)),
               vae.decoder(s64.float(), c))
        assert dev(xd, cd, num_samples=1).dim() == 0
    e64, g64 = _elbo_and_grads(ref64, x.double(), dbl(c), eps.double())
    e32, g32 = _elbo_and_grads(vae, x, c, eps)
    ed_, gd = _elbo_and_grads(dev, xd, cd, ed)
    _check(f"{name} elbo", ed_, e64, e32)
    for k in g64:
        _check(f"{name} {k}.grad", gd[k], g64[k], g32[k])


@gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_one_stepper_step_has_the_autograd_gradients(name, golden_dir):
    from ali_hip.vae import VaeStepper
    vae, ref64, x, c, eps = case(name, golden_dir)
    _, g64 = _elbo_and_grads(ref64, x.double(), dbl(c), eps.double())
    _, g32 = _elbo_and_grads(vae, x, c, eps)
    dev = copy.deepcopy(vae).cuda()
    stepper = VaeStepper(dev, lr=1e-4, kl_weight=KLW, num_samples=S)
    r = stepper.step(x.cuda(), to_dev(c), eps.cuda())
    assert set(r) == {"loss", "logp", "kl"} and all(v.dim() == 0 and v.is_cuda for v in r.values())
    for k, p in dev.named_parameters():
        _check(f"{name} stepper {k}.grad", stepper.opt.grad_views[id(p)], g64[k], g32[k])


def _loop(vae, x, c, eps_list, dtype):
    m = copy.deepcopy(vae).to(dtype)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    cc = {k: v.to(dtype) for k, v in c.items()}
    out = []
    for e in eps_list:
        opt.zero_grad()
        loss = -m.elbo(x.to(dtype), cc, num_samples=S, kl_weight=KLW, eps=e.to(dtype))
        loss.backward()
        opt.step()
        out.append(loss.item())
    return out


@gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_three_steps_vs_the_fp64_adam_loop(name, golden_dir):
    from ali_hip.vae import VaeStepper
    vae, _, x, c, eps = case(name, golden_dir)
    eps_list = [eps, eps.flip(0) * 0.5, -eps]
    l64, l32 = _loop(vae, x, c, eps_list, torch.float64), _loop(vae, x, c, eps_list, torch.float32)
    dev = copy.deepcopy(vae).cuda()
    stepper = VaeStepper(dev, lr=1e-4, kl_weight=KLW, num_samples=S)
    got = [stepper.step(x.cuda(), to_dev(c), e.cuda())["loss"].item() for e in eps_list]
    for i, (g, a, b) in enumerate(zip(got, l64, l32)):
        print(f"VAE {name} step {i} loss dev={g:.9e} fp64={a:.9e} e_dev={abs(g - a):.3e} e_cpu={abs(b - a):.3e}")
    for i, (g, a, b) in enumerate(zip(got, l64, l32)):
        assert abs(g - a) <= YARD * abs(b - a), (name, i, g, a, b)


@gpu
@pytest.mark.parametrize("name", ["mnist", "audio"])
def test_captured_and_eager_steps_agree_bit_for_bit(name, golden_dir):
    from ali_hip.vae import VaeStepper
    vae, _, x, c, eps = case(name, golden_dir)
    out = []
    for capture in (False, True):
        dev = copy.deepcopy(vae).cuda()
        stepper = VaeStepper(dev, lr=1e-4, kl_weight=KLW, num_samples=S, capture=capture, seed=9)
        res = []
        for xi, e in ((x, eps), (x * 0.5, -eps), (-x, None), (x, None)):      # given draws, then drawn in the kernel
            r = stepper.step(xi.cuda(), to_dev(c), None if e is None else e.cuda())
            res.append(torch.stack([r["loss"], r["logp"], r["kl"]]).clone())
        assert int(stepper.opt.step_t.item()) == 4 and int(stepper.draws.item()) == 2
        out.append((res, [p.detach().clone() for p in dev.parameters()]))
        if capture:
            assert len(stepper._graphs) == 2                                  # with and without given draws
            stepper.step(x[:1].cuda(), {k: v[:1].cuda() for k, v in c.items()}, eps[:, :1].cuda())
            assert len(stepper._graphs) == 3                                  # a second shape gets its own graph
            assert int(stepper.opt.step_t.item()) == 5
    (res_e, w_e), (res_c, w_c) = out
    for a, b in zip(res_e, res_c):
        assert torch.equal(a, b)
    for a, b in zip(w_e, w_c):
        assert torch.equal(a, b)
    assert not torch.equal(res_e[2], res_e[3])                                # the counter moved: new draws


@gpu
@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("with_cf", [False, True])
def test_reconstructor_vs_the_per_round_loop(rounds, with_cf, golden_dir):
    from ali_hip.vae import VaeReconstructor
    vae, ref64, x, c, _ = case("mnist", golden_dir)
    dev = copy.deepcopy(vae).cuda().eval()
    B = x.shape[0]
    e = torch.randn(rounds, B, 512, 1, 1, generator=torch.Generator().manual_seed(rounds))
    c_cf = dict(c, digit=c["digit"].roll(1, 0)) if with_cf else None
    xd, cd, cfd = x.cuda(), to_dev(c), None if c_cf is None else to_dev(c_cf)

    def loop(m, xx, cc, cf, ee):
        with torch.no_grad():
            rec = 0
            for r in range(rounds):
                rec = rec + m.decoder(m.encoder.sample(xx, cc, eps=ee[r]), cf if cf is not None else cc)
            return rec / rounds
    want64 = loop(ref64, x.double(), dbl(c), None if c_cf is None else dbl(c_cf), e.double())
    want32 = loop(vae, x, c, c_cf, e)
    module_path = loop(dev, xd, cd, cfd, e.cuda())
    for capture in (False, True):
        rec = VaeReconstructor(dev, rounds=rounds, capture=capture)
        got = rec.add(xd, cd, cfd, e.cuda())
        assert got.shape == (B, 1, 28, 28)
        _check(f"reconstructor rounds={rounds} cf={with_cf} capture={capture}", got, want64, want32)
        # the per-round loop on the module path: another fp32 evaluation on the device (other GEMM tiles: rows B, not
        # rounds * B), itself within the bounds of fp64 -- the two lie within RTOL of the image scale of each other
        diff = (got - module_path).abs().max().item()
        print(f"VAE reconstructor vs module-path loop rounds={rounds} cf={with_cf} capture={capture}: {diff:.3e}")
        assert diff <= RTOL * want64.abs().max().item()
        if capture:
            assert torch.equal(rec.add(xd, cd, cfd, e.cuda()), got)          # replayed
            a, b = rec.add(xd, cd, cfd).clone(), rec.add(xd, cd, cfd).clone()    # drawn in the kernel: new draws per call
            assert not torch.equal(a, b) and bool(torch.isfinite(a).all())
