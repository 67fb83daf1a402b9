"""Shared by tests/test_attribute_scms_audio_cpu.py, tests/test_gpu_cat_kernels.py and
tests/test_gpu_audio_attribute_scm.py: AudioMNIST-like one-hot tables, graphs whose weights are shared between the CPU
statement (fp64: the reference, fp32: the yardstick) and the device, a graph that reaches the branches of csrc/cat.hip,
and the yardstick comparison of DESIGN.md 3.23.

The yardstick, per tensor: max|kernel - fp64| <= MULT * max|fp32 statement - fp64| + FLOOR_ULPS ulp32(max|fp64|).  The
kernels evaluate in fp64 and round once, so their error is about half an ulp of an entry; MULT leaves room for another
summation order, not for a wrong formula."""
import torch

MULT = 4.0
FLOOR_ULPS = 4.0
EPS32 = 2.0 ** -23
TRIO = ("country_of_origin", "native_speaker", "accent")
SIZES = {"small": (5, 2, 6), "wide": (13, 2, 17)}     # (Cc, Cn, Ca): the existing test's; across a k-step and a lane group
CORNER = (5, 2, 1)                                    # a one-class accent: lp exactly 0, nothing to draw
RATIOS = {}                                           # name -> (kernel error, fp32 statement's error), for the report


def within_yardstick(name, got, ref64, f32):
    got, ref64, f32 = (x.detach().double().cpu().reshape(-1) for x in (got, ref64, f32))
    assert got.shape == ref64.shape == f32.shape, (name, got.shape, ref64.shape, f32.shape)
    assert torch.isfinite(got).all() and torch.isfinite(ref64).all(), name
    if not got.numel():
        return 0.0
    err, yard, top = float((got - ref64).abs().max()), float((f32 - ref64).abs().max()), float(ref64.abs().max())
    ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    RATIOS[name] = (err, yard)
    print(f"yardstick {name}: kernel error {err:.3g}, fp32 statement's {yard:.3g}, ratio {ratio:.3g}, "
          f"max|fp64| {top:.3g}")
    assert err <= MULT * yard + FLOOR_ULPS * EPS32 * top, (name, err, yard, top)
    return ratio


def onehot_ds(sizes, n, seed=0):
    """{attribute: one-hot rows [n, classes]} (CPU fp32); accent depends on its parents so that training can learn"""
    g = torch.Generator().manual_seed(seed)
    Cc, Cn, Ca = sizes
    country = torch.randint(0, Cc, (n,), generator=g)
    native = (country + torch.randint(0, 2, (n,), generator=g)) % Cn
    accent = (country + native + (torch.rand(n, generator=g) < 0.2).long()) % Ca
    lab = {"country_of_origin": country, "native_speaker": native, "accent": accent,
           "digit": torch.randint(0, 10, (n,), generator=g), "age": torch.randint(0, 5, (n,), generator=g),
           "gender": torch.randint(0, 2, (n,), generator=g)}
    width = {"country_of_origin": Cc, "native_speaker": Cn, "accent": Ca, "digit": 10, "age": 5, "gender": 2}
    ds = {k: torch.eye(width[k])[v] for k, v in lab.items()}
    for k, w in width.items():                          # every class seen (n >= 17): the roots' widths are exact
        ds[k][:w] = torch.eye(w)
    return ds


def linears(graph):
    """every Linear of the two mechanisms: native_speaker's 4, the towers' 4 + 4 (unregistered), downstream's 2"""
    ns, combo = graph.get_module("native_speaker").model, graph.get_module("accent").model
    nets = [ns, combo.models[0], combo.models[1], combo.downstream]
    return [m for net in nets for m in net if isinstance(m, torch.nn.Linear)]


def trained_params(graph):
    """the twelve trained tensors in theta's order"""
    ns, combo = graph.get_module("native_speaker").model, graph.get_module("accent").model
    return [p for net in (ns, combo.downstream) for m in net if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]


def copy_weights(src, dst):
    with torch.no_grad():
        for a, b in zip(linears(src), linears(dst)):
            b.weight.data.copy_(a.weight.data)
            b.bias.data.copy_(a.bias.data)
    return dst


def new_graph(sizes, seed=0, device="cpu", n=64):
    import attribute_scms.audio_mnist as aa
    torch.manual_seed(seed)
    return aa.AudioMNISTCausalGraph(onehot_ds(sizes, max(n, 64), seed), device=device)


def twin(graph, sizes, dtype=torch.float64, device="cpu", seed=0):
    """a graph on ``device`` in ``dtype`` with ``graph``'s weights (the statement when on the CPU)"""
    t = new_graph(sizes, seed, device)
    if dtype != torch.float32:
        ns, combo = t.get_module("native_speaker").model, t.get_module("accent").model
        for net in (ns, combo.models[0], combo.models[1], combo.downstream):
            net.to(dtype)
    return copy_weights(graph, t)


def branchy_graph(sizes, seed=7):
    """A CPU graph whose weights reach the branches: hidden unit 0 of every ReLU layer dead for every row (zero weights,
    bias -100); native_speaker's second layer all zero (pre-activations exactly 0: the gate is closed, torch's ReLU
    gradient at 0 is 0); last layers scaled up so that classes are well separated; accent's classes 0 and 1 exactly
    tied (equal weight rows and biases), so the first index wins wherever they are the top."""
    g = new_graph(sizes, seed)
    gen = torch.Generator().manual_seed(seed)
    ns, combo = g.get_module("native_speaker").model, g.get_module("accent").model
    with torch.no_grad():
        for net in (ns, combo.models[0], combo.models[1], combo.downstream):
            lins = [m for m in net if isinstance(m, torch.nn.Linear)]
            for m in lins:
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (2.0 / m.in_features) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.3)
            for m in lins[:-1]:
                m.weight[0].zero_()
                m.bias[0] = -100.0
        ns[2].weight.zero_()
        ns[2].bias.zero_()
        ns[6].weight.mul_(6.0)
        ns[6].bias.copy_(torch.linspace(-2.0, 2.0, ns[6].bias.numel()) if ns[6].bias.numel() > 1 else ns[6].bias)
        last = combo.downstream[2]
        last.weight.mul_(6.0)
        if last.out_features > 1:
            last.weight[1].copy_(last.weight[0])
            last.bias[1] = last.bias[0]
    return g


def contexts(sizes, n, kind, seed=3):
    """(country, native, accent) fp32 CPU rows [n, C]: "onehot"; "dense" (random rows; rows 0 and 1 carry exactly tied
    maxima, so the first index is the class); "strided" (one-hot columns of one wider table)"""
    g = torch.Generator().manual_seed(seed + n)
    if kind == "dense":
        out = [torch.rand(n, c, generator=g) for c in sizes]
        for t in out:
            if t.shape[1] > 1:
                t[0, :2] = 2.0
                if n > 1:
                    t[1, -2:] = 3.0
        return out
    rows = [torch.eye(c)[torch.randint(0, c, (n,), generator=g)] for c in sizes]
    if kind == "onehot":
        return rows
    table = torch.zeros(n, sum(sizes) + 5)
    views, off = [], 2
    for r in rows:
        table[:, off:off + r.shape[1]] = r
        views.append(table[:, off:off + r.shape[1]])
        off += r.shape[1] + 1
    return views


def statement_nll(graph, ctx, wgt, dtype):
    """the statement in ``graph``'s dtype on the CPU: (lp [N, 2], the twelve gradients of sum(wgt * lp))"""
    obs = {k: v.to(dtype) for k, v in zip(TRIO, ctx)}
    lp = graph.log_prob(obs)
    lp = torch.stack([lp["native_speaker"], lp["accent"]], dim=1)
    grads = torch.autograd.grad((lp * wgt.to(dtype)).sum(), trained_params(graph), allow_unused=True)
    return lp.detach(), [torch.zeros_like(p) if x is None else x for x, p in zip(grads, trained_params(graph))]


def statement_logits(graph, country, native, dtype):
    """(native_speaker's, accent's) logits of the statement for dense parent rows"""
    ns, ac = graph.get_module("native_speaker").model, graph.get_module("accent").model
    with torch.no_grad():
        return ns(country.to(dtype)), ac(country.to(dtype), native.to(dtype))
