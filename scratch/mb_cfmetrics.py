"""cf_metrics family at the scripts' shapes: one ``AeStepper.step`` at B = 64 (capacity 64, latent 100; eager and
HIP-graph replay) and one ``CfMetrics.add`` at B = 64 with 11 autoencoders (capacity 64, latent 10) and 10 oracles,
each against the torch statement the scripts run without the family on the same GPU: the same layers as stock ``nn``
modules under autograd with ``torch.optim.Adam``, and for the metrics the scripts' per-row loop -- one row at a time,
two autoencoder passes per ``ae_rec`` / ``all_rec`` cell, twenty-one classifier calls and an ``.item()`` per cell --
with every module kept resident (no ``torch.load``).  Then the three kernels of csrc/cfmetrics.hip alone, with the bytes
each must move and the rate that gives.  Every call is timed on its own with device events after a warm-up; prints
median, min and max.  Needs a GPU.  ``--calls N`` (default 20), ``--rows N`` rows of the per-row loop (default 64)."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import train_morphomnist_ae as ae  # noqa: E402
from ali_hip import ops  # noqa: E402
from ali_hip.cfmetrics import AeStepper, CfMetrics, js_div  # noqa: E402
from classifiers.mnist import MNISTClassifier  # noqa: E402


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def show(what, t, extra=""):
    print(f"{what}: median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f}){extra}", flush=True)
    return t[0]


def stock(m):
    """the same layers as stock torch modules (never the HIP path)"""
    return copy.deepcopy(m.chain_view() if hasattr(m, "chain_view") else nn.Sequential(*list(m.children()))).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rows", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    torch.manual_seed(0)
    B = 64
    x = (torch.rand(B, 1, 28, 28) * 2 - 1).cuda()

    # ---- one training step (train_morphomnist_ae.py defaults: capacity 64, latent 100, B = 64)
    E, G = ae.Encoder(latent_dim=100), ae.Decoder(latent_dim=100)
    Es, Gs = stock(E), stock(G)
    opt = torch.optim.Adam(list(Es.parameters()) + list(Gs.parameters()), lr=1e-4, betas=(0.5, 0.9))

    def stock_step():
        opt.zero_grad()
        loss = (x - Gs(Es(x))).square().mean()
        loss.backward()
        opt.step()
        return loss
    t_stock = show("AeStepper B=64: stock torch step", timed(stock_step, a.calls))
    for capture in (False, True):
        st = AeStepper(copy.deepcopy(E).cuda(), copy.deepcopy(G).cuda(), capture=capture)
        t = timed(lambda: st.step(x), a.calls)
        show(f"AeStepper B=64: HIP path {'graph replay' if capture else 'eager'}", t, f"; stock / HIP = {t_stock / t[0]:.2f}x")

    # ---- one metrics batch: 11 autoencoders, 10 oracles, B = 64
    clf = MNISTClassifier().cuda()
    aes = {k: (ae.Encoder().cuda(), ae.Decoder().cuda()) for k in list(range(10)) + ["all"]}
    oracles = [MNISTClassifier().cuda() for _ in range(10)]
    cf = (torch.rand(B, 1, 28, 28) * 2 - 1).cuda()
    orig = torch.randint(0, 10, (B,)).cuda()
    m = CfMetrics(clf, aes, oracles)
    t_add = timed(lambda: m.add(x, cf, orig), a.calls)
    m.reset()
    s_clf, s_or = stock(clf), [stock(o) for o in oracles]
    s_aes = {k: (stock(e), stock(g)) for k, (e, g) in aes.items()}
    digits = orig.tolist()

    @torch.no_grad()
    def script_rows():
        rows = []
        for i in range(a.rows):
            c, xi, d = cf[i:i + 1], x[i:i + 1], digits[i]
            rec = lambda k: s_aes[k][1](s_aes[k][0](c))      # noqa: E731  (ae_rec / all_rec: a pass per cell)
            label = s_clf(c).argmax(1).item()
            row = [label, c.abs().sum().item(), (c - rec(d)).square().sum().cpu().item(),
                   (c - rec(label)).square().sum().cpu().item(),
                   (rec(label) - rec("all")).square().sum().cpu().item()]
            dists = [o(xi) for o in s_or]
            labels = [o(c).argmax(1).item() for o in s_or]
            for j, o in enumerate(s_or):
                row += [int(label == labels[j]), js_div(dists[j], o(c)).cpu().item()]
            rows.append(row)
        return rows
    t_rows = timed(script_rows, max(3, a.calls // 4), warm=1)
    per_row = t_rows[0] / a.rows
    show("CfMetrics.add B=64, 11 autoencoders, 10 oracles: HIP path (graph replay)", t_add)
    show(f"the scripts' per-row loop, {a.rows} rows, modules resident", t_rows,
         f"; {per_row:.3f} ms per row; loop for 64 rows / add = {per_row * 64 / t_add[0]:.1f}x")

    # ---- the kernels alone
    n = B * 784
    y = torch.tanh(torch.randn(n)).cuda()
    xf = x.reshape(-1)
    t = timed(lambda: ops.mse(y, xf, tanh_out=True), a.calls)
    show(f"ali_mse n={n} (loss + gradient)", t, f"; {3 * 4 * n} bytes -> {3 * 4 * n / t[0] / 1e6:.1f} GB/s")
    recon = torch.rand(11, B, 784).cuda()
    o32, t32 = orig.to(torch.int32), torch.randint(0, 10, (B,), dtype=torch.int32).cuda()
    t = timed(lambda: ops.cf_recon(cf.reshape(B, 784), recon, o32, t32), a.calls)
    nb = 4 * 4 * B * 784 + 16 * B
    show(f"ali_cf_recon B={B} N=784 A=11", t, f"; {nb} bytes -> {nb / t[0] / 1e6:.1f} GB/s")
    ox, ocf = torch.randn(10, B, 10).cuda(), torch.randn(10, B, 10).cuda()
    t = timed(lambda: ops.oracle_scores(t32, ox, ocf), a.calls)
    nb = 2 * 4 * 10 * B * 10 + 2 * 4 * B * 10 + 4 * B
    show(f"ali_oracle_scores B={B} J=10 C=10", t, f"; {nb} bytes -> {nb / t[0] / 1e6:.1f} GB/s")


if __name__ == "__main__":
    main()
