"""The attribute_shap family at the evaluation script's setting: MNIST Generator / classifier, one
``ExpectedGradients.shap_values`` call at R = 1 and R = 64 explained rows, S = 200 samples, n_draws = 4, 200 background
rows.

Three ways per call: the executor replayed from HIP graphs, the same executor launched eagerly, and the baseline -- the
estimator as the script runs it through the ``shap`` package, written out in torch on the same GPU under autograd: per
explained row 200 interpolated samples in batches of 50 through the script's model body (repeat, one z per repeated
row, grouped mean) and one ``autograd.grad(outputs[:, c].sum(), X)`` per class.  The baseline runs the same weights on
torch's stock operators (``G.layers`` and the classifier's ``nn.Sequential`` called as such): the drop-in modules'
autograd node frees its saved state in its first backward pass, so ten backward passes over one forward, which is what
the script's loop does, cannot run on it.  The R = 64 baseline is 64 single rows; it is measured on ``--rows`` of
them (default 2) and scaled, and printed as such.

Then the three kernels of csrc/attrib.hip alone at the R = 64 shapes: the time per launch of a loop of back-to-back
launches between two device events, against the bytes the algorithm moves (computed here from the shapes).

Every call is timed on its own with a host clock around work that ends in a device synchronise, after warm-up calls;
prints median, min and max.  Needs a GPU.  ``--calls N`` (default 5)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from ali_hip import ops  # noqa: E402
from ali_hip.attrib import MNIST_SLICES, ExpectedGradients  # noqa: E402
from image_scms.mnist import continuous_feature_map  # noqa: E402

S, N_DRAWS, NB, BATCH = 200, 4, 200, 50


def timed(fn, calls, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def line(what, r, scale=1, note=""):
    print(f"attrib: {what}: median {r[0] * scale:.2f} ms (min {r[1] * scale:.2f}, max {r[2] * scale:.2f}){note}",
          flush=True)
    return r[0] * scale


def rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(n, 13)
    a[torch.arange(n), torch.randint(0, 10, (n,), generator=g)] = 1.0
    a[:, 10:] = torch.rand(n, 3, generator=g) * 2 - 1
    return a.cuda()


def stock_model(G, clf, n):
    """the script's model class body on torch's stock operators"""
    def forward(a):
        attrs = {k: a[:, :, o:o + w].repeat(n, 1, 1).reshape((-1, w)) for k, (o, w) in MNIST_SLICES.items()}
        z = torch.randn((a.shape[0] * n, 512, 1, 1)).to(a.device)
        digit = attrs["digit"].matmul(G.digit_embedding.weight).reshape((-1, 256, 1, 1))
        planes = [continuous_feature_map(attrs[k], size=(1, 1)) for k in sorted(attrs) if k != "digit"]
        img = G.layers(torch.concat([z, digit] + planes, dim=1))
        return torch.nn.Sequential.forward(clf, img).softmax(1).reshape((-1, n, 10)).mean(dim=1)
    return forward


def script_row(model, x, bg):
    """one explained row the way the script's explainer computes it: batches of 50 samples, one backward per class"""
    idx = torch.randint(0, bg.shape[0], (S,), device="cuda")
    t = torch.rand(S, 1, device="cuda")
    b = bg[idx]
    samples, delta = t * x + (1 - t) * b, x - b
    grads = [[] for _ in range(10)]
    for lo in range(0, S, BATCH):
        X = samples[lo:lo + BATCH].reshape(-1, 1, 13).clone().requires_grad_(True)
        out = model(X)
        for c in range(10):
            g, = torch.autograd.grad(out[:, c].sum(), X, retain_graph=c < 9)
            grads[c].append(g.reshape(-1, 13))
    return torch.stack([(delta * torch.cat(g)).mean(dim=0) for g in grads])


def kernel_time(fn, loops=50):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(loops):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / loops * 1e3          # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    import image_scms.mnist as pm
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(0)
    G, clf = pm.Generator().cuda().eval(), MNISTClassifier().cuda().eval()
    bg = rows(NB, 1)
    x1, x64 = rows(1, 2), rows(64, 3)
    model = stock_model(G, clf, N_DRAWS)
    res = {}
    for capture in (True, False):
        ex = ExpectedGradients(G, clf, bg, n_draws=N_DRAWS, nsamples=S, capture=capture)
        tag = "captured" if capture else "eager"
        res[1, tag] = line(f"shap_values R=1 S={S} n_draws={N_DRAWS} executor {tag}",
                           timed(lambda: ex.shap_values(x1), a.calls))
        res[64, tag] = line(f"shap_values R=64 S={S} n_draws={N_DRAWS} executor {tag} "
                            f"(rows_per_launch {ex.default_rows_per_launch(ex._device_layout(bg.device))})",
                            timed(lambda: ex.shap_values(x64), max(a.calls // 2, 2), 1))
    res[1, "ref"] = line("R=1 script's loop (batches of 50, backward per class), stock torch operators under autograd",
                         timed(lambda: script_row(model, x1, bg), a.calls))

    def some_rows():
        for r in range(a.rows):
            script_row(model, x64[r:r + 1], bg)
    res[64, "ref"] = line("R=64 script's loop, stock torch operators under autograd",
                          timed(some_rows, max(a.calls // 2, 2), 1), 64 / a.rows, f" [{a.rows} single rows scaled to 64]")
    for R in (1, 64):
        print(f"attrib: R={R}: script's loop / captured = {res[R, 'ref'] / res[R, 'captured']:.2f}x, "
              f"script's loop / eager = {res[R, 'ref'] / res[R, 'eager']:.2f}x", flush=True)

    # ---- the kernels alone, R = 64
    ex = ExpectedGradients(G, clf, bg, n_draws=N_DRAWS, nsamples=S, capture=False)
    lay = ex._device_layout(bg.device)
    R, N, A, ld = 64, 64 * S * N_DRAWS, 13, lay.ld
    idx = torch.randint(0, NB, (R, S), device="cuda", dtype=torch.int32)
    t, z = torch.rand(R, S, device="cuda"), torch.randn(R, S, N_DRAWS, 512, device="cuda")
    inp, delta, _, _ = ops.eg_input(lay, 512, x64, bg, S, N_DRAWS, idx, t, z)
    logits, g_rows = torch.randn(N, 10, device="cuda"), torch.randn(N, ld, device="cuda")
    glogit, phi = torch.empty(N, 10, device="cuda"), torch.zeros(R, 10, A, device="cuda")
    cases = [
        ("ali_eg_input given z", lambda: ops.eg_input(lay, 512, x64, bg, S, N_DRAWS, idx, t, z),
         4 * (N * ld + N * 512 + R * S * (3 * A + 2))),                       # rows written, z read, x / bg / delta, idx, t
        ("ali_eg_input drawn", lambda: ops.eg_input(lay, 512, x64, bg, S, N_DRAWS), 4 * (N * ld + R * S * 3 * A)),
        ("ali_eg_seed", lambda: ops.eg_seed(logits, 3, 1.0 / (S * N_DRAWS), glogit=glogit), 4 * 2 * N * 10),
        ("ali_eg_reduce", lambda: ops.eg_reduce(lay, g_rows, delta, N_DRAWS, phi, 3),
         4 * (N * (256 + 3) + R * S * A + R * A)),                             # the rows' attribute columns, delta, phi
    ]
    for name, fn, nbytes in cases:
        us = kernel_time(fn)
        print(f"attrib: {name} R=64: {us:.1f} us per launch (loop of 50 between device events), "
              f"{nbytes / 1e6:.1f} MB algorithmic -> {nbytes / us / 1e6:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
