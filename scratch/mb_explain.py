"""The explain family at the evaluation scripts' shapes: MNIST E / G / classifier, one
``HingeLossCFExplainer.explain(steps=30)`` and one ``DeepCounterfactualExplainer.explain(sample_points=100,
metric='mse')``, at B = 1 and at B = 64 through ``explain_batch``.

Three ways per call: the executors of ``ali_hip.explain`` replayed from HIP graphs, the same executors launched eagerly,
and the baseline -- the loop as the reference states it, over the same modules under autograd on the same GPU (what these
callers ran before the family existed: the drop-in classes fall back to exactly that statement for models they do not
recognise, which is how it is reached here).  The B = 64 baseline is 64 single calls; it is measured on ``--rows`` of
them (default 4) and scaled, and printed as such.

Every call is timed on its own with a host clock around work that ends in a device synchronise, after warm-up calls;
prints median, min and max.  Needs a GPU.  ``--calls N`` (default 10)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from explain.cf_example import DeepCounterfactualExplainer, HingeLossCFExplainer  # noqa: E402


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
    print(f"explain: {what}: median {r[0] * scale:.2f} ms (min {r[1] * scale:.2f}, max {r[2] * scale:.2f}){note}",
          flush=True)
    return r[0] * scale


def batch(B, device):
    g = torch.Generator().manual_seed(B)
    x = torch.tanh(torch.randn(B, 1, 28, 28, generator=g)).to(device)
    attrs = {"digit": torch.eye(10)[torch.randint(0, 10, (B,), generator=g)].to(device)}
    for k in ("thickness", "intensity", "slant"):
        attrs[k] = (torch.rand(B, 1, generator=g) * 2 - 1).to(device)
    return x, attrs, torch.randint(0, 10, (B,), generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    import image_scms.mnist as pm
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(0)
    E, G, clf = pm.Encoder().cuda().eval(), pm.Generator().cuda().eval(), MNISTClassifier().cuda().eval()
    kw = dict(categorical_features=["digit"], features_to_ignore=["slant"])
    hinge = HingeLossCFExplainer(E, G, clf, "digit", 512, **kw)
    hinge_ref = HingeLossCFExplainer(lambda *v: E(*v), lambda z, c: G(z, c), clf, "digit", 512, **kw)
    sweep = DeepCounterfactualExplainer(E, G, clf, "digit")
    sweep_ref = DeepCounterfactualExplainer(lambda *v: E(*v), lambda z, c: G(z, c), clf, "digit")
    x1, a1, t1 = batch(1, "cuda")
    xb, ab, tb = batch(64, "cuda")
    rows = [(xb[b:b + 1], {k: v[b:b + 1] for k, v in ab.items()}, int(tb[b])) for b in range(a.rows)]
    res = {}

    # ---- the hinge loop
    def h1(ex):
        return lambda: ex.explain(x1, a1, target_class=int(t1[0]), steps=a.steps)

    def hb():
        return hinge.explain_batch(xb, ab, tb.cuda(), steps=a.steps)

    def h_rows():
        for x, at, t in rows:
            hinge_ref.explain(x, at, target_class=t, steps=a.steps)
    for capture in (True, False):
        h1(hinge)()                                            # (builds the executor)
        hinge._stepper.capture = capture
        tag = "captured" if capture else "eager"
        res["h1", tag] = line(f"hinge steps={a.steps} B=1 executor {tag}", timed(h1(hinge), a.calls))
        res["h64", tag] = line(f"hinge steps={a.steps} B=64 explain_batch executor {tag}", timed(hb, a.calls))
    res["h1", "ref"] = line(f"hinge steps={a.steps} B=1 autograd statement", timed(h1(hinge_ref), a.calls))
    res["h64", "ref"] = line(f"hinge steps={a.steps} B=64 autograd statement", timed(h_rows, max(a.calls // 3, 3), 1),
                             64 / a.rows, f" [{a.rows} single calls scaled to 64]")

    # ---- the sweep
    def s1(ex):
        return lambda: ex.explain(x1, a1, int(t1[0]), sample_points=100, metric="mse")

    def sb():
        return sweep.explain_batch(xb, ab, tb.tolist(), sample_points=100, metric="mse")

    def s_rows():
        for x, at, t in rows:
            sweep_ref.explain(x, at, t, sample_points=100, metric="mse")
    for capture in (True, False):
        s1(sweep)()
        sweep._sweep.capture = capture
        tag = "captured" if capture else "eager"
        res["s1", tag] = line(f"sweep S=100 mse B=1 executor {tag}", timed(s1(sweep), a.calls))
        res["s64", tag] = line(f"sweep S=100 mse B=64 explain_batch executor {tag}", timed(sb, max(a.calls // 3, 3), 1))
    res["s1", "ref"] = line("sweep S=100 mse B=1 autograd statement", timed(s1(sweep_ref), a.calls))
    res["s64", "ref"] = line("sweep S=100 mse B=64 autograd statement", timed(s_rows, max(a.calls // 3, 3), 1),
                             64 / a.rows, f" [{a.rows} single calls scaled to 64]")
    for k in ("h1", "h64", "s1", "s64"):
        print(f"explain: {k}: statement / captured = {res[k, 'ref'] / res[k, 'captured']:.2f}x, "
              f"statement / eager = {res[k, 'ref'] / res[k, 'eager']:.2f}x", flush=True)


if __name__ == "__main__":
    main()
