"""Classifier family at the scoring scripts' own shapes (MNIST B=128, AudioMNIST B=128 with mc_rounds=4, whale B=64):
one training step (ClassifierStepper, HIP-graph replay) and one scoring batch (GeneratorScore: generator rounds, every
classifier, device counters, one graph) against what these callers run without the family -- the same layers as a stock
``nn.Sequential`` on ROCm PyTorch with ``CrossEntropyLoss`` + ``torch.optim.Adam``, and for scoring the script's loop
body (``GeneratorSampler`` image, stock classifiers, ``.argmax(1) == .argmax(1)).sum()`` and its host read per
classifier).  Every call is timed on its own with device events after a warm-up; prints median, min and max per
measurement and the ratio of the medians.  Needs a GPU.  ``--calls N`` (default 20), ``--only FAMILY``."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from ali_hip.classify import ClassifierStepper, GeneratorScore  # noqa: E402
from ali_hip.step import GeneratorSampler  # noqa: E402


def family(name):
    if name == "mnist":
        import image_scms.mnist as im
        from classifiers.mnist import MNISTClassifier
        attrs = {"digit": 10}
        cont = ("thickness", "intensity", "slant")
        return im.Generator(), {"digit": MNISTClassifier()}, attrs, cont, 28, 128, 1
    if name == "audio":
        import image_scms.audio_mnist as im
        from classifiers.audio_mnist import ATTRIBUTE_DIMS, AudioMNISTClassifier
        clfs = {k: AudioMNISTClassifier(ATTRIBUTE_DIMS[k]) for k in ("gender", "digit", "accent")}
        return im.Generator(), clfs, dict(ATTRIBUTE_DIMS), (), 128, 128, 4
    import image_scms.whalecalls as im
    from classifiers.whalecalls import NARWClassifier
    return im.Generator(), {"call_type": NARWClassifier()}, {"call_type": 3}, (), 256, 64, 1


def timed(fn, calls, warm=3, sync_each=False):
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


def report(name, what, new, old):
    print(f"{name}: {what}: HIP path median {new[0]:.3f} ms (min {new[1]:.3f}, max {new[2]:.3f}); stock torch median "
          f"{old[0]:.3f} ms (min {old[1]:.3f}, max {old[2]:.3f}); stock / HIP = {old[0] / new[0]:.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    for name in ("mnist", "audio", "whale"):
        if a.only and name != a.only:
            continue
        torch.manual_seed(0)
        G, clfs, attr_dims, cont, hw, B, R = family(name)
        G = G.cuda().eval()
        clfs = {k: m.cuda() for k, m in clfs.items()}
        stock = {k: nn.Sequential(*copy.deepcopy(list(m.children()))).cuda() for k, m in clfs.items()}
        attrs = {k: torch.eye(n)[torch.randint(0, n, (B,))].cuda() for k, n in attr_dims.items()}
        attrs.update({k: torch.rand(B, 1).cuda() * 2 - 1 for k in cont})

        # ---- one training step of the family's first classifier
        key = next(iter(clfs))
        x, y = torch.rand(B, 1, hw, hw).cuda() * 2 - 1, attrs[key]
        stepper = ClassifierStepper(copy.deepcopy(clfs[key]), lr=1e-4, capture=True)
        ref = copy.deepcopy(stock[key])
        opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
        crit = nn.CrossEntropyLoss()

        def stock_step():
            opt.zero_grad()
            pred = ref(x)
            loss = crit(pred, y)
            loss.backward()
            opt.step()
            return torch.eq(pred.argmax(dim=1), y.argmax(dim=1)).float().mean()
        report(name, f"training step B={B}", timed(lambda: stepper.step(x, y), a.calls), timed(stock_step, a.calls))
        del stepper, ref, opt

        # ---- one scoring batch: mc-round mean image, every classifier, the hit counts
        score = GeneratorScore(G, clfs, mc_rounds=R)
        sampler = GeneratorSampler(G)
        zs = torch.randn(R, B, 512, 1, 1).cuda()

        @torch.no_grad()
        def stock_score():
            gen = sampler(zs, attrs)
            return [(stock[k](gen).argmax(1) == attrs[k].argmax(1)).sum().cpu().item() for k in stock]
        report(name, f"scoring batch B={B} mc_rounds={R} classifiers={len(clfs)}",
               timed(lambda: score.add(attrs, zs), a.calls), timed(stock_score, a.calls))
        del score, sampler
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
