"""The bounding parallelogram of ``measure_image`` at B = 1000 images of 28 x 28, at scales 16 and 4:
``MorphoMeasure.measure`` with and without ``bound_frac`` (the extra launch per chunk and the columns formed from it),
``ali_morpho_bounds`` alone on one chunk next to ``ali_morpho_binarise`` on the same chunk (both form the up-sampled
image twice, so binarise is the comparison), and the host statement ``morphomnist.measure.measure_image`` per image
(timed on ``--cpu-images`` images).  Every call is timed on its own with device events after a warm-up; prints median,
min and max.  Needs a GPU.  ``--calls N`` (default 5), ``--batch B`` (default 1000), ``--scales`` (default 16 4)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import morpho_cases as mc  # noqa: E402
from ali_hip import ops  # noqa: E402
from ali_hip.morpho import MorphoMeasure  # noqa: E402
from morphomnist.measure import measure_image  # noqa: E402


def timed(fn, calls, warm=1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--scales", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--cpu-images", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    B = a.batch
    pred = mc.generator_images(B, seed=0)
    x = torch.from_numpy(pred).cuda()
    for s in a.scales:
        plain, bound = MorphoMeasure(scale=s), MorphoMeasure(scale=s, bound_frac=.02)
        n = min(bound.chunk_for(28, 28), B)
        print(f"--- B={B} scale {s}: chunks of {n} (without bound_frac: {min(plain.chunk_for(28, 28), B)})", flush=True)
        t_plain = show("MorphoMeasure.measure", timed(lambda: (plain.measure(x), plain.reset()), a.calls))
        t_bound = show("MorphoMeasure(bound_frac=.02).measure", timed(lambda: (bound.measure(x), bound.reset()), a.calls))
        print(f"    bounds add {t_bound - t_plain:.3f} ms ({t_bound / t_plain:.2f}x)", flush=True)
        xs = x[:n]
        AH, AW = bound.operators(28, 28, x.device)
        ws = bound._workspace(n, 28, 28, x.device)
        t_bin = show(f"ali_morpho_binarise B={n}", timed(lambda: ops.morpho_binarise(xs, s, AH, AW, .5, ws=ws), a.calls))
        t_bd = show(f"ali_morpho_bounds B={n}", timed(lambda: ops.morpho_bounds(xs, s, AH, AW, .02, ws=ws), a.calls))
        print(f"    bounds / binarise = {t_bd / t_bin:.2f}", flush=True)
        t0 = time.perf_counter()
        for im in (255 * (pred[:a.cpu_images] + 1) / 2).astype(np.float64):
            measure_image(im, scale=s, verbose=False)
        per = (time.perf_counter() - t0) / a.cpu_images * 1e3
        print(f"    the host measure_image: {per:.1f} ms per image, {per * B / 1e3:.1f} s for {B}; statement / HIP = "
              f"{per * B / t_bound:.0f}x", flush=True)


if __name__ == "__main__":
    main()
