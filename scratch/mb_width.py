"""``SetWidth`` at B = 1000 strokes of 28 x 28, at scales 16 and 4: ``MorphoPerturb.set_width`` end to end (plain, with
``intensity``, with ``validate``), then on one chunk ``ali_morpho_width`` next to ``ali_morpho_bounds`` (both form the
up-sampled rows and their prefixes; bounds has a pass more and the vertical cdf) and ``ali_morpho_affine_reduce`` next to
``ali_morpho_shear_reduce`` (the same reduce behind another warp), and the host statement
``morphomnist.perturb.width_image`` per image (timed on ``--cpu-images`` images).  Every call is timed on its own with
device events after a warm-up; prints median, min and max.  Needs a GPU.  ``--calls N`` (default 5), ``--batch B``
(default 1000), ``--scales`` (default 16 4)."""
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
from ali_hip.morpho import MorphoPerturb  # noqa: E402
from morphomnist.perturb import width_image  # noqa: E402


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
    g = np.random.default_rng(7)
    width = torch.from_numpy(g.uniform(4.0, 14.0, size=B)).cuda()                       # float64 target widths
    inten = torch.from_numpy(g.uniform(80, 250, size=B).astype(np.float32)).cuda()
    for s in a.scales:
        mp = MorphoPerturb(scale=s)
        n = min(mp.width_chunk_for(28, 28), B)
        print(f"--- B={B} scale {s}: chunks of {n}", flush=True)
        t_plain = show("MorphoPerturb.set_width", timed(lambda: mp.set_width(x, width), a.calls))
        show("MorphoPerturb.set_width(intensity)", timed(lambda: mp.set_width(x, width, inten), a.calls))
        out = mp.set_width(x, width, validate=True)
        show("MorphoPerturb.set_width(validate=True)", timed(lambda: mp.set_width(x, width, validate=True), a.calls),
             f"; status 0 on {int((out['status'] == 0).sum())}, off target {int(out['off_target'].sum())} of {B}")
        xs, ws_ = x[:n], width[:n].contiguous()
        AH, AW = mp.measure.operators(28, 28, x.device)
        RH, RW = mp.reduce_operators(28, 28, x.device)
        ws = mp._width_workspace(n, 28, 28, x.device)
        bits, fg, _ = ops.morpho_binarise(xs, s, AH, AW, .5, ws=ws)
        show(f"ali_morpho_binarise B={n}", timed(lambda: ops.morpho_binarise(xs, s, AH, AW, .5, ws=ws), a.calls))
        t_w = show(f"ali_morpho_width B={n}", timed(lambda: ops.morpho_width(xs, s, bits, fg, ws_, AH, AW, .02, ws=ws),
                                                     a.calls))
        t_b = show(f"ali_morpho_bounds B={n}", timed(lambda: ops.morpho_bounds(xs, s, AH, AW, .02, ws=ws), a.calls))
        print(f"    width / bounds = {t_w / t_b:.2f}", flush=True)
        sums, wb, st = ops.morpho_width(xs, s, bits, fg, ws_, AH, AW, .02, ws=ws)
        t_a = show(f"ali_morpho_affine_reduce B={n}",
                   timed(lambda: ops.morpho_affine_reduce(bits, 28, 28, s, sums, wb, st, RH, RW, ws=ws), a.calls))
        shear_t = torch.zeros(n, dtype=torch.float64, device=x.device)                  # (rows with a status: zeros in both)
        t_s = show(f"ali_morpho_shear_reduce B={n}",
                   timed(lambda: ops.morpho_shear_reduce(bits, 28, 28, s, sums, shear_t, st, RH, RW, ws=ws), a.calls))
        print(f"    affine_reduce / shear_reduce = {t_a / t_s:.2f}", flush=True)
        t0 = time.perf_counter()
        for b, im in enumerate((255 * (pred[:a.cpu_images] + 1) / 2).astype(np.float64)):
            width_image(im, float(width[b]), scale=s)
        per = (time.perf_counter() - t0) / a.cpu_images * 1e3
        print(f"    the host width_image: {per:.1f} ms per image, {per * B / 1e3:.1f} s for {B}; statement / HIP = "
              f"{per * B / t_plain:.0f}x", flush=True)


if __name__ == "__main__":
    main()
