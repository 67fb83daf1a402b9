"""The Morpho-MNIST local perturbations at the data-set builders' shape: ``MorphoLocal.apply`` of B = 512 images of 28 x 28
at scale 16 for each kind (and a mixed ``kind`` tensor), against ``MorphoPerturb.apply`` on the same batch (the existing
seven-launch pipeline: the yardstick), ``MorphoMeasure.measure`` (the four launches both begin with) and the host
statement ``morphomnist.perturb.local_image`` (timed on ``--cpu-images`` images, reported per image), then the new
launches alone on one chunk.  Every call is timed on its own with device events after a warm-up; prints median, min and
max.  Needs a GPU.  ``--calls N`` (default 5), ``--batch B`` (default 512)."""
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
from ali_hip.morpho import KINDS, MorphoLocal, MorphoMeasure, MorphoPerturb, local_image_bytes  # noqa: E402
from morphomnist import perturb  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--cpu-images", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    B, s = a.batch, a.scale
    pred = mc.generator_images(B, seed=0)
    x = torch.from_numpy(pred).cuda()
    ml, mp, mm = MorphoLocal(scale=s), MorphoPerturb(scale=s, max_radius=24), MorphoMeasure(scale=s)
    n = min(ml.chunk_for(28, 28), B)
    print(f"--- B={B} scale {s}: {local_image_bytes(28, 28, s)} bytes per image, chunks of {n}", flush=True)
    t_measure = show("MorphoMeasure.measure (the four launches both begin with)",
                     timed(lambda: (mm.measure(x), mm.reset()), a.calls))
    g = np.random.default_rng(0)
    targets = tuple(torch.from_numpy(g.uniform(lo, hi, size=B).astype(np.float32)).cuda()
                    for lo, hi in ((1.5, 4.5), (-0.4, 0.4), (80, 250)))
    t_perturb = show("MorphoPerturb.apply (seven launches: the yardstick)", timed(lambda: mp.apply(x, *targets), a.calls))
    mixed = (torch.arange(B, device="cuda") % 5).to(torch.int32)
    for kind in KINDS + (mixed,):
        name = kind if isinstance(kind, str) else "mixed"
        t = show(f"MorphoLocal.apply {name}", timed(lambda: ml.apply(x, kind), a.calls))
        out = ml.apply(x, kind)
        print(f"    after the four measurement launches {t - t_measure:.3f} ms; MorphoLocal / MorphoPerturb = "
              f"{t / t_perturb:.2f}; status 0 rows {int((out['status'] == 0).sum())} of {B}", flush=True)
        if isinstance(kind, str):
            t0 = time.perf_counter()
            for im in pred[:a.cpu_images].astype(np.float64):
                perturb.local_image(im, kind, s)
            per = (time.perf_counter() - t0) / a.cpu_images * 1e3
            print(f"    the host statement: {per:.1f} ms per image, {per * B / 1e3:.1f} s for {B}; statement / HIP = "
                  f"{per * B / t:.0f}x", flush=True)
    # the new launches alone, on one chunk
    xs = x[:n]
    AH, AW = mm.operators(28, 28, x.device)
    RH, RW = ml.reduce_operators(28, 28, x.device)
    ws = ml._workspace(n, 28, 28, x.device)
    Wh = 28 * s
    bits, fg, hstats = ops.morpho_binarise(xs, s, AH, AW, 0.5, ws=ws)
    d2, st = ops.morpho_edt(bits, Wh, ws=ws)
    skel = ops.morpho_thin(bits, d2, fg, st, mm._keep, 0, ws=ws)
    _, values, _ = ops.morpho_measure(xs, s, skel, d2, fg, hstats, st)
    show(f"complement + ali_morpho_edt of it B={n}",
         timed(lambda: ops.morpho_edt(ops.morpho_complement(bits, Wh), Wh, ws=ws), a.calls))
    d2c = ops.morpho_edt(ops.morpho_complement(bits, Wh), Wh, ws=ws)[0]
    for k, name in enumerate(KINDS):
        kd = torch.full((n,), k, dtype=torch.int32, device="cuda")
        loc = lambda: ops.morpho_locate(skel, d2, st, kd, s, ml.prune, ml.prune, 3)
        show(f"ali_morpho_locate {name} B={n}", timed(loc, a.calls))
        n_cand, _, ce, en = loc()
        run = lambda: ops.morpho_local(bits, Wh, d2, d2c, values[:, 2], st, kd, n_cand, ce, en, s, frac_radius=ml.frac_radius)
        show(f"ali_morpho_local {name} B={n}", timed(run, a.calls))
        new, _, sums, st2 = run()
        show(f"ali_morpho_shear_reduce (no target) {name} B={n}",
             timed(lambda: ops.morpho_shear_reduce(new, 28, 28, s, sums, None, st2, RH, RW, ws=ws), a.calls))


if __name__ == "__main__":
    main()
