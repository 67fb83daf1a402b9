"""morphomnist perturbations at the measured-counterfactual scripts' shapes: the build time of the footprint table (all
radii up to ``--max-radius``, a one-off host cost), one ``MorphoPerturb.apply`` of B = 1000 images of 28 x 28 at scale 16
against the CPU statement ``morphomnist.perturb.counterfactual_image`` the scripts' loop would run (timed on
``--cpu-images`` images, reported per image: the loop is sequential), then the three new kernels of csrc/morpho.hip alone
on one chunk.  Every call is timed on its own with device events after a warm-up; prints median, min and max.  Needs a
GPU.  ``--calls N`` (default 5), ``--batch B`` (default 1000)."""
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
from ali_hip.morpho import MorphoPerturb, perturb_image_bytes  # noqa: E402
from morphomnist import perturb as stmt  # noqa: E402


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
    ap.add_argument("--cpu-images", type=int, default=6)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--max-radius", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    B, scale = a.batch, a.scale
    t0 = time.perf_counter()
    table = stmt.half_width_table(a.max_radius)
    print(f"footprint table, radii 0 .. {a.max_radius}: {time.perf_counter() - t0:.2f} s on the host, {table.nbytes} bytes",
          flush=True)
    pred = mc.generator_images(B, seed=0)
    x = torch.from_numpy(255 * (pred + 1) / 2).cuda()
    g = np.random.default_rng(0)
    targets = [g.uniform(lo, hi, size=B).astype(np.float32) for lo, hi in ((1.5, 4.5), (-0.4, 0.4), (80, 250))]
    t, s, i = (torch.from_numpy(v).cuda() for v in targets)
    mp = MorphoPerturb(scale=scale, max_radius=a.max_radius)
    n = min(mp.chunk_for(28, 28), B)
    print(f"--- scale {scale}: {perturb_image_bytes(28, 28, scale)} bytes per image, chunks of {n}", flush=True)
    t_hip = timed(lambda: mp.apply(x, t, s, i), a.calls)
    show(f"MorphoPerturb.apply B={B} scale={scale} (no host read)", t_hip, f"; {t_hip[0] / B * 1e3:.1f} us per image")
    out = mp.apply(x, t, s, i)
    print(f"status counts: {torch.bincount(out['status'], minlength=5).tolist()}; radius {int(out['radius'].min())} .. "
          f"{int(out['radius'].max())}", flush=True)
    host = x.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    for b in range(a.cpu_images):
        stmt.counterfactual_image(host[b], targets[0][b], targets[1][b], targets[2][b], scale, max_radius=a.max_radius)
    per = (time.perf_counter() - t0) / a.cpu_images * 1e3
    print(f"CPU statement (counterfactual_image, fp64): {per:.1f} ms per image over {a.cpu_images} images; the device's "
          f"{t_hip[0] / B:.4f} ms per image is {per / (t_hip[0] / B):.0f} x", flush=True)
    # the three new kernels alone, on one chunk's bitmaps and thickness
    xc, tc, sc, ic = x[:n], t[:n], (-torch.tan(s[:n].double())), i[:n]
    mm = mp.measure
    AH, AW = mm.operators(28, 28, x.device)
    RH, RW = mp.reduce_operators(28, 28, x.device)
    ws = mp._workspace(n, 28, 28, x.device)
    bits, fg, hstats = ops.morpho_binarise(xc, scale, AH, AW, 0.5, ws=ws)
    d2, st = ops.morpho_edt(bits, 28 * scale, ws=ws)
    skel = ops.morpho_thin(bits, d2, fg, st, mm._keep, 0, ws=ws)
    _, values, _ = ops.morpho_measure(xc, scale, skel, d2, fg, hstats, st)
    half = mp.half_table(x.device)
    shaped, _, sums, st2 = ops.morpho_reshape(bits, 28 * scale, values[:, 2], tc, st, half, scale, ws=ws)
    q, _ = ops.morpho_shear_reduce(shaped, 28, 28, scale, sums, sc, st2, RH, RW, ws=ws)
    show(f"ali_morpho_reshape        n={n}", timed(lambda: ops.morpho_reshape(bits, 28 * scale, values[:, 2], tc, st, half,
                                                                              scale, ws=ws), a.calls))
    show(f"ali_morpho_shear_reduce   n={n}", timed(lambda: ops.morpho_shear_reduce(shaped, 28, 28, scale, sums, sc, st2, RH,
                                                                                   RW, ws=ws), a.calls))
    show(f"ali_morpho_set_intensity  n={n}", timed(lambda: ops.morpho_set_intensity(q, ic, st2), a.calls))


if __name__ == "__main__":
    main()
