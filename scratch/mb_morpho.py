"""morphomnist family at the measured-counterfactual scripts' shapes: one ``MorphoMeasure.measure`` of B = 1000 images of
28 x 28 at scale 16 (what the scripts use) and at scale 4, against the CPU statement ``morphomnist.morpho`` the scripts'
``extract_observed_attributes`` loop would run (timed on ``--cpu-images`` images, reported per image: the loop is
sequential), then the four kernels of csrc/morpho.hip alone on one chunk.  Every call is timed on its own with device
events after a warm-up; prints median, min and max, and the largest number of foreground pixels of an image (the cap of
the thinning rounds).  Needs a GPU.  ``--calls N`` (default 5), ``--batch B`` (default 1000)."""
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
from ali_hip.morpho import MorphoMeasure, per_image_bytes, statement_row  # noqa: E402
from morphomnist import morpho as stmt  # noqa: E402


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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    B = a.batch
    pred = mc.generator_images(B, seed=0)
    x = torch.from_numpy(255 * (pred + 1) / 2).cuda()
    for scale in (16, 4):
        mm = MorphoMeasure(scale=scale)
        n = min(mm.chunk_for(28, 28), B)
        print(f"--- scale {scale}: {per_image_bytes(28, 28, scale)} bytes per image, chunks of {n}", flush=True)
        t_hip = timed(lambda: (mm.measure(x), mm.reset()), a.calls)
        show(f"MorphoMeasure.measure B={B} scale={scale} (no host read)", t_hip, f"; {t_hip[0] / B * 1e3:.1f} us per image")
        t0 = time.perf_counter()
        for im in x[:a.cpu_images].cpu().numpy().astype(np.float64):
            statement_row(im, scale)
        per = (time.perf_counter() - t0) / a.cpu_images * 1e3
        print(f"the CPU statement (numpy / scipy, the sequential thinning loop in Python): {per:.1f} ms per image, "
              f"{per * B / 1e3:.1f} s for {B}; statement / HIP = {per * B / t_hip[0]:.0f}x", flush=True)
        # the four kernels alone, on one chunk
        xs = x[:n]
        AH, AW = mm.operators(28, 28, x.device)
        ws = mm._workspace(n, 28, 28, x.device)
        keep = stmt.keep_bits()
        show(f"ali_morpho_binarise B={n}", timed(lambda: ops.morpho_binarise(xs, scale, AH, AW, 0.5, ws=ws), a.calls))
        bits, fg, hstats = ops.morpho_binarise(xs, scale, AH, AW, 0.5, ws=ws)
        show(f"ali_morpho_edt B={n}", timed(lambda: ops.morpho_edt(bits, 28 * scale, ws=ws), a.calls))
        d2, status = ops.morpho_edt(bits, 28 * scale, ws=ws)
        show(f"ali_morpho_thin B={n}", timed(lambda: ops.morpho_thin(bits, d2, fg, status, keep, 0, ws=ws), a.calls),
             f"; largest foreground {int(fg.max())} pixels")
        skel = ops.morpho_thin(bits, d2, fg, status, keep, 0, ws=ws)
        show(f"ali_morpho_measure B={n}", timed(lambda: ops.morpho_measure(xs, scale, skel, d2, fg, hstats, status),
                                               a.calls))
        assert int(status.max()) == 0


if __name__ == "__main__":
    main()
