"""What ``mnist.train(device="cuda", batch_size=512)`` sustains, input pipeline included, next to the bench line.

20 * 512 synthetic uint8 MorphoMNIST images; ``input_pipeline="host"`` (the default: per-iteration host scaling, host
z draw, uploads) and ``"device"`` alternate, ``--reps`` times each.  The first three iterations of a run (graph capture,
SURVEY 8d) are discarded: the clock starts, after a device synchronise, when the fourth iteration is issued and stops
when ``train`` returns (its last statement synchronises: ``d_score.item()``).  Per run:

  wall ms / iteration and img/s  over the timed iterations, epoch boundaries (permutation, score read-back) included;
  host ms / iteration            mean time between two consecutive iteration calls inside an epoch: what the loop's own
                                 host code costs, blocking pageable copies included, the final synchronise excluded.

Then the same tree's ``python bench.py --gpus 1`` (a child process) for ``ms_per_step``.
usage: python scratch/train_loop_time.py [--epochs 6] [--reps 3] [--no-bench]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "imagecfgen-pytorch_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402

BS, N_BATCHES, SKIP = 512, 20, 3


def timed_train(pipeline, x, a, epochs):
    import ali_hip
    import image_scms.mnist as pm
    from ali_hip.step import AliStepper
    marks = []                 # host clock at the start of every iteration call
    t_start = [None]

    def hooked(fn):
        def call(self, *args, **kw):
            if len(marks) == SKIP:
                torch.cuda.synchronize()
                t_start[0] = time.perf_counter()
            marks.append(time.perf_counter())
            return fn(self, *args, **kw)
        return call
    real = AliStepper.step, AliStepper.step_indexed
    AliStepper.step, AliStepper.step_indexed = hooked(real[0]), hooked(real[1])
    try:
        ali_hip.manual_seed(1)
        torch.manual_seed(1)
        np.random.seed(1)
        pm.train(x, a, n_epochs=epochs, device="cuda", save_images_every=None, batch_size=BS, input_pipeline=pipeline)
        torch.cuda.synchronize()
        t_end = time.perf_counter()
    finally:
        AliStepper.step, AliStepper.step_indexed = real
    n_timed = len(marks) - SKIP
    assert len(marks) == epochs * N_BATCHES and n_timed > 0
    wall = (t_end - t_start[0]) / n_timed
    gaps = [marks[i + 1] - marks[i] for i in range(SKIP, len(marks) - 1) if (i + 1) % N_BATCHES]
    return {"pipeline": pipeline, "iterations": n_timed, "wall_ms_per_iter": round(1e3 * wall, 3),
            "img_per_s": round(BS / wall, 1), "host_ms_per_iter": round(1e3 * sum(gaps) / len(gaps), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-bench", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_loop_time.py measures on the GPU; no GPU found")
    import ali_oracle as orc
    x, a = orc.synth_morphomnist(N_BATCHES * BS, seed=1)
    x = x.to(torch.uint8)
    runs = []
    for _ in range(args.reps):
        for pipeline in ("host", "device"):
            r = timed_train(pipeline, x, a, args.epochs)
            runs.append(r)
            print(json.dumps(r), flush=True)
    out = {}
    for pipeline in ("host", "device"):
        ms = sorted(r["wall_ms_per_iter"] for r in runs if r["pipeline"] == pipeline)
        host = sorted(r["host_ms_per_iter"] for r in runs if r["pipeline"] == pipeline)
        med = ms[len(ms) // 2]
        out[pipeline] = {"wall_ms_per_iter": med, "min": ms[0], "max": ms[-1], "img_per_s": round(1e3 * BS / med, 1),
                         "host_ms_per_iter": host[len(host) // 2]}
    if not args.no_bench:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup",
                              "10"], capture_output=True, text=True, cwd=ROOT, timeout=300)
        line = next((ln for ln in reversed(res.stdout.splitlines()) if ln.startswith("{")), None)
        if res.returncode or line is None:
            sys.exit(f"bench.py failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
        out["bench_ms_per_step"] = json.loads(line)["ms_per_step"]
    print(json.dumps({"train_loop_time": out}))


if __name__ == "__main__":
    main()
