"""Griffin-Lim per family setting at the GeneratorSampler batch: one call (HIP-graph replay, device events, warm-up)
against (a) the same loop written with torch.stft / torch.istft on the same GPU and (b) that loop on the host CPU, and
the achieved bytes/s of ali_gl_ola / ali_gl_phase alone against their algorithmic bytes.  Needs a GPU; prints one line
per measurement.  ``--no-cpu`` skips (b), ``--calls N`` sets the timed calls (default 10)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from ali_hip import ops  # noqa: E402
from ali_hip.griffinlim import GriffinLim, griffinlim_torch  # noqa: E402

SETTINGS = {"audio": (dict(n_fft=255, win_length=128), 256, 128), "whale": (dict(n_fft=511, win_length=128, hop_length=24), 128, 256),
            "esrf": (dict(n_fft=1023, win_length=256, hop_length=79), 64, 512)}      # kwargs, batch, frames


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    for name, (kw, B, T) in SETTINGS.items():
        if a.only and name != a.only:
            continue
        gl = GriffinLim(**kw)
        F, win, hop = gl.F, gl.win, gl.hop
        g = torch.Generator().manual_seed(0)
        spec = torch.rand(B, F, T, generator=g).pow(4).cuda()
        ms = timed(lambda: gl(spec), a.calls)
        print(f"{name}: B={B} F={F} T={T} n_iter=32  graph replay {ms:.3f} ms/call ({gl.launches} launches)")
        ms_t = timed(lambda: griffinlim_torch(spec, **kw), max(2, a.calls // 3), warm=1)
        print(f"{name}: torch.stft/istft loop on the same GPU {ms_t:.3f} ms/call")
        if not a.no_cpu:
            sc = spec.cpu()
            t0 = time.time()
            griffinlim_torch(sc, **kw)
            print(f"{name}: torch.stft/istft loop on the host CPU, {torch.get_num_threads()} threads: {(time.time() - t0) * 1e3:.0f} ms/call")
        # the two per-iteration kernels alone, on the call's own buffers
        st = gl._states[(B, T)]
        ms_o = timed(lambda: ops.gl_ola(st["fr"], st["renv"], gl.n_fft, hop, st["L"], st["frames"]), 50)
        ms_p = timed(lambda: ops.gl_phase(st["Y"][0], st["Y"][1], st["mag"], gl.m, st["X"]), 50)
        by_o = 4.0 * (2 * B * T * win + B * (st["L"] + gl.n_fft))            # frames in and out, envelope-sized stretch
        by_p = 4.0 * B * T * F * (2 + 2 + 1 + 2)                              # Y, tprev, mag in, X out
        print(f"{name}: ali_gl_ola {ms_o * 1e3:.1f} us, {by_o / ms_o / 1e9:.2f} TB/s of {by_o / 1e6:.1f} MB algorithmic; "
              f"ali_gl_phase {ms_p * 1e3:.1f} us, {by_p / ms_p / 1e9:.2f} TB/s of {by_p / 1e6:.1f} MB algorithmic")


if __name__ == "__main__":
    main()
