"""cf_eval family at the AudioMNIST scripts' shapes (60 subjects, 10 digits, 5400 validation recordings of 128 x 128):
one ``ManifoldBank`` build at 5400 x 16384, ``errors`` at M = 81 and M = 4096, and one ``CounterfactualEval.add`` at
B = 81 with the AudioMNIST stacks (BiGAN, fine-tuned BiGAN, VAE, a 60-way subject classifier; captured and eager), each
against the statement audiomnist_cf_eval.py runs on the same GPU: ``(cf.unsqueeze(1) - rows).square().sum((1, 2))`` for
the subject's own recordings, and the same over the whole data set streamed in batches of 128 for every other
subject's, with the ``.cpu()`` reads of the script.  Then the two kernels of csrc/cfeval.hip alone, with the bytes each
must move and the rate that gives.  Every call is timed on its own with device events after a warm-up; prints median,
min and max.  Needs a GPU.  ``--calls N`` (default 10); the torch statements run ``max(3, N // 3)`` times."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from ali_hip import ops  # noqa: E402
from ali_hip.cfeval import CounterfactualEval, ManifoldBank  # noqa: E402

O, C, PER_CELL, D = 60, 10, 9, 128 * 128


def timed(fn, calls, warm=2):
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


@torch.no_grad()
def script_errors(cf, rows, r_owner, r_cls, subject, d, stream=128):
    """audiomnist_cf_eval.py:93-131 for one (subject, d) and one image tensor, the ratio read back as the script does"""
    same_x = rows[(r_owner == subject) & (r_cls == d)]
    same = (cf.unsqueeze(1) - same_x).square().sum(dim=(1, 2)) / len(same_x)
    other = torch.zeros(len(cf), device=cf.device)
    denom = 0
    keep = r_owner != subject
    s_rows, s_cls = rows[keep], r_cls[keep]
    for lo in range(0, len(s_rows), stream):
        other_x = s_rows[lo:lo + stream][s_cls[lo:lo + stream] == d]
        other += (cf.unsqueeze(1) - other_x).square().sum(dim=(1, 2))
        denom += len(other_x)
    other /= denom
    return (same / other).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    slow = max(3, a.calls // 3)
    torch.manual_seed(0)
    N = O * C * PER_CELL
    rows = (torch.clip(torch.randn(N, D), -3, 3) / 3).cuda()
    cell = torch.arange(N) % (O * C)
    r_owner, r_cls = (cell // C).cuda(), (cell % C).cuda()

    # ---- the bank, once per evaluation
    t = timed(lambda: ManifoldBank(rows, r_owner, r_cls, O, C), a.calls)
    show(f"ManifoldBank build {N} x {D} (CSR by torch ops + ali_group_moments)", t)
    bank = ManifoldBank(rows, r_owner, r_cls, O, C)

    # ---- errors for one (subject, digit) batch and for a large batch
    for M in (81, 4096):
        cf = (torch.rand(M, D) * 2 - 1).cuda()
        ow = torch.full((M,), 7, dtype=torch.int32).cuda()
        cl = torch.full((M,), 3, dtype=torch.int32).cuda()
        t_hip = timed(lambda: bank.errors(cf, ow, cl), a.calls)
        t_ref = timed(lambda: script_errors(cf, rows, r_owner, r_cls, 7, 3), slow, warm=1)
        show(f"errors M={M}: HIP path", t_hip)
        show(f"errors M={M}: the script's broadcasting statement, data set streamed in batches of 128", t_ref,
             f"; statement / HIP = {t_ref[0] / t_hip[0]:.1f}x")

    # ---- one batch of the evaluation loop: 81 recordings of one subject, five images each
    import image_scms.audio_mnist as pm
    from classifiers.audio_mnist import AudioMNISTClassifier
    from deepscm_vae.audio_mnist import VAE
    B = 81
    ops.set_workspace_bytes(1 << 30)             # (the d = 64 stacks at B = 81; the bank's kernels need 100 KB of it)
    models = {"bigan": (pm.Encoder().cuda().eval(), pm.Generator().cuda().eval()),
              "bigan_ft": (pm.Encoder().cuda().eval(), pm.Generator().cuda().eval()),
              "vae": VAE(device="cuda").eval()}
    clf = AudioMNISTClassifier(60).cuda().eval()
    x = (torch.clip(torch.randn(B, 1, 128, 128), -3, 3) / 3).cuda()
    attrs = {k: torch.eye(n)[torch.randint(0, n, (B,))].cuda() for k, n in pm.ATTRIBUTE_DIMS.items()}
    cf_attrs = dict(attrs)
    cf_attrs["digit"] = torch.eye(10)[torch.full((B,), 3)].cuda()
    subject = torch.full((B,), 7).cuda()
    z = torch.randn(3, B, 512, 1, 1).cuda()

    @torch.no_grad()
    def script_body():
        out = {}
        for name, m in models.items():
            if name == "vae":
                codes, G = m.encoder(x, attrs)[0], m.decoder
            else:
                codes, G = m[0](x, attrs), m[1]
            imgs = {"cf": G(codes, cf_attrs), "int": G(torch.randn_like(codes), cf_attrs)}
            for kind, img in imgs.items():
                out[f"{name}_{kind}"] = script_errors(img.flatten(start_dim=1), rows, r_owner, r_cls, 7, 3)
                out[f"{name}_{kind}_hit"] = (clf(img).argmax(1) == subject).int().cpu().numpy()
        return out
    t_ref = timed(script_body, slow, warm=1)
    show("loop body B=81, 3 models x (cf, int): the scripts' statements on the same modules", t_ref)
    for capture in (True, False):
        ev = CounterfactualEval(models, bank, {"subject": clf}, capture=capture)
        t = timed(lambda: ev.add(x, attrs, cf_attrs, subject, 3, labels={"subject": subject}, z=z), a.calls)
        show(f"CounterfactualEval.add B=81: {'graph replay' if capture else 'eager'}", t,
             f"; statements / add = {t_ref[0] / t[0]:.1f}x")
        ev.reset()

    # ---- the kernels alone
    cellv = r_owner * C + r_cls
    order = torch.argsort(cellv, stable=True).to(torch.int32)
    start = torch.cat([cellv.new_zeros(1), torch.bincount(cellv, minlength=O * C).cumsum(0)]).to(torch.int32)
    t = timed(lambda: ops.group_moments(rows, order, start, O, C), a.calls)
    nb = 4 * N * D + 16 * (O * C + C) * D + 8 * O * C * D * 2
    show(f"ali_group_moments N={N} D={D} O*C={O * C} (both launches; the totals re-read S and Q)", t,
         f"; {nb} bytes -> {nb / t[0] / 1e6:.1f} GB/s")
    for M in (81, 4096):
        cf = (torch.rand(M, D) * 2 - 1).cuda()
        ow = torch.randint(0, O, (M,), dtype=torch.int32).cuda()
        cl = torch.randint(0, C, (M,), dtype=torch.int32).cuda()
        out = torch.empty(M, 3, device="cuda")
        t = timed(lambda: ops.manifold_err(cf, ow, cl, bank.S, bank.Q, bank.TS, bank.TQ, bank.cnt, bank.tcnt, out=out),
                  a.calls)
        nb = (4 + 32) * M * D + 12 * M
        show(f"ali_manifold_err M={M} D={D}, random cells", t,
             f"; {nb} bytes when no moment row is shared -> {nb / t[0] / 1e6:.1f} GB/s")


if __name__ == "__main__":
    main()
