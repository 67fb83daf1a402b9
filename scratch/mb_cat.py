"""AudioMNIST attribute SCM at the training script's own shapes (attribute_scms.audio_mnist.train: batches of 10 000
rows; the counterfactual-score scripts: 128 rows per ``attrs_graph.sample``): the device path of ``ali_hip.cat`` against
the torch statement of the same graph run on CUDA tensors (a second graph with the device path switched off: ATen /
rocBLAS launches, autograd, ``torch.optim.Adam``, ``Categorical.sample`` and the host read of the redraw loop), and the
kernels of csrc/cat.hip alone.  Every call is timed on its own with device events after a warm-up; prints median, min
and max per measurement and the ratio of the medians.  Needs a GPU.  ``--calls N`` (default 50), ``--rows N`` (default
10000), ``--sweep`` (the forward + gradient launches alone over N = 32 .. 16384: where the launch floor ends)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from ali_hip import ops  # noqa: E402
from ali_hip.cat import CatStepper  # noqa: E402
import attribute_scms.audio_mnist as aa  # noqa: E402

TRIO = ("country_of_origin", "native_speaker", "accent")
SIZES = {"country_of_origin": 12, "native_speaker": 2, "accent": 15, "digit": 10, "age": 6, "gender": 2}


def timed(fn, calls, warm=5):
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


def report(what, new, old):
    print(f"{what}: HIP path median {new[0] * 1e3:.1f} us (min {new[1] * 1e3:.1f}, max {new[2] * 1e3:.1f}); torch statement "
          f"median {old[0] * 1e3:.1f} us (min {old[1] * 1e3:.1f}, max {old[2] * 1e3:.1f}); statement / HIP = "
          f"{old[0] / new[0]:.1f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    torch.manual_seed(0)
    N = a.rows
    ds = {k: torch.eye(c)[torch.arange(N) * 7 % c if k != "accent" else torch.randint(0, c, (N,))].cuda()
          for k, c in SIZES.items()}
    graph = aa.AudioMNISTCausalGraph(ds, device="cuda")
    ref = aa.AudioMNISTCausalGraph(ds, device="cuda")
    ref._cat = None                                             # the statement on the same GPU
    trio = [ds[k] for k in TRIO]
    obs = dict(zip(TRIO, trio))

    def script_step(g, opt):
        def step():
            opt.zero_grad()
            lp = g.log_prob(obs)
            loss = -(lp["native_speaker"] + lp["accent"]).mean()
            loss.backward()
            opt.step()
            return loss
        return step

    def params(g):
        return [p for k in TRIO[1:] for p in g.get_module(k).parameters()]
    old = timed(script_step(ref, torch.optim.Adam(params(ref), lr=1e-2)), a.calls)
    for capture in (True, False):
        stepper = CatStepper(graph, lr=1e-2, capture=capture)
        report(f"training step N={N} ({'HIP graph' if capture else 'three eager launches'})",
               timed(lambda: stepper.step(*trio), a.calls), old)
    report(f"training step N={N} (CatLogProb under autograd, torch Adam)",
           timed(script_step(graph, torch.optim.Adam(params(graph), lr=1e-2)), a.calls), old)

    # the score scripts' batch: 128 rows
    rows = {k: v[:128].argmax(1) for k, v in ds.items()}
    cond = {k: v for k, v in rows.items() if k != "accent"}

    def redraw_loop(g):                                          # the scripts' loop: redraw the batch until every row differs
        s = g.sample(obs_in=cond)
        while (s["accent"] == rows["accent"]).sum().item() > 0:
            new = g.sample(obs_in=cond)
            s["accent"] = torch.where(s["accent"] == rows["accent"], new["accent"], s["accent"])
        return s
    report("sample, 128 rows", timed(lambda: graph.sample(obs_in={"country_of_origin": rows["country_of_origin"]}), a.calls),
           timed(lambda: ref.sample(obs_in={"country_of_origin": rows["country_of_origin"]}), a.calls))
    report("sample_differing, 128 rows (statement: the redraw loop with its host read)",
           timed(lambda: graph.sample_differing(cond, "accent", rows["accent"]), a.calls), timed(lambda: redraw_loop(ref), a.calls))
    act = {"native_speaker": 1 - rows["native_speaker"]}
    report("sample_cf, 128 rows", timed(lambda: graph.sample_cf(rows, act), a.calls), timed(lambda: ref.sample_cf(rows, act), a.calls))

    # the kernels alone (event-timed single launches include the launch itself)
    st = graph._cat
    _, Cn, Ca = st.sizes
    wgt = torch.randn(N, 2).cuda()
    y = (rows["native_speaker"], rows["accent"])
    c128 = trio[0][:128]
    for what, fn in ((f"ali_cat_nll lp + out3 N={N}", lambda: ops.cat_nll(st.theta, st.towers, *trio)),
                     (f"ali_cat_nll lp + gtheta (two launches) N={N}", lambda: ops.cat_nll(st.theta, st.towers, *trio, wgt=wgt, want_grad=True)),
                     ("ali_cat_map sample N=128", lambda: ops.cat_map(ops.CAT_SAMPLE, st.theta, st.towers, c128, Cn, Ca)),
                     ("ali_cat_map differ N=128", lambda: ops.cat_map(ops.CAT_DIFFER, st.theta, st.towers, c128, Cn, Ca,
                                                                     y=(y[0], None), v=(None, y[1]), node=1)),
                     ("ali_cat_map abduct N=128", lambda: ops.cat_map(ops.CAT_ABDUCT, st.theta, st.towers, c128, Cn, Ca, y=y)),
                     ("ali_cat_map cf N=128", lambda: ops.cat_map(ops.CAT_CF, st.theta, st.towers, c128, Cn, Ca, y=y,
                                                                 v=(1 - y[0], None), cf_mask=1))):
        med, lo, hi = timed(fn, a.calls)
        print(f"{what}: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
    if a.sweep:
        n = 32
        while n <= min(N, 16384):
            part = [t[:n] for t in trio]
            med, lo, hi = timed(lambda: ops.cat_nll(st.theta, st.towers, *part, want_grad=True), a.calls)
            print(f"sweep ali_cat_nll lp + gtheta N={n}: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
            n *= 2


if __name__ == "__main__":
    main()
