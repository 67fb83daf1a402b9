"""The contrastive family at the evaluation scripts' setting: a ``MNISTClassifier`` (random weights: the time does not
depend on them), 28 x 28 images, one pertinent-negative search (5 rounds of 1000 iterations) and one counterfactual
search (5 rounds of 100) with the default hyper-parameters, at B = 1 and B = 64 images per call; and one
pertinent-positive search (pn's hyper-parameters, background 0), whose captured time is also given as a ratio to the
captured pertinent-negative search of the same run.

Three ways per search: ``ContrastiveSearch`` replayed from its HIP graph, the same executor launched eagerly, and the
yardstick -- the torch statement of the same search (``cem_pn_statement`` / ``ce_statement`` / ``cem_pp_statement``) on
the same GPU under
autograd, the classifier called as a plain ``nn.Sequential`` on torch's stock operators.  The statement is warmed with a
short search (5 iterations, one round) so that its operators are set up, then timed on whole searches.

Every call is timed on its own with a host clock around work that ends in a device synchronise; prints median, min and
max.  Needs a GPU.  ``--calls N`` (default 3) for the executor, ``--ref-calls N`` (default 1) for the statement,
``--modes`` (default pn ce pp) for the searches."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from ali_hip.contrast import ContrastiveSearch, ce_statement, cem_pn_statement, cem_pp_statement  # noqa: E402


def timed(fn, calls, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def line(what, r, n):
    print(f"contrast: {what}: median {r[0]:.1f} ms (min {r[1]:.1f}, max {r[2]:.1f}) over {n} call(s)", flush=True)
    return r[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--ref-calls", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--modes", nargs="+", default=["pn", "ce", "pp"], choices=["pn", "ce", "pp"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    from classifiers.mnist import MNISTClassifier
    torch.manual_seed(0)
    clf = MNISTClassifier().cuda().eval()
    stock = lambda x: torch.nn.Sequential.forward(clf, x)  # noqa: E731
    g = torch.Generator().manual_seed(1)
    images = (torch.rand(max(a.batches), 1, 28, 28, generator=g) * 2 - 1).cuda()
    res = {}
    statements = {"pn": cem_pn_statement, "ce": ce_statement, "pp": cem_pp_statement}
    for mode in a.modes:
        statement = statements[mode]
        for B in a.batches:
            x = images[:B].contiguous()
            for capture in (True, False):
                ex = ContrastiveSearch(clf, mode, capture=capture)
                tag = "captured" if capture else "eager"
                res[mode, B, tag] = line(f"{mode} search B={B} ({ex.replays_per_search} replays) executor {tag}",
                                         timed(lambda: ex.run(x), a.calls), a.calls)
            statement(stock, x, num_iterations=5, binary_search_steps=1)
            res[mode, B, "ref"] = line(f"{mode} search B={B} torch statement under autograd, stock operators",
                                       timed(lambda: statement(stock, x), a.ref_calls, 0), a.ref_calls)
            print(f"contrast: {mode} B={B}: statement / captured = {res[mode, B, 'ref'] / res[mode, B, 'captured']:.2f}x, "
                  f"statement / eager = {res[mode, B, 'ref'] / res[mode, B, 'eager']:.2f}x, per replay captured "
                  f"{res[mode, B, 'captured'] / ex.replays_per_search * 1e3:.1f} us", flush=True)
            if mode == "pp" and ("pn", B, "captured") in res:
                print(f"contrast: B={B}: captured pp / captured pn = "
                      f"{res['pp', B, 'captured'] / res['pn', B, 'captured']:.3f}", flush=True)


if __name__ == "__main__":
    main()
