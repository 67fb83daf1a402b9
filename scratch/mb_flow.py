"""Attribute-SCM family at the training script's own shapes (train_mnist_attribute_scm.py: batches of 10 000 rows;
causal_graph_cf.py: 100 counterfactuals of one row each): the device path of ``ali_hip.flow`` against the torch
statement of the same graph run on CUDA tensors (``MNISTCausalGraph.statement(torch.float32, "cuda")``: ATen launches
of the transforms in ``attribute_scms/_flows.py``, autograd, ``torch.optim.Adam``), and the four kernels of
csrc/flow.hip alone.  Every call is timed on its own with device events after a warm-up; prints median, min and max per
measurement and the ratio of the medians.  Needs a GPU.  ``--calls N`` (default 50), ``--rows N`` (default 10000)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch  # noqa: E402

from ali_hip import ops  # noqa: E402
from ali_hip.flow import FlowStepper  # noqa: E402
import attribute_scms.mnist as am  # noqa: E402

NAMES = ("thickness", "intensity", "slant")


def synth_attrs(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(n, 13)
    a[torch.arange(n), torch.randint(0, 10, (n,), generator=g)] = 1
    t = torch.exp(torch.randn(n, generator=g) * 0.3 + 0.8)
    a[:, 10] = t
    a[:, 11] = 60 + 190 * torch.sigmoid(0.5 * t + torch.randn(n, generator=g))
    a[:, 12] = torch.randn(n, generator=g) * 0.3
    return a


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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no time"
    torch.manual_seed(0)
    N = a.rows
    table = synth_attrs(N).cuda()
    cols = {k: table[:, j:j + 1].contiguous() for k, j in zip(NAMES, (10, 11, 12))}
    graph = am.MNISTCausalGraph(table, device="cuda")

    # one training step
    ref = graph.statement(torch.float32, "cuda")
    params = [p for k in NAMES for p in ref.get_module(k).parameters()]
    opt = torch.optim.Adam(params, lr=1e-2)

    def statement_step():
        opt.zero_grad()
        lp = ref.log_prob(cols)
        loss = -(lp["thickness"] + lp["intensity"] + lp["slant"]).mean()
        loss.backward()
        opt.step()
        return loss
    old = timed(statement_step, a.calls)
    for capture in (True, False):
        stepper = FlowStepper(graph, lr=1e-2, capture=capture)
        report(f"training step N={N} ({'HIP graph' if capture else 'three eager launches'})",
               timed(lambda: stepper.step(*(cols[k] for k in NAMES)), a.calls), old)
    dopt = torch.optim.Adam([p for k in NAMES for p in graph.get_module(k).parameters()], lr=1e-2)

    def autograd_step():
        dopt.zero_grad()
        lp = graph.log_prob(cols)
        loss = -(lp["thickness"] + lp["intensity"] + lp["slant"]).mean()
        loss.backward()
        dopt.step()
        return loss
    report(f"training step N={N} (FlowLogProb under autograd, torch Adam)", timed(autograd_step, a.calls), old)

    # counterfactuals: the script's 100 calls of one row against one call of 100 rows
    for g in (graph, ref):
        for tr in g.trainable():
            tr.training = False
    rows = {k: v[:100] for k, v in cols.items()}
    rows["digit"] = table[:100, :10].argmax(1)
    act = {"thickness": rows["thickness"] + 1}

    def one_by_one(g):
        return [g.sample_cf({k: v[r:r + 1] for k, v in rows.items()}, {"thickness": act["thickness"][r:r + 1]})
                for r in range(100)]
    calls = max(a.calls // 5, 5)
    report("sample_cf, 100 calls of one row", timed(lambda: one_by_one(graph), calls), timed(lambda: one_by_one(ref), calls))
    report("sample_cf, one call of 100 rows", timed(lambda: graph.sample_cf(rows, act), a.calls),
           timed(lambda: ref.sample_cf(rows, act), a.calls))
    report(f"sample N={N}", timed(lambda: graph.sample(n=N), a.calls), timed(lambda: ref.sample(n=N), a.calls))

    # the kernels alone (event-timed single launches include the launch itself)
    st = graph._flow
    t, i, s = (cols[k] for k in NAMES)
    wgt = torch.randn(N, 3).cuda()
    obs = torch.cat([t, i, s], 1).contiguous()
    logits, y = torch.randn(N, 6).cuda(), torch.randint(0, 6, (N,)).cuda()
    for what, fn in (("ali_flow_stats", lambda: ops.flow_stats(t)),
                     ("ali_flow_nll lp only", lambda: ops.flow_nll(t, i, s, st.theta, st.cst, st.moving)),
                     ("ali_flow_nll lp + gtheta", lambda: ops.flow_nll(t, i, s, st.theta, st.cst, st.moving, wgt=wgt,
                                                                      want_grad=True)),
                     ("ali_flow_map counterfactual", lambda: ops.flow_map(obs, st.theta, st.cst, st.moving, st.moving,
                                                                          cf_mask=1, val=obs)),
                     ("ali_gumbel_posterior C=6", lambda: ops.gumbel_posterior(logits, y))):
        med, lo, hi = timed(fn, a.calls)
        print(f"{what} N={N}: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)


if __name__ == "__main__":
    main()
