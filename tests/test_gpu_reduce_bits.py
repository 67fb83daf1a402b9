"""The bits of every kernel that reduces in a fixed order (csrc/xent.hip, vae.hip, gan.hip, explain.hip): lanes by xor
butterfly, waves in order, blocks through write-through partials that the block arriving last folds in a fixed order.
The other tests of these kernels compare with fp64 within a tolerance, which a reordered sum would pass; this one
compares the raw bits of every output with ``tests/golden/reduce_bits.npz``.

The golden file is recorded on an MI355X at the commit it names (``commit`` inside it), with
``python tests/test_gpu_reduce_bits.py --record [--commit NAME] [--out PATH]``.  It holds the outputs of up to 64
elements whole and a 64-bit checksum (blake2b over the bytes) of the larger ones.  A change of the fold order, of a
butterfly or of the fp64 row arithmetic changes these bits and is a bug unless it is the point of the change; a ROCm
upgrade that changes the device's ``exp`` / ``log`` / ``tanh`` / ``pow`` is a legitimate reason to record it again.

Inputs are closed forms such as ((i * 37 + 11) % 101 - 50) / 16, exact in fp32: nothing depends on a generator.  Every
case also makes the same calls twice and asks for equal bits, and asks that the workspace's reserved head (the arrival
counter at its end included) is back at zero.  Shapes are the smallest that reach each stage of each kernel; they are
listed at the cases."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_bits.npz")
WHOLE = 64                                    # outputs of up to this many elements are stored whole


def _ops():
    from ali_hip import ops
    return ops


def seq(shape, mul=37, add=11, mod=101, div=16.0):
    """((i * mul + add) % mod - mod // 2) / div over the flattened index i, as fp32 on the device"""
    n = int(np.prod(shape))
    i = torch.arange(n, dtype=torch.int64)
    return (((i * mul + add) % mod - mod // 2).double() / div).float().reshape(shape).cuda()


def bits(t):
    """the raw bits of a tensor: int32 for fp32, the integers themselves otherwise"""
    t = t.detach().contiguous().cpu()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).numpy().reshape(-1)


def entry(a):
    """what the golden file keeps of an output"""
    if a.size <= WHOLE:
        return a
    return np.array([int.from_bytes(hashlib.blake2b(a.tobytes(), digest_size=8).digest(), "little")], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------- the cases
# Each returns {name: tensor}.  (B, C) etc. as the kernels name them.
def xent(B, C):
    """(9, 10): 3 blocks, the last one partly empty; (5, 70): lanes stride twice; (4100, 3): 1024 blocks, grid stride"""
    ops = _ops()
    logit = seq((B, C), 37, 11, 101, 16.0)
    r, j = torch.arange(B).reshape(B, 1), torch.arange(C).reshape(1, C)
    hot = (j == (r * 7 + 3) % C).float()
    soft = ((r * 5 + j * 3) % 8).float() / 8.0
    target = torch.where(r % 2 == 0, hot, soft).cuda()
    acc = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    out2, gl, pred = ops.softmax_xent(logit, target, gscale=0.5, want_pred=True, hits_accum=acc)
    bare, none, _ = ops.softmax_xent(logit, target, want_grad=False)
    assert none is None
    return {"out2": out2, "glogit": gl, "pred": pred, "hits_accum": acc, "out2_nograd": bare}


def latent(B, S, L):
    """with KL.  (3, 2, 300): columns stride; (300, 1, 5): the fold strides over more than 256 partials"""
    ops = _ops()
    mean, lv = seq((B, L), 37, 11, 101, 16.0), seq((B, L), 29, 5, 67, 32.0)
    eps = seq((S, B, L), 13, 7, 89, 16.0)
    rows = torch.empty(S * B, L, device="cuda")
    kl, _ = ops.vae_latent_fwd(mean, lv, S, rows, eps=eps)
    return {"rows": rows, "kl": kl}


def loglik(B, S, P):
    """(2, 2, 1032): vector path; (2, 2, 1030): scalar path; (515, 2, 8): 1030 rows on 1024 blocks, a strided fold"""
    ops = _ops()
    x, xhat = seq((B, P), 37, 11, 101, 64.0), seq((S * B, P), 29, 5, 67, 64.0)
    kl_sum = torch.full((1,), 12.5, device="cuda")
    out3, g = ops.vae_loglik(x, xhat, S, -5.0, kl_sum, 2.0, gscale=0.5)
    bare, none = ops.vae_loglik(x, xhat, S, -5.0, kl_sum, 2.0, want_grad=False)
    assert none is None
    return {"out3": out3, "gxhat": g, "out3_nograd": bare}


def penalty(B, P):
    """(3, 4100): vector path, threads stride; (3, 4099): scalar path; (1, 4): fewer elements than waves"""
    ops = _ops()
    g0 = seq((B, P), 37, 11, 101, 256.0)
    inplace = g0.clone()
    out2, v = ops.gp_penalty(inplace, weight=10.0, out=inplace)
    assert v is inplace
    bare, none = ops.gp_penalty(g0, weight=10.0, want_v=False)
    assert none is None
    return {"out2": out2, "v": v, "out2_nov": bare}


def dist(S, N):
    """(3, 9000): split 3; (2, 262149): the split capped at 64; L1 and L2, one x row and one per row of y"""
    ops = _ops()
    y, x = seq((S, N), 37, 11, 101, 16.0), seq((S, N), 29, 5, 67, 16.0)
    out = {}
    for mode, tag in ((ops.DIST_L1, "l1"), (ops.DIST_L2, "l2")):
        out[tag + "_x1"] = ops.row_dist(x[:1], y, mode)
        out[tag + "_xS"] = ops.row_dist(x, y, mode)
    return out


def hinge(B, C):
    """rows with a target, rows compared with orig_pred (target < 0), and the same rows with nothing to compare with"""
    ops = _ops()
    logit, orig = seq((B, C), 37, 11, 101, 16.0), seq((B, C), 29, 5, 67, 16.0)
    target = torch.tensor([(b * 4 + 1) % C if b % 3 else -1 for b in range(B)], dtype=torch.int32, device="cuda")
    m = seq((B,), 13, 7, 89, 8.0)
    out, gl = ops.cf_hinge(logit, target, m, 0.75, orig_pred=orig)
    out_n, gl_n = ops.cf_hinge(logit, target, m, 0.75)
    return {"out": out, "glogit": gl, "out_noorig": out_n, "glogit_noorig": gl_n}


def cf_input():
    """a softmax segment of width 300 through a table and a tanh segment; B = 2, two steps"""
    ops = _ops()
    B, W = 2, 300
    segs = [(ops.CF_SOFTMAX, W, 0, 32, 0, 0), (ops.CF_TANH, 32, W, 0, -1, W)]     # (every column of a row is written)
    table = seq((W, ops.CF_EMB), 13, 7, 89, 64.0)
    lay = ops.CfLayout(segs, [table], 32 + ops.CF_EMB, 32 + ops.CF_EMB + 32)
    raw = seq((B, lay.raw_ld), 37, 11, 101, 16.0)
    m, v = torch.zeros_like(raw), torch.zeros_like(raw)
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    g_rows = seq((B, lay.ld), 29, 5, 67, 32.0)
    out = {}
    for it in (1, 2):
        rows, attrs = ops.cf_input_fwd(lay, raw, None)
        graw = torch.empty_like(raw)
        ops.cf_input_step(lay, g_rows, rows, attrs, raw, m, v, step, 0.1, graw=graw)
        out.update({f"rows{it}": rows, f"attrs{it}": attrs, f"graw{it}": graw, f"raw{it}": raw.clone(),
                    f"m{it}": m.clone(), f"v{it}": v.clone(), f"step{it}": step.clone()})
    return out


CASES = {}
for _fn, _shapes in ((xent, [(9, 10), (5, 70), (4100, 3)]), (latent, [(3, 2, 300), (300, 1, 5)]),
                     (loglik, [(2, 2, 1032), (2, 2, 1030), (515, 2, 8)]), (penalty, [(3, 4100), (3, 4099), (1, 4)]),
                     (dist, [(3, 9000), (2, 262149)]), (hinge, [(5, 10), (3, 70)]), (cf_input, [()])):
    for _s in _shapes:
        CASES["-".join([_fn.__name__] + [str(n) for n in _s])] = (_fn, _s)


def run_case(name):
    """the case's outputs as {name/output: bits}: run twice, equal bits asked for, the reserved head at zero"""
    fn, shape = CASES[name]
    first = {k: bits(t) for k, t in fn(*shape).items()}
    again = {k: bits(t) for k, t in fn(*shape).items()}
    for k in first:
        assert np.array_equal(first[k], again[k]), f"{name}/{k}: a second run gives other bits"
    head = _ops().workspace(torch.device("cuda"))[:4096]
    assert int(head.count_nonzero()) == 0, f"{name}: the workspace's reserved head is not back at zero"
    return {f"{name}/{k}": a for k, a in first.items()}


_GOLD = {}


def golden():
    if not _GOLD:
        with np.load(GOLDEN) as z:
            _GOLD.update({k: z[k] for k in z.files})
    return _GOLD


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bits_are_the_recorded_ones(name):
    gold = golden()
    got = run_case(name)
    assert sorted(k for k in gold if k.startswith(name + "/")) == sorted(got), name
    for k, a in got.items():
        e, want = entry(a), gold[k]
        what = "bits" if a.size <= WHOLE else f"checksum of {a.size} elements"
        assert e.dtype == want.dtype and np.array_equal(e, want), \
            f"{k}: {what} {e.tolist()} differ from the recorded {want.tolist()} (commit {gold['commit']})"


def record(path, commit):
    out = {"commit": np.array(commit), "device": np.array(torch.cuda.get_device_name(0))}
    for name in CASES:
        for k, a in run_case(name).items():
            out[k] = entry(a)
            print(f"{k}: {a.size} elements -> {out[k].tolist() if out[k].size <= 4 else '(whole)'}")
    np.savez_compressed(path, **out)
    print(f"recorded {len(out) - 2} outputs of {len(CASES)} cases at {commit} into {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    import argparse
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "imagecfgen-pytorch_amd"))
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--commit", default=None, help="default: git rev-parse --short HEAD")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    if a.commit is None:
        import subprocess
        a.commit = subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], text=True).strip()
    assert torch.cuda.is_available(), "recording needs the GPU"
    record(a.out, a.commit)
