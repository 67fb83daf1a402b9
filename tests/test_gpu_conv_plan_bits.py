"""The executor of csrc/gconv.hip transcribes the plan faithfully: output BYTES of a dozen launches, one per launch
shape the planner can decide, against digests recorded before the launch rules were gathered into one planner
(tests/golden/gconv_bits.json).  A dropped or swapped field of the plan (split count, tail split, dispatch order, XCD
chunk, uniform tiles, kernel instance, grid) changes the summation order or the result itself, and fp32 inputs drawn
from a normal distribution make every summation order show in the low bits; the split-K fold adds its slabs in slab
order, so every launch here is deterministic.

The geometries are the ones tests/test_gpu_conv_geometry.py and tests/test_gpu_conv_geometry_f16.py established as the
smallest that reach each path.  ``python tests/test_gpu_conv_plan_bits.py FILE`` writes the digests of the library it
runs on to FILE (how the golden file was made)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

# id -> (geometry B, H, W, C, P, Q, K, R, S, stride, pad; which: 0 ali_conv_fwd / 1 ali_conv_bwd_data; precision;
#        fp16 twins of both operands; fused BatchNorm statistics (bn_mode 1); tuning variables)
CASES = {
    # 600 blocks of 64 x 64 on uniform tiles (B = 64 rows per pixel): 512 whole, 88 cut two ways along K
    "tail": ((64, 16, 22, 64, 15, 20, 128, 2, 3, 1, 0), 0, "f32", False, False, {}),
    # the same under fp16: 150 tiles of 128 x 128, split-K over all of them
    "tail-f16-splitk": ((64, 16, 22, 64, 15, 20, 128, 2, 3, 1, 0), 0, "f16", False, False, {}),
    # 570 blocks of the fp16 loop, 58 left over and cut two ways
    "tail16": ((64, 18, 30, 64, 19, 30, 64, 2, 3, 1, 1), 0, "f16", False, False, {}),
    "tail16-twins": ((64, 18, 30, 64, 19, 30, 64, 2, 3, 1, 1), 0, "f16", True, False, {}),
    # gconv_kernel512<256, 256, .., 3>, ragged M and N
    "lds-dma": ((3, 9, 14, 64, 9, 15, 128, 3, 2, 1, 1), 0, "f16", True, False, {"ALI_BM": 256, "ALI_BN": 256}),
    # padded data gradient, pixel-major, whole k-loops: dispatched in the order of ali_conv_tile_order
    "ordered-dgrad": ((70, 5, 9, 64, 7, 9, 96, 3, 5, 1, 2), 1, "f32", False, False, {"ALI_SPLITK": 1}),
    # 2100 blocks, image-major: XCD-contiguous chunks with a ragged last one
    "xcd": ((4, 121, 142, 32, 120, 140, 128, 2, 3, 1, 0), 0, "f32", False, False, {}),
    # uniform tiles with the fused BatchNorm statistics of a "same" 3 x 3 convolution, split-K
    "uniform-bn": ((64, 6, 10, 32, 6, 10, 64, 3, 3, 1, 1), 0, "f32", False, True, {}),
    # MODE 3 (8 channels) and MODE 0 (6 channels) first layers
    "mode3": ((5, 13, 10, 8, 7, 4, 24, 2, 5, 2, 1), 0, "f32", False, False, {}),
    "mode0": ((3, 9, 14, 6, 9, 15, 10, 3, 2, 1, 1), 0, "f32", False, False, {}),
    # conv_first_kernel (one partial slot per image) and conv_s2_first_kernel
    "first-per-image": ((64, 12, 20, 8, 8, 16, 32, 5, 5, 1, 0), 0, "f32", False, True, {}),
    "first-row-walking": ((2, 40, 71, 4, 19, 35, 64, 5, 5, 2, 1), 0, "f32", False, False, {}),
}
# one ali_gemm_launch_multi of four recorded jobs: two split-K launches and two on uniform tiles
BATCH = [(6, 11, 8, 32, 6, 4, 72, 3, 4, 2, 1), (64, 6, 10, 32, 6, 10, 64, 3, 3, 1, 1)] * 2


def _ops():
    from ali_hip import ops
    return ops


def _normal(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32)).cuda()


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        torch.cuda.synchronize()
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _operands(gt, which, seed):
    """(geometry, gathered operand, packed weights, output) of ali_conv_fwd (0) / ali_conv_bwd_data (1)"""
    ops = _ops()
    B, H, W, C, P, Q, K, R, S, stride, pad = gt
    if which == 0:
        a, w, out = _normal(seed, B, H, W, C), _normal(seed + 1, K, R * S, C), torch.zeros(B, P, Q, K, device="cuda")
    else:
        a, w, out = _normal(seed, B, P, Q, K), _normal(seed + 1, C, R * S, K), torch.zeros(B, H, W, C, device="cuda")
    return ops.geom(*gt), a, w * (1.0 / (R * S * (C if which == 0 else K)) ** 0.5), out


def digest(cid):
    ops = _ops()
    gt, which, prec, twins, bn, env = CASES[cid]
    geom, a, w, out = _operands(gt, which, 1000 + 10 * sorted(CASES).index(cid))
    bias = _normal(7, out.shape[-1])
    if twins:
        ops.ensure_shadow16(a)
        ops.ensure_shadow16(w)
    with ops.tuning(**env), ops.precision(prec):
        part = None
        if bn:
            slots = ops.conv_mtiles(geom, which)[0]
            part = torch.zeros(2, out.shape[-1], slots, device="cuda")
            ep = ops.epilogue(bias=bias, act=ops.ACT_LEAKY, slope=0.2, bn_fwd=(part, 1, None, slots))
        else:
            ep = ops.epilogue(bias=bias, act=ops.ACT_LEAKY, slope=0.2)
        (ops.conv_fwd if which == 0 else ops.conv_bwd_data)(geom, a, w, out, ep)
        return _sha(out) if part is None else _sha(out, part)


def digest_batch():
    ops = _ops()
    ops.reload_tuning()
    outs, keep = [], []
    with ops.gemm_batch() as b:
        for i, gt in enumerate(BATCH):
            geom, a, w, out = _operands(gt, 0, 2000 + 10 * i)
            ops.conv_fwd(geom, a, w, out, ops.epilogue(bias=_normal(8 + i, out.shape[-1]), act=ops.ACT_LEAKY, slope=0.1))
            outs.append(out)
            keep.append((a, w))
        recorded = len(b.jobs)
    assert recorded == 4 or not ops.PAIR_GEMMS, recorded          # all four went out in ONE combined launch
    return _sha(*outs)


def _golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gconv_bits.json")
    with open(path) as f:
        return json.load(f)


@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_launch_bytes_are_unchanged(cid):
    assert digest(cid) == _golden()[cid]


@gpu
def test_four_job_launch_bytes_are_unchanged():
    assert digest_batch() == _golden()["gemm-batch-4"]


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "imagecfgen-pytorch_amd"))
    rec = {cid: digest(cid) for cid in CASES}
    rec["gemm-batch-4"] = digest_batch()
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))
