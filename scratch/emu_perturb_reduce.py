"""Why ``ali_morpho_shear_reduce`` takes its reduce operators in fp64: an emulation on the host of the
kernel's two sums -- T = warped RW^T over the set pixels of a row in ascending x, raw = 255 RH T in ascending y -- with
the operators and the arithmetic in a chosen precision, held to the entry-wise yardstick of the kernel tests
(``flow_cases.within_yardstick``: |got - fp64| <= 4 |CPU-fp32 statement - fp64| + 4 fp32 ulp) on the batch of
``tests/test_gpu_morpho_perturb_kernels.py::test_shear_reduce`` at 28 x 28, scale 4, B = 70.  Three variants: operators,
T and sums in fp32 (what the issue sketched); operators rounded to fp32 with T and sums in fp64; all fp64 (the kernel).
Prints, for each, the pixels outside the yardstick, the worst ratio and the largest error in fp32 ulps of the reference.
No GPU.  ``--shape H W s B``."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import perturb_cases as pc  # noqa: E402
from flow_cases import EPS32, FLOOR_ULPS, MULT  # noqa: E402
from morphomnist import morpho, perturb  # noqa: E402

SHEARS = (0.0, 0.31, -0.31, 0.9, -0.9, 1000.0)                       # of the kernel tests


def sequential(terms, dtype):
    """the sum of ``terms`` [n, ...] along axis 0 in ascending order, every addition rounded to ``dtype``"""
    acc = np.zeros(terms.shape[1:], dtype=dtype)
    for t in terms:
        acc = (acc + t).astype(dtype)
    return acc


def emulate(warped, scale, op_dtype, acc_dtype):
    """raw [H, W] fp32 as the kernel forms it, with operators rounded to ``op_dtype`` and T and the sums in ``acc_dtype``
    (the products of the second sum are rounded on their own here; the kernel fuses them, which is no less exact)"""
    Hh, Wh = warped.shape
    RH = morpho.reduce_operator(Hh // scale, scale).astype(op_dtype).astype(acc_dtype)
    RW = morpho.reduce_operator(Wh // scale, scale).astype(op_dtype).astype(acc_dtype)
    T = sequential(warped.T[:, :, None] * RW.T[:, None, :], acc_dtype)             # [Wh, Hh, W] summed over x
    acc = sequential(RH.T[:, :, None] * T[:, None, :], acc_dtype)                   # [Hh, H, W] summed over y
    return (acc_dtype(255) * acc).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=(28, 28, 4, 70), metavar=("H", "W", "s", "B"))
    H, W, s, B = ap.parse_args().shape
    images = pc.built(H * s, W * s, B)
    ref, yard, got = [], [], {"fp32 operators, fp32 sums": [], "fp32 operators, fp64 sums": [], "fp64 (the kernel)": []}
    for b in range(B):
        bitmap, _, sums, status = perturb.reshape_stage(images[b], 1.0, None, s)
        if status:
            continue
        warped = perturb.shear_stage(bitmap, sums, SHEARS[b % len(SHEARS)], s)[2]
        ref.append(perturb.shear_stage(bitmap, sums, SHEARS[b % len(SHEARS)], s)[3])
        yard.append(perturb.shear_stage(bitmap, sums, SHEARS[b % len(SHEARS)], s, np.float32)[3])
        got["fp32 operators, fp32 sums"].append(emulate(warped, s, np.float32, np.float32))
        got["fp32 operators, fp64 sums"].append(emulate(warped, s, np.float32, np.float64))
        got["fp64 (the kernel)"].append(emulate(warped, s, np.float64, np.float64))
    ref, yard = np.stack(ref), np.stack(yard).astype(np.float64)
    ydev = np.abs(yard - ref)
    floor = FLOOR_ULPS * EPS32 * np.abs(ref) + 1e-37
    print(f"{H} x {W}, scale {s}: {len(ref)} live images of {B}, {ref.size} pixels; the CPU-fp32 statement's largest "
          f"error {ydev.max():.3g}")
    for name, raws in got.items():
        err = np.abs(np.stack(raws).astype(np.float64) - ref)
        beyond = np.clip(err - floor, 0, None)
        ratio = np.where(beyond > 0, beyond / np.maximum(ydev, 1e-300), 0)
        bad = err > MULT * ydev + floor
        ulps = (err / np.maximum(EPS32 * np.abs(ref), 1e-37)).max()
        print(f"  {name}: {int(bad.sum())} pixels outside the yardstick, worst ratio {ratio.max():.3g}, largest error "
              f"{err.max():.3g} = {ulps:.3g} fp32 ulp of the reference")


if __name__ == "__main__":
    main()
