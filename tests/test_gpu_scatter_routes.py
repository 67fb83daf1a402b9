"""Every launch plan of the scatter-form transposed convolutions (csrc/direct.hip: ali_tconv_scatter /
ali_tconv_scatter_wgrad; csrc/elementwise.hip: ali_col2im).

ali_tconv_scatter picks tconv_scatter_kernel<NT> by tap columns (N = NC * R * S: NT = 1..4 tiles of 16) and shrinks the
output tile of a block from 32x64 to 4x8 until the contributions of the input pixels that reach it fit 64 KB of LDS: 19
(NT; OBH x OBW) plans over the filters ali_tconv_scatter_ok admits.  ali_tconv_scatter_wgrad picks
tconvs_wgrad_mfma_kernel<NT,4> by taps (NT = 1: <= 16, 2: 17..32) and halves the band height RB 8 -> 4 -> 2 -> 1 until the
band's rows of the one-channel map fit 64 KB: 8 plans, then the refusal.  ali_col2im has one template per NC = 1..8.
``ops.tconv_scatter_plan`` -- the launches' own plan -- is asserted first in every case, so a later change of the launch
arithmetic cannot move a case silently; every case has a rectangular map and spans at least two tiles (bands) per axis
with a ragged last one.

Convention of test_gpu_conv_geometry.py (its RTOL, YARD and ``check``).  Reference: F.conv_transpose2d with autograd on
the CPU in fp64, bias and activation applied in fp64 (ali_col2im alone: the contributions as the input channels of a
transposed convolution with one-hot weights, which is the same sum).  Yardstick: the same computation in CPU fp32.  With
e(t) = max|t - ref64| every device output is held to e <= 4 * e(cpu fp32) and e <= 2e-4 * max|ref64|.  Outputs are
prefilled with NaN; a strided output's neighbour columns must keep it; operand columns the op must not read (the other
channels of a strided one-channel map, its positions no tap reaches, the padding columns of the contribution rows) are
NaN.  Inputs are seeded from the case id.  Every forward case also runs the two-launch form (1x1 ali_conv_fwd +
ali_col2im) and holds the two to each other at 2e-5; weight gradients run twice in their own layout and once in the
pack's [taps][64] order, all bit-identical, and leave the workspace's reserved head at zero.  DESIGN.md 4 has the
measured ratios per plan.

plan                    case ids
  scatter<1;16x32>      f-1-16x32, f-n16
  scatter<1;16x64>      f-1-16x64
  scatter<1;32x64>      f-1-32x64, f-dead-tile
  scatter<2;8x16>       f-2-8x16
  scatter<2;8x32>       f-2-8x32
  scatter<2;16x32>      f-2-16x32
  scatter<2;16x64>      f-2-16x64, f-n32
  scatter<2;32x64>      f-2-32x64, f-n18
  scatter<3;8x16>       f-3-8x16, f-n48
  scatter<3;8x32>       f-3-8x32, f-3-8x32-lds
  scatter<3;16x32>      f-3-16x32
  scatter<3;16x64>      f-3-16x64
  scatter<3;32x64>      f-3-32x64, f-n35
  scatter<4;4x8>        f-4-4x8
  scatter<4;4x16>       f-4-4x16
  scatter<4;8x16>       f-4-8x16
  scatter<4;16x32>      f-4-16x32, f-dgrad-planes
  scatter<4;16x64>      f-4-16x64
  scatter<4;32x64>      f-4-32x64, f-n49
  scatter_wgrad<1;rb8>  w-1-rb8-s1, w-1-rb8-4x4, w-2x7-135
  scatter_wgrad<1;rb4>  w-2x7-136, w-2x7-291
  scatter_wgrad<1;rb2>  w-2x7-292, w-2x7-681
  scatter_wgrad<1;rb1>  w-2x7-682
  scatter_wgrad<2;rb8>  w-5x5-429, w-5x5-429-short, w-4x5-453, w-5x4-209, w-2-rb8-s1
  scatter_wgrad<2;rb4>  w-5x5-430, w-5x5-743, w-4x5-454, w-5x4-210
  scatter_wgrad<2;rb2>  w-5x5-744, w-5x5-1168, w-5x4-390
  scatter_wgrad<2;rb1>  w-5x5-1169, w-5x5-1636, w-4x5-1364
  col2im<NC>            c-nc1 .. c-nc8, c-stride (NC = 1)
(test_cases_name_every_plan holds this table against the cases and the cases against the query.)
"""
import ctypes
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_geometry import RTOL, YARD, check, nan   # noqa: F401  (RTOL, YARD: the bounds ``check`` applies)

gpu = pytest.mark.gpu

NO_MFMA = {"ALI_NO_T1_MFMA": 1}
LDS_MAX = 64 * 1024
WS_RESERVED = 4096           # the head of every workspace: the GEMM kernels' arrival counters
TWO_LAUNCH_RTOL = 2e-5       # one-launch against two-launch form (test_gpu_kernels.py's bound for the pair)

# (case id, output) -> why the 4x yardstick does not apply (the 2e-4 cap still does).  At most 3; see DESIGN.md 4.
CAP_ONLY = {}


def _ops():
    from ali_hip import ops
    return ops


def _lib():
    import ali_hip
    return ali_hip.load()


def _last_error():
    msg = _lib().ali_last_error()
    return msg.decode() if msg else ""


class Fw:
    """One ali_tconv_scatter launch: x [B,H,W,64] through an R x S filter to NC channels of [B,Hout,Wout,ostride]"""

    def __init__(self, cid, plan, B, H, W, NC, R, S, stride, pad, opad=(0, 0), bias=True, act="none", ostride=None):
        self.id, self.plan, self.op = "f-" + cid, f"scatter<{plan}>", "fwd"
        self.B, self.H, self.W, self.NC, self.R, self.S, self.stride, self.pad, self.opad = B, H, W, NC, R, S, stride, pad, opad
        self.bias, self.act, self.ostride = bias, act, ostride or NC
        self.Hout = (H - 1) * stride - 2 * pad + R + opad[0]
        self.Wout = (W - 1) * stride - 2 * pad + S + opad[1]
        self.N, self.T = NC * R * S, R * S

    def query(self):
        return ("fwd", self.B, self.H, self.W, 64, self.Hout, self.Wout, self.R, self.S, self.stride, self.pad, self.NC, self.ostride)


class Wg:
    """One ali_tconv_scatter_wgrad launch: big [B,P,Q,64], small = one channel of [B,H,W,sstride], dw [64,1,R,S]"""

    def __init__(self, cid, plan, B, P, Q, R, S, stride, pad, opad=(0, 0), sstride=1):
        self.id, self.plan, self.op = "w-" + cid, f"scatter_wgrad<{plan}>", "wgrad"
        self.B, self.P, self.Q, self.R, self.S, self.stride, self.pad, self.opad, self.sstride = B, P, Q, R, S, stride, pad, opad, sstride
        self.H = (P - 1) * stride - 2 * pad + R + opad[0]
        self.W = (Q - 1) * stride - 2 * pad + S + opad[1]
        self.T = R * S

    def query(self):
        return ("wgrad", self.B, self.P, self.Q, 64, self.H, self.W, self.R, self.S, self.stride, self.pad, 1, self.sstride)


class C2:
    """One ali_col2im launch: contrib [B,H,W,ldc] to NC channels of [B,Hout,Wout,ostride]"""

    def __init__(self, cid, NC, B, H, W, R, S, stride, pad, opad=(0, 0), ldc=None, ostride=None, bias=True, act="none"):
        self.id, self.op = "c-" + cid, "col2im"
        self.B, self.H, self.W, self.NC, self.R, self.S, self.stride, self.pad, self.opad = B, H, W, NC, R, S, stride, pad, opad
        self.N = NC * R * S
        self.ldc, self.ostride, self.bias, self.act = ldc or self.N, ostride or NC, bias, act
        self.Hout = (H - 1) * stride - 2 * pad + R + opad[0]
        self.Wout = (W - 1) * stride - 2 * pad + S + opad[1]


# Forward: the smallest map that spans two tiles per axis with a ragged last one, on the filter that takes the plan.
# Across the cases: pad 0 / 1 / R - 1, output_padding 0 / stride - 1 different per axis, bias or not, the three
# activations, ostride = NC and > NC.           id, plan (NT;OBHxOBW), B, H, W, NC, R, S, stride, pad
FWD = [
    Fw("1-16x32", "1;16x32", 2, 12, 33, 2, 6, 1, 1, 0, act="tanh", ostride=3),                  # 17 x 33
    Fw("1-16x64", "1;16x64", 3, 17, 62, 2, 1, 4, 1, 0, bias=False, act="leaky"),                # 17 x 65
    Fw("1-32x64", "1;32x64", 2, 17, 32, 1, 3, 5, 2, 1, opad=(0, 1)),                            # 33 x 66
    Fw("2-8x16", "2;8x16", 2, 10, 20, 1, 8, 4, 1, 3, act="tanh"),                               # 11 x 17, N = 32
    Fw("2-8x32", "2;8x32", 3, 7, 35, 2, 6, 2, 1, 1, bias=False, act="leaky"),                   # 10 x 34
    Fw("2-16x32", "2;16x32", 2, 17, 30, 2, 2, 5, 1, 0, ostride=4),                              # 18 x 34
    Fw("2-16x64", "2;16x64", 2, 10, 33, 2, 3, 5, 2, 2, opad=(1, 0), act="tanh"),                # 18 x 65, pad R - 1
    Fw("2-32x64", "2;32x64", 2, 18, 34, 1, 5, 5, 2, 2, opad=(1, 1), act="tanh"),                # 36 x 68: the production tail
    Fw("3-8x16", "3;8x16", 2, 6, 15, 2, 5, 4, 1, 0, act="leaky"),                               # 10 x 18
    Fw("3-8x32", "3;8x32", 3, 12, 33, 2, 3, 6, 1, 2, bias=False),                               # 10 x 34, pad R - 1
    Fw("3-16x32", "3;16x32", 2, 9, 16, 2, 4, 6, 2, 1, opad=(1, 0), act="tanh", ostride=5),      # 19 x 34, N = 48
    Fw("3-16x64", "3;16x64", 2, 8, 30, 2, 3, 6, 2, 0, opad=(0, 1)),                             # 17 x 65
    Fw("3-32x64", "3;32x64", 2, 12, 22, 2, 3, 6, 3, 1, opad=(2, 0), act="leaky"),               # 36 x 67
    Fw("4-4x8", "4;4x8", 2, 7, 11, 1, 8, 8, 1, 0, act="tanh"),                                  # 14 x 18, N = 64: LDC = 65
    Fw("4-4x16", "4;4x16", 3, 5, 14, 2, 4, 8, 1, 1, bias=False),                                # 6 x 19, N = 64
    Fw("4-8x16", "4;8x16", 2, 13, 19, 2, 4, 7, 1, 3, act="leaky"),                              # 10 x 19, pad R - 1
    Fw("4-16x32", "4;16x32", 2, 8, 14, 2, 4, 7, 2, 0, opad=(1, 0), act="tanh"),                 # 19 x 33
    Fw("4-16x64", "4;16x64", 2, 7, 22, 2, 4, 7, 3, 2, opad=(0, 2), ostride=3),                  # 18 x 68
    Fw("4-32x64", "4;32x64", 2, 9, 17, 2, 4, 7, 4, 1, opad=(3, 0), act="leaky"),                # 37 x 69: stride 4
    # 11 * 34 = 374 input pixels x LDC 37 x 4 = 65416 bytes: 120 under the limit
    Fw("3-8x32-lds", "3;8x32", 2, 6, 33, 2, 6, 3, 1, 0, act="tanh"),                            # 11 x 35
    # the NT boundaries from both sides, with the N that filters of at most 8 x 8 taps and 1-2 channels can form next to
    # them: 16 | 18 (17 is prime), 32 | 35 (33 = 3 * 11, 34 = 2 * 17), 48 | 49
    Fw("n16", "1;16x32", 2, 16, 30, 2, 2, 4, 1, 0, act="leaky"),                                # 17 x 33
    Fw("n18", "2;32x64", 2, 12, 21, 1, 3, 6, 3, 0, opad=(0, 2)),                                # 36 x 68
    Fw("n32", "2;16x64", 2, 9, 32, 2, 4, 4, 2, 1, opad=(1, 1), bias=False),                     # 19 x 65
    Fw("n35", "3;32x64", 2, 9, 17, 1, 5, 7, 4, 2, opad=(0, 3), act="tanh"),                     # 33 x 70
    Fw("n48", "3;8x16", 3, 6, 12, 1, 6, 8, 1, 1),                                               # 9 x 17
    Fw("n49", "4;32x64", 2, 12, 23, 1, 7, 7, 3, 3, opad=(2, 1), act="tanh"),                    # 36 x 68, pad 3
    # Hout = 7 * 4 + 2 + 3 = 33: output row 32 is a tile of its own, its only congruent tap (r = 0) points at input row 8,
    # which does not exist -- the tile has no input pixel and every pixel of the row is act(bias)
    Fw("dead-tile", "1;32x64", 2, 8, 17, 2, 2, 3, 4, 0, opad=(3, 1), act="tanh"),               # 33 x 68
    # the consumed input planes of a first Conv2d(C, 64, 5, stride 2, pad 2)'s data gradient on a 37 x 70 input, as
    # chain._plane_grads launches it: x = the [B, 19, 35, 64] gradient map, two planes, no bias; test_forward takes its
    # reference from autograd's dx[:, planes]
    Fw("dgrad-planes", "4;16x32", 2, 19, 35, 2, 5, 5, 2, 2, opad=(0, 1), bias=False),           # 37 x 70
]
DGRAD_PLANES = (3, 1)        # of a 5-channel input

# Weight gradient.  B = 2 and an odd P with a ragged last band; the 64-channel operand stays under 3 MB, which bounds P
# by the width: 9 / 11 rows up to Q = 430, 7 at 743 / 744, 5 at 1168 / 1169, 3 at 1636.
#                   id, plan (NT;rbRB), B, P, Q, R, S, stride, pad
WGRAD = [
    # 5 x 5, stride 2 (the production filter): both sides of every limit of the band height
    Wg("5x5-429", "2;rb8", 2, 11, 429, 5, 5, 2, 2, opad=(1, 1)),             # 65440 bytes of LDS; 858 steps per band
    Wg("5x5-429-short", "2;rb8", 2, 5, 429, 5, 5, 2, 2, opad=(0, 1)),        # P < RB: one band of 5 rows
    Wg("5x5-430", "2;rb4", 2, 11, 430, 5, 5, 2, 2, opad=(1, 0)),
    Wg("5x5-743", "2;rb4", 2, 7, 743, 5, 5, 2, 1, sstride=4),                # 65520 bytes
    Wg("5x5-744", "2;rb2", 2, 7, 744, 5, 5, 2, 2, opad=(1, 1)),
    Wg("5x5-1168", "2;rb2", 2, 5, 1168, 5, 5, 2, 0, opad=(1, 1)),            # 65504 bytes; pad 0: row and column H - 1 / W - 1 unreached
    Wg("5x5-1169", "2;rb1", 2, 5, 1169, 5, 5, 2, 2),
    Wg("5x5-1636", "2;rb1", 2, 3, 1636, 5, 5, 2, 2, opad=(1, 1)),            # 65504 bytes: the last width the launch takes
    # rectangular filters at their own limits (test_case_takes_its_plan holds each limit against the query)
    Wg("4x5-453", "2;rb8", 2, 9, 453, 4, 5, 2, 1, opad=(1, 0)),
    Wg("4x5-454", "2;rb4", 2, 9, 454, 4, 5, 2, 1),
    Wg("4x5-1364", "2;rb1", 2, 3, 1364, 4, 5, 2, 0, opad=(0, 1)),
    Wg("5x4-209", "2;rb8", 2, 11, 209, 5, 4, 3, 1, opad=(2, 0), sstride=4),
    Wg("5x4-210", "2;rb4", 2, 9, 210, 5, 4, 3, 0, opad=(1, 2)),
    Wg("5x4-390", "2;rb2", 2, 7, 390, 5, 4, 3, 2),
    # one tap tile (<= 16 taps): 2 x 7, stride 4 -- rows 2, 3 (mod 4) of the small map are reached by no tap
    Wg("2x7-135", "1;rb8", 2, 11, 135, 2, 7, 4, 0, opad=(3, 0)),
    Wg("2x7-136", "1;rb4", 2, 9, 136, 2, 7, 4, 1, opad=(0, 3)),
    Wg("2x7-291", "1;rb4", 2, 7, 291, 2, 7, 4, 0),
    Wg("2x7-292", "1;rb2", 2, 7, 292, 2, 7, 4, 1, opad=(2, 1), sstride=4),
    Wg("2x7-681", "1;rb2", 2, 5, 681, 2, 7, 4, 0, opad=(1, 3)),
    Wg("2x7-682", "1;rb1", 2, 3, 682, 2, 7, 4, 0, opad=(3, 3)),
    # stride 1; 11 * 7 = 77 pixels (not a multiple of 4), 14 four-pixel steps per band (< 32: not every wave's prefetch
    # slot is used); 17 taps by the side of 16
    Wg("1-rb8-s1", "1;rb8", 3, 11, 7, 3, 3, 1, 1),
    Wg("1-rb8-4x4", "1;rb8", 2, 9, 13, 4, 4, 2, 1, opad=(1, 0)),             # 16 taps
    Wg("2-rb8-s1", "2;rb8", 2, 9, 15, 3, 6, 1, 0),                           # 18 taps, stride 1, pad 0
]

# ali_col2im: one case per template; R != S, strides 1..4, ldc > N (NaN in the padding columns), ostride > NC,
# output_padding, output pixels no tap reaches (stride > R or S).    id, NC, B, H, W, R, S, stride, pad
COL2IM = [
    C2("nc1", 1, 3, 7, 9, 2, 3, 1, 1, act="tanh"),
    C2("nc2", 2, 3, 6, 9, 3, 2, 2, 0, opad=(1, 0), ldc=15, act="leaky"),
    C2("nc3", 3, 2, 5, 8, 1, 4, 3, 0, opad=(2, 1), ostride=5),                           # rows 1, 2 (mod 3): bias only
    C2("nc4", 4, 2, 5, 7, 4, 2, 4, 1, opad=(3, 0), bias=False, act="tanh"),              # columns with (ox + 1) % 4 >= 2: 0
    C2("nc5", 5, 2, 6, 5, 5, 3, 2, 2, opad=(1, 1), ldc=76),
    C2("nc6", 6, 3, 5, 6, 2, 2, 1, 0, act="leaky", ostride=6),
    C2("nc7", 7, 2, 5, 7, 3, 5, 3, 1, ostride=8, act="tanh"),
    C2("nc8", 8, 2, 6, 7, 2, 4, 2, 1, opad=(0, 1), ldc=72, bias=False),
    # ew_grid (csrc/elementwise.hip) launches at most 2048 blocks of 256 threads = 524288 threads, one output pixel each
    # per step: 2 * 514 * 512 = 526336 pixels, so the first 2048 threads take a second step
    C2("stride", 1, 2, 257, 256, 2, 2, 2, 0, act="tanh"),
]

CASES = FWD + WGRAD + COL2IM
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ----------------------------------------------------------------------------------------------------------------------
# host side (no GPU): the launch arithmetic restated, the plans, the refusals

def fwd_restated(NC, R, S, stride):
    """(NT, OBH, OBW, LDS bytes) of ali_tconv_scatter, restated here: the query is held to it, not it to the query"""
    N = NC * R * S
    ldc = N | 1

    def npx(bh, bw):
        return ((bh - 1 + R - 1) // stride + 1) * ((bw - 1 + S - 1) // stride + 1)
    obh, obw = 32, 64
    while npx(obh, obw) * ldc * 4 > LDS_MAX and (obh > 4 or obw > 8):
        if obw > 2 * obh and obw > 8:
            obw >>= 1
        elif obh > 4:
            obh >>= 1
        else:
            obw >>= 1
    return (N + 15) // 16, obh, obw, npx(obh, obw) * ldc * 4


def wgrad_restated(Q, R, S, stride):
    """(tap tiles, RB, LDS bytes) of ali_tconv_scatter_wgrad, None where the band image of one row exceeds 64 KB"""
    nt = (R * S + 15) // 16

    def lds(rb):
        return max((((rb - 1) * stride + R) * ((Q - 1) * stride + S) + 3) & ~3, 4 * 4 * nt * 64 * 4) * 4
    rb = 8
    while rb > 1 and lds(rb) > LDS_MAX:
        rb >>= 1
    return None if lds(rb) > LDS_MAX else (nt, rb, lds(rb))


def plan_of(ops, c):
    return ops.tconv_scatter_plan(*c.query())


def _docstring_table():
    table = {}
    for line in __doc__.splitlines():
        m = re.match(r"  (scatter\S+)\s+(.*)", line)
        if m:
            table[m.group(1)] = set(m.group(2).split(", "))
    return table


def test_cases_name_every_plan():
    ops = _ops()
    ops.reload_tuning()
    # forward: every filter ali_tconv_scatter_ok admits has a plan -- the "filter too large" arm of the launch is
    # unreachable (the 4 x 8 tile of the largest filter, 1 x 8 x 8, needs 11 * 15 * 65 * 4 = 42900 bytes) -- and the
    # plan is the restated arithmetic's
    plans = set()
    for NC in (1, 2):
        for R in range(1, 9):
            for S in range(1, 9):
                for stride in range(1, 5):
                    if not ops.tconv_scatter_ok(64, NC, R, S, stride):
                        assert NC * R * S > 64
                        assert ops.tconv_scatter_plan("fwd", 2, 9, 11, 64, 40, 50, R, S, stride, 0, NC=NC) is None
                        continue
                    got = ops.tconv_scatter_plan("fwd", 2, 9, 11, 64, 40, 50, R, S, stride, 0, NC=NC)
                    assert got is not None, (NC, R, S, stride, _last_error())
                    assert (got.nt, got.obh, got.obw, got.lds) == fwd_restated(NC, R, S, stride), (NC, R, S, stride, got)
                    assert got.lds <= LDS_MAX
                    plans.add(got.name)
    assert len(plans) == 19 and plans == {c.plan for c in FWD}, plans ^ {c.plan for c in FWD}
    # weight gradient: every filter of at most 32 taps, stride 1..4, over a sweep of the width
    widths = sorted(set(range(1, 48)) | set(range(48, 8400, 29)) | {c.Q + d for c in WGRAD for d in (0, 1)} | {1637, 2047, 2048})
    plans = set()
    for R in range(1, 33):
        for S in range(1, 32 // R + 1):
            for stride in range(1, 5):
                for Q in widths:
                    got = ops.tconv_scatter_plan("wgrad", 2, 9, Q, 64, 8 * stride + R, (Q - 1) * stride + S, R, S, stride, 0)
                    want = wgrad_restated(Q, R, S, stride)
                    if want is None:
                        assert got is None, (R, S, stride, Q, got)
                        continue
                    assert got is not None, (R, S, stride, Q, _last_error())
                    assert (got.nt, got.rb, got.lds) == want and got.lds <= LDS_MAX, (R, S, stride, Q, got)
                    plans.add(got.name)
    assert len(plans) == 8 and plans == {c.plan for c in WGRAD}, plans ^ {c.plan for c in WGRAD}
    # the cases
    assert len(CAP_ONLY) <= 3 and all(k[0] in BY_ID for k in CAP_ONLY)
    assert all(c.H != c.W for c in CASES)
    for table in (FWD, WGRAD, COL2IM):
        assert 3 * sum(c.R != c.S for c in table) >= len(table)
    assert len({(c.R, c.S, c.stride) for c in WGRAD if c.R != c.S}) >= 3
    assert {c.NC for c in COL2IM} == set(range(1, 9))
    # the docstring's table is the cases'
    by_plan = {}
    for c in FWD + WGRAD:
        by_plan.setdefault(c.plan, set()).add(c.id)
    assert _docstring_table() == by_plan


def _ew_threads():
    """the largest grid of ew_grid, in threads, read from the source"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "imagecfgen-pytorch_amd", "csrc",
                            "elementwise.hip")).read()
    block = int(re.search(r"constexpr int kEwBlock = (\d+);", src).group(1))
    body = src[src.index("static inline int ew_grid("):]
    cap = int(re.search(r"if \(b > (\d+)\) b = \1;", body).group(1))
    return cap * block


def _reached(n_in, n_out, taps, stride, pad):
    """which positions of an output axis some tap of some input position reaches"""
    hit = [False] * n_out
    for i in range(n_in):
        for r in range(taps):
            o = i * stride - pad + r
            if 0 <= o < n_out:
                hit[o] = True
    return hit


# (filter, stride) -> the last width ali_tconv_scatter_wgrad takes at each band height, and the first it refuses
WGRAD_LIMITS = {
    (5, 5, 2): {8: 429, 4: 743, 2: 1168, 1: 1636, "refused": 1637},
    (4, 5, 2): {8: 453, 4: 817, 2: 1363, 1: 2046, "refused": 2047},
    (5, 4, 3): {8: 209, 4: 389, 2: 682, 1: 1091, "refused": 1092},
    (2, 7, 4): {8: 135, 4: 291, 2: 681, 1: 2047, "refused": 2048},
}


@pytest.mark.parametrize("key", list(WGRAD_LIMITS), ids=["%dx%d-s%d" % k for k in WGRAD_LIMITS])
def test_weight_gradient_limits(key):
    """every limit of the band height: the last width that fits names RB, the next one RB / 2 (or the refusal)"""
    ops = _ops()
    ops.reload_tuning()
    R, S, stride = key
    lim = WGRAD_LIMITS[key]
    nt = (R * S + 15) // 16

    def ask(Q):
        got = ops.tconv_scatter_plan("wgrad", 2, 9, Q, 64, 8 * stride + R, (Q - 1) * stride + S, R, S, stride, 0)
        assert _lib().ali_tconv_scatter_wgrad_ws(2, 9, Q, 64, R, S, stride) == (0 if got is None else got.ws)
        return got
    for rb in (8, 4, 2, 1):
        at, past = ask(lim[rb]), ask(lim[rb] + 1)
        assert at.name == f"scatter_wgrad<{nt};rb{rb}>" and at.lds <= LDS_MAX, (key, rb, at)
        if rb > 1:
            assert past.name == f"scatter_wgrad<{nt};rb{rb // 2}>", (key, rb, past)
        else:
            assert past is None and lim["refused"] == lim[1] + 1
            assert "64 KB" in _last_error()
    if key == (5, 5, 2):    # the production filter's figures
        assert [ask(lim[rb]).lds for rb in (8, 4, 2, 1)] == [65440, 65520, 65504, 65504]


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_case_takes_its_plan(cid):
    """the launches' own plan names the case's -- and the arithmetic of the launch parameters puts the case where its
    comment says: tiles per axis with a ragged last tile, bands with a ragged last band, steps per band"""
    ops, c = _ops(), BY_ID[cid]
    ops.reload_tuning()
    if c.op == "col2im":
        pixels = c.B * c.Hout * c.Wout
        assert (pixels > _ew_threads()) == (cid == "c-stride")
        if cid == "c-stride":
            assert _ew_threads() == 2048 * 256 and pixels - _ew_threads() == 2048        # no larger than the cap asks for
        assert c.ldc >= c.N and c.ostride >= c.NC
        return
    got = plan_of(ops, c)
    assert got is not None and got.name == c.plan, (cid, got, _last_error())
    with ops.tuning(**NO_MFMA):
        assert plan_of(ops, c) is None
    if c.op == "fwd":
        nt, obh, obw, lds = fwd_restated(c.NC, c.R, c.S, c.stride)
        assert (got.nt, got.obh, got.obw, got.lds) == (nt, obh, obw, lds)
        ty, tx = -(-c.Hout // obh), -(-c.Wout // obw)
        assert ty >= 2 and tx >= 2 and c.Hout % obh and c.Wout % obw, (cid, c.Hout, c.Wout)
        assert got.blocks == ty * tx * c.B and c.B in (2, 3)
        assert c.opad[0] < c.stride and c.opad[1] < c.stride
        assert c.H * c.W * c.B * 64 * 4 <= 4 << 20
        want_n = {"f-n16": 16, "f-n18": 18, "f-n32": 32, "f-n35": 35, "f-n48": 48, "f-n49": 49, "f-4-4x8": 64,
                  "f-2-8x16": 32, "f-3-16x32": 48}.get(cid)
        assert want_n is None or c.N == want_n
        if cid == "f-3-8x32-lds":
            assert lds == 65416
        if cid == "f-dead-tile":    # row 32 is the second tile row; r = 0 is its only congruent tap and points past the map
            assert c.Hout == 33 and obh == 32 and (32 + c.pad) % c.stride == 0 and (32 + c.pad) // c.stride == c.H
            assert c.R <= c.stride
        if cid == "f-dgrad-planes":
            assert (c.Hout % 2, c.Wout % 2) == (1, 0)
            assert ((c.Hout + 2 * c.pad - c.R) // c.stride + 1, (c.Wout + 2 * c.pad - c.S) // c.stride + 1) == (c.H, c.W)
    else:
        nt, rb, lds = wgrad_restated(c.Q, c.R, c.S, c.stride)
        assert (got.nt, got.rb, got.lds) == (nt, rb, lds)
        bands = -(-c.P // rb)
        assert (got.bands, got.blocks) == (bands, c.B * bands)
        assert got.ws == got.blocks * 64 * c.T * 4 + WS_RESERVED == _lib().ali_tconv_scatter_wgrad_ws(c.B, c.P, c.Q, 64, c.R, c.S, c.stride)
        last = c.P - (bands - 1) * rb
        assert rb == 1 or last < rb, (cid, "the last band is ragged", c.P, rb)
        assert (bands == 1) == (cid == "w-5x5-429-short")
        assert c.B * c.P * c.Q * 64 * 4 < 3_000_000
        steps = -(-min(rb, c.P) * c.Q // 4)
        if cid == "w-1-rb8-s1":
            assert steps < 32 and (c.P * c.Q) % 4 and (last * c.Q) % 4
        if cid == "w-5x5-429":
            assert steps > 64
        lim = WGRAD_LIMITS.get((c.R, c.S, c.stride))
        if lim:     # a case named after a limit sits on it or one past it
            assert c.Q in {lim[r] + d for r in (8, 4, 2, 1) for d in (0, 1)} - {lim["refused"]}, cid


def test_the_table_covers_what_the_issue_lists():
    """pad 0 / 1 / R - 1, output_padding 0 and stride - 1 different per axis, bias or not, the three activations,
    ostride = NC and > NC (forward); stride 1, pad 0 and > 0, output_padding with unreached positions, sstride 4 (wgrad)"""
    assert {0, 1} <= {c.pad for c in FWD} and any(c.pad == c.R - 1 and c.pad > 1 for c in FWD)
    assert any(c.opad == (0, 0) for c in FWD)
    assert any(c.opad[0] == c.stride - 1 != c.opad[1] for c in FWD) and any(c.opad[1] == c.stride - 1 != c.opad[0] for c in FWD)
    assert {c.bias for c in FWD} == {True, False} and {c.act for c in FWD} == {"none", "leaky", "tanh"}
    assert any(c.ostride == c.NC for c in FWD) and any(c.ostride > c.NC for c in FWD)
    assert {c.stride for c in FWD} == {1, 2, 3, 4} == {c.stride for c in WGRAD} == {c.stride for c in COL2IM}
    assert any(c.pad == 0 for c in WGRAD) and any(c.pad > 0 for c in WGRAD) and any(c.sstride == 4 for c in WGRAD)
    assert any(c.opad != (0, 0) and not all(_reached(c.P, c.H, c.R, c.stride, c.pad))
               and not all(_reached(c.Q, c.W, c.S, c.stride, c.pad)) for c in WGRAD)
    assert any(c.ldc > c.N for c in COL2IM) and any(c.ostride > c.NC for c in COL2IM) and any(c.opad != (0, 0) for c in COL2IM)
    assert any(not all(_reached(c.H, c.Hout, c.R, c.stride, c.pad)) for c in COL2IM)


# (what, query arguments, a word of the message): the launch refuses with ALI_ERR_BAD_ARG, the query answers None
#                 op, B, H, W, C, Hout, Wout, R, S, stride, pad, NC, ostride
REFUSED = [
    ("fwd-C-32", ("fwd", 2, 5, 7, 32, 7, 9, 3, 3, 1, 0, 1, 1), "bad argument"),
    ("fwd-NC-3", ("fwd", 2, 5, 7, 64, 7, 9, 3, 3, 1, 0, 3, 3), "bad argument"),
    ("fwd-N-65", ("fwd", 2, 5, 7, 64, 9, 19, 5, 13, 1, 0, 1, 1), "bad argument"),       # (5 * 13 = 65 tap columns)
    ("fwd-N-70", ("fwd", 2, 5, 7, 64, 9, 13, 5, 7, 1, 0, 2, 2), "bad argument"),        # (R, S <= 8, only N > 64)
    ("fwd-R-9", ("fwd", 2, 5, 7, 64, 13, 7, 9, 1, 1, 0, 1, 1), "bad argument"),
    ("fwd-stride-5", ("fwd", 2, 5, 7, 64, 23, 33, 3, 3, 5, 0, 1, 1), "bad argument"),
    ("fwd-B-65536", ("fwd", 65536, 1, 2, 64, 1, 2, 1, 1, 1, 0, 1, 1), "bad argument"),
    ("fwd-ostride-1", ("fwd", 2, 5, 7, 64, 7, 9, 3, 3, 1, 0, 2, 1), "bad argument"),
    ("wgrad-K-32", ("wgrad", 2, 5, 7, 32, 7, 9, 3, 3, 1, 0, 1, 1), "unsupported shape"),
    ("wgrad-33-taps", ("wgrad", 2, 5, 7, 64, 7, 17, 3, 11, 1, 0, 1, 1), "unsupported shape"),
    ("wgrad-5x5-1637", ("wgrad", 2, 3, 1637, 64, 7, 3275, 5, 5, 2, 2, 1, 1), "64 KB"),
    ("wgrad-2x7-2048", ("wgrad", 2, 3, 2048, 64, 10, 8195, 2, 7, 4, 0, 1, 1), "64 KB"),
]
REFUSED_IDS = [r[0] for r in REFUSED]


@pytest.mark.parametrize("what,q,word", REFUSED, ids=REFUSED_IDS)
def test_refusals_of_the_query(what, q, word):
    ops = _ops()
    ops.reload_tuning()
    op, B, H, W, C, Hout, Wout, R, S, stride, pad, NC, ostride = q
    assert ops.tconv_scatter_plan(op, B, H, W, C, Hout, Wout, R, S, stride, pad, NC=NC, ostride=ostride) is None
    assert word in _last_error() and "ali_tconv_scatter" in _last_error()
    out = (ctypes.c_int64 * 6)()
    assert _lib().ali_tconv_scatter_plan({"fwd": 0, "wgrad": 1}[op], B, H, W, C, Hout, Wout, NC, ostride, R, S, stride, pad, out) == -1
    if op == "wgrad":
        assert _lib().ali_tconv_scatter_wgrad_ws(B, H, W, C, R, S, stride) == 0
    elif what not in ("fwd-B-65536", "fwd-ostride-1"):       # (those two are the launch's, not the filter's)
        assert not ops.tconv_scatter_ok(C, NC, R, S, stride)
    # one step back the shape is served
    back = {"fwd-C-32": dict(C=64), "fwd-NC-3": dict(NC=2), "fwd-N-65": dict(S=8, Wout=14), "fwd-N-70": dict(NC=1, ostride=1), "fwd-R-9": dict(R=8, Hout=12),
            "fwd-stride-5": dict(stride=4, Hout=19, Wout=27), "fwd-B-65536": dict(B=65535), "fwd-ostride-1": dict(ostride=2),
            "wgrad-K-32": dict(C=64), "wgrad-33-taps": dict(S=10, Wout=16), "wgrad-5x5-1637": dict(W=1636, Wout=3273),
            "wgrad-2x7-2048": dict(W=2047, Wout=8191)}[what]
    kw = dict(zip("op B H W C Hout Wout R S stride pad NC ostride".split(), q))
    kw.update(back)
    assert ops.tconv_scatter_plan(kw.pop("op"), **kw) is not None, (what, _last_error())


def test_more_than_a_million_bands_is_refused():
    """B * bands > 2^20 slabs: by the query alone (the operand would be hundreds of megabytes)"""
    ops = _ops()
    ops.reload_tuning()
    for B, P in ((1 << 17, 64), (1 << 17, 65), (1 << 20, 8), (1 << 20, 9)):
        got = ops.tconv_scatter_plan("wgrad", B, P, 5, 64, 2 * P + 1, 11, 3, 3, 2, 0)
        bands = -(-P // 8)
        assert (got is None) == (B * bands > 1 << 20), (B, P, got)
        if got is None:
            assert "2^20" in _last_error() and _lib().ali_tconv_scatter_wgrad_ws(B, P, 5, 64, 3, 3, 2) == 0
        else:
            assert got.blocks == 1 << 20


def test_no_mfma_setting_refuses_every_scatter_launch():
    ops = _ops()
    with ops.tuning(**NO_MFMA):
        assert not ops.tconv_scatter_ok(64, 1, 5, 5, 2)
        assert _lib().ali_tconv_scatter_wgrad_ws(2, 9, 11, 64, 5, 5, 2) == 0
        assert all(plan_of(ops, c) is None for c in FWD + WGRAD)
    assert ops.tconv_scatter_ok(64, 1, 5, 5, 2) and _lib().ali_tconv_scatter_wgrad_ws(2, 9, 11, 64, 5, 5, 2) > 0


# ----------------------------------------------------------------------------------------------------------------------
# references (computed once per case, never modified)

def _slope(dt):
    return torch.tensor(0.2).to(dt)      # (the device's slope is the fp32 0.2)


def _act(pre, act, dt):
    if act == "tanh":
        return torch.tanh(pre)
    if act == "leaky":
        return torch.where(pre > 0, pre, pre * _slope(dt))
    return pre


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.id.encode()))


def _inputs(c):
    g, t = _gen(c), {}
    if c.op == "fwd":
        t["x"] = torch.randn(c.B, 64, c.H, c.W, generator=g)
        t["bias"] = torch.randn(c.NC, generator=g) * 0.5
        if c.id == "f-dgrad-planes":        # the whole Conv2d weight [64, 5, R, S]; the launch sees two of its planes
            t["wconv"] = torch.randn(64, 5, c.R, c.S, generator=g) / (c.T * 5) ** 0.5
            t["w"] = t["wconv"][:, list(DGRAD_PLANES)].contiguous()
        else:
            t["w"] = torch.randn(64, c.NC, c.R, c.S, generator=g) * (c.stride ** 2 / (64 * c.T)) ** 0.5
    elif c.op == "wgrad":
        t["big"] = torch.randn(c.B, 64, c.P, c.Q, generator=g)
        t["small"] = torch.randn(c.B, 1, c.H, c.W, generator=g)
    else:
        t["contrib"] = torch.randn(c.B, c.N, c.H, c.W, generator=g)
        t["bias"] = torch.randn(c.NC, generator=g) * 0.5
        onehot = torch.zeros(c.N, c.NC, c.R, c.S)         # contribution column (r * S + s) * NC + ch -> tap (r, s) of ch
        for r in range(c.R):
            for s in range(c.S):
                for ch in range(c.NC):
                    onehot[(r * c.S + s) * c.NC + ch, ch, r, s] = 1.0
        t["w"] = onehot
    return t


def _host(c, t, dt):
    if c.op == "wgrad":
        w = torch.zeros(64, 1, c.R, c.S, dtype=dt, requires_grad=True)
        y = F.conv_transpose2d(t["big"].to(dt), w, None, stride=c.stride, padding=c.pad, output_padding=c.opad)
        (dw,) = torch.autograd.grad(y, w, t["small"].to(dt))
        return {"dw": dw}
    if c.id == "f-dgrad-planes":    # autograd's data gradient of the Conv2d, the consumed planes of it
        x = torch.zeros(c.B, 5, c.Hout, c.Wout, dtype=dt, requires_grad=True)
        (dx,) = torch.autograd.grad(F.conv2d(x, t["wconv"].to(dt), None, stride=c.stride, padding=c.pad), x, t["x"].to(dt))
        return {"y": dx[:, list(DGRAD_PLANES)]}
    src = t["x"] if c.op == "fwd" else t["contrib"]
    bias = t["bias"].to(dt) if c.bias else None
    y = F.conv_transpose2d(src.to(dt), t["w"].to(dt), bias, stride=c.stride, padding=c.pad, output_padding=c.opad)
    return {"y": _act(y, c.act, dt)}


_REF = {}


def reference(c):
    hit = _REF.get(c.id)
    if hit is None:
        t = _inputs(c)
        hit = _REF[c.id] = {"in": t, "ref": _host(c, t, torch.float64), "f32": _host(c, t, torch.float32)}
    return hit


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def w_rows(w):
    """[64,NC,R,S] -> the launches' [(r*S+s)*NC + c][64]"""
    K, NC = w.shape[:2]
    return w.reshape(K, NC, -1).permute(2, 1, 0).reshape(-1, K).contiguous().cuda()


ACT = {"none": "ACT_NONE", "leaky": "ACT_LEAKY", "tanh": "ACT_TANH"}


def strided_out(c):
    """(the [B,Hout,Wout,ostride] buffer, its first NC columns, the others)"""
    full = nan(c.B, c.Hout, c.Wout, c.ostride)
    return full, full[..., :c.NC], full[..., c.NC:]


# ----------------------------------------------------------------------------------------------------------------------
# device

@gpu
@pytest.mark.parametrize("cid", [c.id for c in FWD])
def test_forward(cid):
    ops, c = _ops(), BY_ID[cid]
    ops.reload_tuning()
    r = reference(c)
    t = r["in"]
    x, w = nhwc(t["x"]).cuda(), w_rows(t["w"])
    bias = t["bias"].cuda() if c.bias else None
    act = getattr(ops, ACT[c.act])
    assert plan_of(ops, c).name == c.plan and ops.tconv_scatter_ok(64, c.NC, c.R, c.S, c.stride)
    full, out, others = strided_out(c)
    ops.tconv_scatter(x, w, bias, full, c.B, c.H, c.W, 64, c.Hout, c.Wout, c.NC, c.ostride, c.R, c.S, c.stride, c.pad, act, 0.2)
    torch.cuda.synchronize()
    check(c, r, "y", out.permute(0, 3, 1, 2), prefix="SCATTER", cap_only=CAP_ONLY)
    assert torch.isnan(others).all().item(), f"{cid}: wrote outside its channels"
    if cid == "f-dead-tile":
        row = out[:, 32]                                        # [B, Wout, NC]: act(bias) everywhere
        assert torch.equal(row, row[:1, :1].expand_as(row)), "f-dead-tile: the tile without input pixels is not constant"
        assert torch.equal(r["ref"]["y"][:, :, 32], torch.tanh(t["bias"].double()).reshape(1, -1, 1).expand(c.B, c.NC, c.Wout))
    # the two-launch form it replaces: per-pixel tap contributions by a 1x1 GEMM, then ali_col2im
    contrib = nan(c.B, c.H, c.W, c.N)
    ops.conv_fwd(ops.geom(c.B, c.H, c.W, 64, c.H, c.W, c.N, 1, 1, 1, 0), x, w.reshape(c.N, 1, 64), contrib, ops.epilogue())
    full2, two, others2 = strided_out(c)
    ops.col2im(contrib, c.N, bias, full2, c.B, c.H, c.W, c.Hout, c.Wout, c.NC, c.ostride, c.R, c.S, c.stride, c.pad, act, 0.2)
    torch.cuda.synchronize()
    check(c, r, "y", two.permute(0, 3, 1, 2), what="y-two-launch", prefix="SCATTER", cap_only=CAP_ONLY)
    assert torch.isnan(others2).all().item(), f"{cid}: ali_col2im wrote outside its channels"
    scale = two.double().abs().max().item()
    e_pair = (out.double() - two.double()).abs().max().item()
    print(f"SCATTER case={cid} one-launch vs two-launch: {e_pair:.3e} of {scale:.3e}")
    assert e_pair <= TWO_LAUNCH_RTOL * scale, f"{cid}: the two forms differ by {e_pair:.3e} of {scale:.3e}"


def _small_operand(c, t):
    """the one-channel map as channel 1 of [B,H,W,sstride] (channel 0 of a dense one); NaN in the other channels and at
    every position no tap of any pixel reaches"""
    rows = torch.tensor(_reached(c.P, c.H, c.R, c.stride, c.pad))
    cols = torch.tensor(_reached(c.Q, c.W, c.S, c.stride, c.pad))
    g = t["small"][:, 0].clone()
    g[:, ~rows, :] = float("nan")
    g[:, :, ~cols] = float("nan")
    planes = nan(c.B, c.H, c.W, c.sstride)
    small = planes[..., 1 if c.sstride > 1 else 0]
    small.copy_(g.cuda())
    return small


def _dw_buffer(c, layout):
    """(buffer, [64,1,R,S] view of it)"""
    if layout == "pack":        # [taps][64]: the forward pack's order
        buf = nan(c.T, 64)
        return buf, torch.as_strided(buf, (64, 1, c.R, c.S), (1, c.T * 64, c.S * 64, 64))
    buf = nan(64, 1, c.R, c.S)
    return buf, buf


@gpu
@pytest.mark.parametrize("cid", [c.id for c in WGRAD])
def test_weight_gradient(cid):
    ops, c = _ops(), BY_ID[cid]
    ops.reload_tuning()
    r = reference(c)
    t = r["in"]
    big, small = nhwc(t["big"]).cuda(), _small_operand(c, t)
    assert plan_of(ops, c).name == c.plan
    runs = []
    for layout in ("own", "own", "pack"):
        buf, view = _dw_buffer(c, layout)
        got = ops.tconv_scatter_wgrad(big, small, c.sstride, view, view.stride(0), view.stride(3), c.B, c.P, c.Q, 64, c.H, c.W,
                                      c.R, c.S, c.stride, c.pad)
        assert got is view
        torch.cuda.synchronize()
        runs.append(view)
    check(c, r, "dw", runs[0], prefix="SCATTER", cap_only=CAP_ONLY)
    assert torch.equal(runs[0], runs[1]), f"{cid}: two runs differ (the reductions are fixed-order)"
    assert torch.equal(runs[0], runs[2].contiguous()), f"{cid}: the pack-order result differs from the own-layout one"
    # the slabs live behind the workspace's reserved head (the GEMM kernels' arrival counters, left at zero)
    assert not ops.workspace(torch.device("cuda"))[:WS_RESERVED].any().item()


@gpu
@pytest.mark.parametrize("cid", [c.id for c in COL2IM])
def test_col2im(cid):
    ops, c = _ops(), BY_ID[cid]
    r = reference(c)
    t = r["in"]
    contrib = nan(c.B, c.H, c.W, c.ldc)                     # the padding columns of a row must not be read
    contrib[..., :c.N] = nhwc(t["contrib"]).cuda()
    bias = t["bias"].cuda() if c.bias else None
    full, out, others = strided_out(c)
    ops.col2im(contrib, c.ldc, bias, full, c.B, c.H, c.W, c.Hout, c.Wout, c.NC, c.ostride, c.R, c.S, c.stride, c.pad,
               getattr(ops, ACT[c.act]), 0.2)
    torch.cuda.synchronize()
    check(c, r, "y", out.permute(0, 3, 1, 2), prefix="SCATTER", cap_only=CAP_ONLY)
    assert torch.isnan(others).all().item(), f"{cid}: wrote outside its channels"


@gpu
@pytest.mark.parametrize("what,q,word", REFUSED, ids=REFUSED_IDS)
def test_refusals_launch_nothing(what, q, word):
    """the launch answers ALI_ERR_BAD_ARG with the planner's message; the output keeps its NaN"""
    ops = _ops()
    ops.reload_tuning()
    op, B, H, W, C, Hout, Wout, R, S, stride, pad, NC, ostride = q
    assert ops.tconv_scatter_plan(op, B, H, W, C, Hout, Wout, R, S, stride, pad, NC=NC, ostride=ostride) is None
    lib = _lib()
    x = torch.ones(B, H, W, C, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if op == "fwd":
        w, out = torch.ones(NC * R * S, C, device="cuda"), nan(B, Hout, Wout, max(ostride, NC))
        with pytest.raises(RuntimeError, match=r"ali_tconv_scatter failed \(rc=-1\).*" + word):
            ops.tconv_scatter(x, w, None, out, B, H, W, C, Hout, Wout, NC, ostride, R, S, stride, pad)
    else:
        small, out = torch.ones(B, Hout, Wout, device="cuda"), nan(C, 1, R, S)
        assert ops.tconv_scatter_wgrad(x, small, 1, out, R * S, 1, B, H, W, C, Hout, Wout, R, S, stride, pad) is None
        ws = ops.workspace(torch.device("cuda"))
        rc = lib.ali_tconv_scatter_wgrad(x.data_ptr(), small.data_ptr(), 1, out.data_ptr(), R * S, 1, B, H, W, C, Hout, Wout,
                                         R, S, stride, pad, ws.data_ptr(), ws.numel(), stream)
        assert rc == -1 and word in _last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item()


@gpu
def test_col2im_refusals_launch_nothing():
    ops = _ops()
    out = nan(2, 6, 8, 9)
    with pytest.raises(RuntimeError, match="ali_col2im"):       # no template for 9 channels
        ops.col2im(torch.ones(2, 5, 7, 36, device="cuda"), 36, None, out, 2, 5, 7, 6, 8, 9, 9, 2, 2, 1, 0)
    with pytest.raises(RuntimeError, match="ali_col2im"):       # ldc one short of NC * R * S = 12
        ops.col2im(torch.ones(2, 5, 7, 12, device="cuda"), 11, None, out, 2, 5, 7, 6, 8, 3, 9, 2, 2, 1, 0)
    ops.col2im(torch.ones(2, 5, 7, 12, device="cuda"), 12, None, out, 2, 5, 7, 6, 8, 3, 9, 2, 2, 1, 0)      # (one more: served)
    torch.cuda.synchronize()
    assert torch.isnan(out[..., 3:]).all().item() and not torch.isnan(out[..., :3]).any().item()


@gpu
def test_weight_gradient_workspace_and_setting():
    """a workspace one byte short is ALI_ERR_WORKSPACE; under ALI_NO_T1_MFMA=1 ``ops.tconv_scatter_wgrad`` answers None;
    ``dw`` keeps its NaN both times"""
    ops, lib = _ops(), _lib()
    ops.reload_tuning()
    B, P, Q, R, S, stride, pad = 2, 9, 11, 5, 5, 2, 2
    H, W = 2 * P, 2 * Q
    big, small, dw = torch.ones(B, P, Q, 64, device="cuda"), torch.ones(B, H, W, device="cuda"), nan(64, 1, R, S)
    ws = ops.workspace(torch.device("cuda"))
    need = ops.tconv_scatter_plan("wgrad", B, P, Q, 64, H, W, R, S, stride, pad).ws
    assert need == lib.ali_tconv_scatter_wgrad_ws(B, P, Q, 64, R, S, stride) == B * 2 * 64 * 25 * 4 + WS_RESERVED <= ws.numel()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.ali_tconv_scatter_wgrad(big.data_ptr(), small.data_ptr(), 1, dw.data_ptr(), 25, 1, B, P, Q, 64, H, W, R, S, stride,
                                     pad, ws.data_ptr(), need - 1, stream)
    assert rc == -2 and "workspace too small" in _last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dw).all().item()
    with ops.tuning(**NO_MFMA):
        assert not ops.tconv_scatter_ok(64, 1, R, S, stride) and lib.ali_tconv_scatter_wgrad_ws(B, P, Q, 64, R, S, stride) == 0
        assert ops.tconv_scatter_wgrad(big, small, 1, dw, 25, 1, B, P, Q, 64, H, W, R, S, stride, pad) is None
    torch.cuda.synchronize()
    assert torch.isnan(dw).all().item()
    rc = lib.ali_tconv_scatter_wgrad(big.data_ptr(), small.data_ptr(), 1, dw.data_ptr(), 25, 1, B, P, Q, 64, H, W, R, S, stride,
                                     pad, ws.data_ptr(), need, stream)           # exactly enough: served
    torch.cuda.synchronize()
    assert rc == 0 and not torch.isnan(dw).any().item()
