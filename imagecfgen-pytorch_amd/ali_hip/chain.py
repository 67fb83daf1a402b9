"""Fused execution of an ``nn.Sequential`` conv stack on the HIP kernels.

A stack (``Encoder.layers``, ``Generator.layers``, ``Discriminator.dx/dz/dxz``;
reference image_scms/mnist.py:30-40,63-74,98-136) is parsed once into *stages*

    [Dropout2d] [BatchNorm2d] [Dropout2d]  ->  Conv2d | ConvTranspose2d | Linear(+Unflatten) | Flatten+Linear
                                           ->  LeakyReLU | ReLU | Tanh

and executed as ONE autograd node: forward runs the NHWC kernels stage by stage,
backward is hand scheduled -- the activation derivative of stage i-1 (and the
Dropout2d mask in front of stage i) is folded into the epilogue of stage i's
data-gradient GEMM, BatchNorm backward is fused with the LeakyReLU derivative.
Which kernel serves a stage -- forward, weight gradient, data gradient -- is decided in one place (``route``).
The ``nn`` modules only own the parameters (reference layouts, reference
``state_dict`` keys); their own ``forward`` is never called on CUDA tensors.
"""
import weakref
from collections import namedtuple
from typing import List, Optional

import torch
import torch.nn as nn

from . import dropout as _dropout
from . import ops
from .ops import ACT_LEAKY, ACT_NONE, ACT_TANH


def _pad4(c: int) -> int:
    return (c + 3) // 4 * 4


class Stage:
    """One convolution (or Linear) of the stack with what sits in front of it (``pre``: ("drop", p) / ("bn", module)
    in module order; ``pattern``: their kinds) and the activation behind it."""
    __slots__ = ("kind", "mod", "act", "slope", "pre", "pattern", "has_drop", "drop_p", "bn", "unflat", "index", "hw")

    def __init__(self, kind, mod, pre, index):
        self.kind, self.mod, self.pre, self.index = kind, mod, pre, index
        self.act, self.slope, self.unflat = ACT_NONE, 0.0, None
        self.hw = None       # kind "flat": the map the Flatten sees, known at the first forward (``resolve_flat``)
        self.pattern = [k for k, _ in pre]
        self.has_drop = "drop" in self.pattern
        self.drop_p = next((a for k, a in pre if k == "drop"), None)
        self.bn = next((a for k, a in pre if k == "bn"), None)


class PackCache:
    """Kernel-layout copies of one parameter (the reference layouts stay the master copies: Conv
    [Cout,Cin,kh,kw], ConvT [Cin,Cout,kh,kw], Linear [out,in]).

    A copy is rebuilt when the parameter's version / storage changed since it was built (``load_state_dict``, a
    ``torch.optim`` step, any in-place edit bumps the version).  Static mode (AliStepper, graph capture): the rebuild
    happens IN PLACE so buffers keep their addresses, and ``refresh()`` rewrites every copy right after the optimiser
    kernel that changed the parameters (that kernel works on raw pointers and does not bump versions)."""

    def __init__(self):
        self.store = {}
        self.static = False

    def make_static(self):
        """from here on copies are rebuilt in place (the parameters were just re-pointed: what was built is dropped)"""
        self.store.clear()
        self.static = True

    @staticmethod
    def _tag(param):
        return (param.data_ptr(), param._version, tuple(param.shape))

    def get(self, key, param: torch.Tensor, builder):
        hit = self.store.get(key)
        tag = self._tag(param)
        if hit is not None and hit[0] == tag:
            return hit[1]
        with torch.no_grad():
            val = builder(hit[1] if (hit is not None and self.static) else None)
            ops.after_packs(lambda v=val: ops.refresh_shadow16(v))   # the fp16 twin (precision "f16"), if it has one
        self.store[key] = (tag, val, builder, param)
        return val

    def refresh(self):
        with torch.no_grad():
            for key, (tag, val, builder, param) in list(self.store.items()):
                out = builder(val)
                assert out.data_ptr() == val.data_ptr()
                ops.after_packs(lambda v=val: ops.refresh_shadow16(v))
                self.store[key] = (self._tag(param), val, builder, param)


def _refuse(i: int, m, why: str):
    raise NotImplementedError(f"ali_hip.chain: layer {i} ({m.__class__.__name__}): {why}")


def _check_layer(i: int, m):
    """Refuses, at plan construction, every setting of layer ``i`` that the stages cannot represent: they carry one
    stride / padding / output padding per convolution (``stride[0]`` ...), dense undilated zero-padded kernels, an
    affine BatchNorm with a fixed momentum, an Unflatten of dim 1 and a Dropout2d that keeps something."""
    if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        if isinstance(m.padding, str):
            _refuse(i, m, f"padding={m.padding!r} (only explicit integer padding)")
        for name in ("stride", "padding") + (("output_padding",) if isinstance(m, nn.ConvTranspose2d) else ()):
            v = tuple(getattr(m, name))
            if len(set(v)) != 1:
                _refuse(i, m, f"{name}={v} (both entries must be equal)")
        if tuple(m.dilation) != (1, 1):
            _refuse(i, m, f"dilation={tuple(m.dilation)} (only 1)")
        if m.groups != 1:
            _refuse(i, m, f"groups={m.groups} (only 1)")
        if m.padding_mode != "zeros":
            _refuse(i, m, f"padding_mode={m.padding_mode!r} (only 'zeros')")
    elif isinstance(m, nn.BatchNorm2d):
        if m.momentum is None:
            _refuse(i, m, "momentum=None (the cumulative moving average is not implemented)")
        if not m.affine:
            _refuse(i, m, "affine=False (the kernels read a weight and a bias)")
    elif isinstance(m, nn.Unflatten):
        if m.dim != 1:
            _refuse(i, m, f"dim={m.dim} (only dim=1)")
    elif isinstance(m, nn.Dropout2d) or m.__class__.__name__ in ("Dropout2d", "TapedDropout2d"):
        if not 0.0 <= float(m.p) < 1.0:
            _refuse(i, m, f"p={m.p} (outside [0, 1))")


class ChainPlan:
    def __init__(self, seq: nn.Sequential):
        self.seq = weakref.ref(seq)          # the plan lives in a WeakKeyDictionary keyed by seq: no strong cycle
        self.stages: List[Stage] = []
        self.cache = PackCache()
        pre = []
        mods = list(seq)
        for i, m in enumerate(mods):
            _check_layer(i, m)
        i = 0
        flat = False          # an nn.Flatten() was seen: the Linear behind it is a "flat" stage
        while i < len(mods):
            m = mods[i]
            name = m.__class__.__name__
            if flat and not isinstance(m, nn.Linear):
                raise NotImplementedError("ali_hip.chain: unsupported layer Flatten (only in front of a Linear)")
            if isinstance(m, nn.Dropout2d) or name in ("Dropout2d", "TapedDropout2d"):
                pre.append(("drop", float(m.p)))
            elif isinstance(m, nn.BatchNorm2d):
                pre.append(("bn", m))
            elif isinstance(m, nn.Flatten):
                # Flatten -> Linear(C*h*w, O) on an NHWC [B,h,w,C] map: an unpadded stride-1 Conv2d(C, O, (h, w)) whose
                # weight is the Linear's [O, C*h*w] storage viewed as [O, C, h, w] (classifiers/mnist.py:21-22)
                if (m.start_dim, m.end_dim) != (1, -1):
                    raise NotImplementedError("ali_hip.chain: unsupported layer Flatten (start_dim / end_dim not 1 / -1)")
                flat = True
            elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
                kind = "convT" if isinstance(m, nn.ConvTranspose2d) else ("conv" if isinstance(m, nn.Conv2d)
                                                                          else "flat" if flat else "linear")
                flat = False
                st = Stage(kind, m, pre, len(self.stages))
                pre = []
                if kind == "linear" and i + 1 < len(mods) and isinstance(mods[i + 1], nn.Unflatten):
                    st.unflat = tuple(mods[i + 1].unflattened_size)
                    i += 1
                if i + 1 < len(mods) and isinstance(mods[i + 1], nn.LeakyReLU):
                    st.act, st.slope = ACT_LEAKY, float(mods[i + 1].negative_slope)
                    i += 1
                elif i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
                    # LeakyReLU with slope 0: max(v, 0) forward, y > 0 ? 1 : 0 backward (0 at exactly 0, as torch's)
                    st.act, st.slope = ACT_LEAKY, 0.0
                    i += 1
                elif i + 1 < len(mods) and isinstance(mods[i + 1], nn.Tanh):
                    st.act = ACT_TANH
                    i += 1
                self.stages.append(st)
            else:
                raise NotImplementedError(f"ali_hip.chain: unsupported layer {name}")
            i += 1
        if flat:
            raise NotImplementedError("ali_hip.chain: unsupported layer Flatten (no Linear behind it)")
        if pre:
            raise NotImplementedError("trailing Dropout2d/BatchNorm2d without a convolution")
        for st in self.stages:
            if st.pattern not in ([], ["drop"], ["bn"], ["drop", "bn"], ["bn", "drop"]):
                raise NotImplementedError(f"unsupported pre-op pattern {st.pattern}")

    @property
    def out_channels(self) -> int:
        """channels of the last stage's output"""
        return _out_shape(self.stages[-1], 1, 1, 1, 1)[3]

    def params(self) -> List[torch.Tensor]:
        out = []
        for st in self.stages:
            if st.bn is not None:
                out += [st.bn.weight, st.bn.bias]
            out.append(st.mod.weight)
            if st.mod.bias is not None:
                out.append(st.mod.bias)
        return out

    # ------------------------------------------------------------------ packing
    def packed(self, st: Stage, which, cin_stride: int):
        """which = 'fwd' | 'dgrad' kernel-layout weights of a stage (see include/ali_hip.h); 'scatter' and
        ('scatter_dgrad', planes): the 1x1 GEMM weights of the scatter-form transposed convolutions (ali_col2im)."""
        w = st.mod.weight
        dev = w.device
        hw = st.hw

        def build(dst=None):
            def buf(*shape, zero=False):
                if dst is not None:
                    return dst.reshape(shape)
                return (torch.zeros if zero else torch.empty)(*shape, device=dev)
            if which == "scatter":            # ConvT [Ci][Co][R][S] -> rows n = tap*Co + co, columns ci (pad: 0)
                Ci, Co, R, S = w.shape
                out = buf(R * S * Co, 1, cin_stride, zero=True)
                # as a pack: "row" tap, "tap" co, channel ci -- joins the batched re-pack launch of an optimiser step
                ops.pack_weights(w.detach(), out, R * S, Co, Ci, cin_stride, 1, R * S, Co * R * S)
                return out
            if isinstance(which, tuple) and which[0] == "scatter_dgrad":   # Conv [K][C][R][S] -> rows tap*NP + j, cols k
                K, C, R, S = w.shape
                if len(which[1]) == 1:        # one plane: rows = taps, channel k; source = the plane's [K][.][R][S] slice
                    out = buf(R * S, 1, K)
                    src = w.detach().reshape(-1)[which[1][0] * R * S:]
                    ops.pack_weights(src, out, R * S, 1, K, K, 1, 0, C * R * S)
                    return out
                sel = torch.stack([w.detach()[:, c] for c in which[1]], dim=0)          # [NP][K][R][S], slices only
                out = buf(R * S * len(which[1]), 1, K)
                out[:, 0, :].copy_(sel.permute(2, 3, 0, 1).reshape(R * S * len(which[1]), K))
                return out
            if st.kind == "flat":             # the Linear's [O][C*h*w] storage read as a Conv2d weight [O][C][h][w]
                O, T = w.shape[0], hw[0] * hw[1]
                C = w.shape[1] // T
                if T > FLAT_TAPS:             # a 1x1 GEMM over T*C channels: [O][1][T*C] and its transpose [T*C][1][O]
                    if which == "fwd":        # (the same permutation as below; cin_stride == T*C: nothing is padded)
                        return ops.pack_weights(w.detach(), buf(O, 1, T * C), O, T, C, C, C * T, 1, T)
                    return ops.pack_weights(w.detach(), buf(T * C, 1, O), T, C, O, O, 1, T, C * T)
                if which == "fwd":            # [O][T][Cpad]
                    return ops.pack_weights(w.detach(), buf(O, T, cin_stride), O, T, C, cin_stride, C * T, 1, T)
                out = buf(cin_stride, T, O, zero=True)             # [Cpad][T][O]; rows >= C stay zero
                ops.pack_weights(w.detach(), out, C, T, O, O, T, 1, C * T)
                return out
            if w.dim() == 4:
                src = _storage_view(w)     # (weights may live in the forward pack's order already: FlatGroup.layouts)
                s0, s1, _, s3 = w.stride()
            if st.kind == "conv":
                K, C, R, S = w.shape
                T = R * S
                if which == "fwd":      # [K][T][Cpad]
                    return ops.pack_weights(src, buf(K, T, cin_stride), K, T, C, cin_stride, s0, s3, s1)
                out = buf(cin_stride, T, K, zero=True)             # [Cpad][T][K]; rows >= C stay zero
                ops.pack_weights(src, out, C, T, K, K, s1, s3, s0)
                return out
            if st.kind == "convT":
                Ci, Co, R, S = w.shape
                T = R * S
                if which == "fwd":      # convT forward == data-gradient GEMM: [Co][T][Ci_pad]
                    return ops.pack_weights(src, buf(Co, T, cin_stride), Co, T, Ci, cin_stride, s1, s3, s0)
                # convT dgrad == conv forward GEMM: [Ci_pad][T][Co]; rows >= Ci stay zero
                out = buf(cin_stride, T, Co, zero=True)
                ops.pack_weights(src, out, Ci, T, Co, Co, s0, s3, s1)
                return out
            # linear (+Unflatten(C,h,w)): 1x1 conv whose output channel n' = t*C + co is NHWC [B,h,w,C]
            O, I = w.shape
            Cc, hh, ww = st.unflat if st.unflat else (O, 1, 1)
            T = hh * ww
            if which == "fwd":
                return ops.pack_weights(w.detach(), buf(O, 1, cin_stride), T, Cc, I, cin_stride, I, T * I, 1)
            fwd = self.packed(st, "fwd", cin_stride)
            out = buf(cin_stride, 1, O, zero=True)                 # [I_pad][1][O] = transpose of the fwd pack
            ops.pack_weights(fwd, out, I, 1, O, O, 1, 0, cin_stride)
            return out

        twin = getattr(w, "_ali_flat16", None)
        if which == "fwd" and (not ops._PRECISION["f16"] or twin is not None) and w.dim() == 4 \
                and tuple(w.stride()) == _fwd_pack_strides(st) \
                and cin_stride == (w.shape[1] if st.kind == "conv" else w.shape[0]):
            # the master weights ARE the forward pack (FlatGroup.layouts): no copy to refresh.  fp16-MFMA path: the Adam
            # launch keeps an fp16 twin of the flat parameter buffer (FlatGroup.flat16); its segment is the pack's twin
            n_out = w.shape[0] if st.kind == "conv" else w.shape[1]
            alias = _storage_view(w).view(n_out, w.shape[2] * w.shape[3], cin_stride)
            if ops._PRECISION["f16"]:
                alias._ali16 = twin.view(n_out, w.shape[2] * w.shape[3], cin_stride)
            return alias
        val = self.cache.get((st.index, which, cin_stride) + ((hw,) if st.kind == "flat" else ()), w, build)
        if ops._PRECISION["f16"] and which in ("fwd", "dgrad"):
            with torch.no_grad():
                ops.ensure_shadow16(val)         # fp16 twin of the packed weights, re-rounded whenever they are re-packed
        return val

    def packed_bias(self, st: Stage):
        b = st.mod.bias
        if b is None:
            return None
        if st.kind != "linear" or not st.unflat:
            return b.detach()
        Cc, hh, ww = st.unflat
        def build(dst=None):
            val = b.detach().reshape(Cc, hh * ww).t().contiguous().reshape(-1)
            if dst is not None:
                dst.copy_(val)
                return dst
            return val
        return self.cache.get((st.index, "bias"), b, build)


# ---------------------------------------------------------------------- shapes
def _out_shape(st: Stage, B, H, W, C):
    m = st.mod
    if st.kind == "conv":
        R, S = m.kernel_size
        s, p = m.stride[0], m.padding[0]
        return B, (H + 2 * p - R) // s + 1, (W + 2 * p - S) // s + 1, m.out_channels
    if st.kind == "convT":
        R, S = m.kernel_size
        s, p, op = m.stride[0], m.padding[0], m.output_padding[0]
        return B, (H - 1) * s - 2 * p + R + op, (W - 1) * s - 2 * p + S + op, m.out_channels
    if st.unflat:
        Cc, hh, ww = st.unflat
        return B, hh, ww, Cc
    return B, 1, 1, m.out_features       # Linear, and Flatten + Linear: the whole map is the kernel


FLAT_TAPS = 28      # the conv kernels take at most 28 taps (csrc/ali_common.h: kMaxTaps)


def flat_gemm(st: Stage) -> bool:
    """A Flatten + Linear on a map of more than ``FLAT_TAPS`` positions: the NHWC map [B,h,w,C] (unpadded) already is
    the row [B,1,1,h*w*C], so the stage runs as a 1x1 GEMM over h*w*C input channels on weights permuted to that
    order (train_morphomnist_ae.py:23-24, a 7 x 7 map)."""
    return st.kind == "flat" and st.hw is not None and st.hw[0] * st.hw[1] > FLAT_TAPS


def resolve_flat(st: Stage, in_shape, c_log: int):
    """A "flat" stage meets its input map [B,h,w,Cp] with ``c_log`` real channels: fixes ``st.hw`` (it decides the
    weight view and the packs) or raises when the Linear was built for another map."""
    _, H, W, _ = in_shape
    if st.mod.in_features != c_log * H * W:
        raise ValueError(f"ali_hip.chain: Flatten + Linear(in_features={st.mod.in_features}) on a {c_log} x {H} x {W} "
                         f"map ({c_log * H * W} features)")
    if H * W > FLAT_TAPS and (in_shape[3] != c_log or st.pre):
        # (read as one row, the map has no channel axis left for padding, a Dropout2d mask or BatchNorm statistics)
        raise NotImplementedError(f"ali_hip.chain: Flatten of a {H} x {W} map with padded channels ({c_log} of "
                                  f"{in_shape[3]}) or pre-ops {st.pattern}: a map of more than {FLAT_TAPS} positions "
                                  f"is read as one row")
    st.hw = (H, W)


def trace(plan: "ChainPlan", in_shape, c_log: int):
    """[(input shape, output shape, Route)] of every stage for an NHWC input ``in_shape`` with ``c_log`` real channels
    (no tensors, no device: what ``chain_forward_gen`` will decide)."""
    out = []
    cur = tuple(in_shape)
    for st in plan.stages:
        if st.kind == "flat":
            resolve_flat(st, cur, c_log)
        nxt = _out_shape(st, *cur)
        out.append((cur, nxt, route(st, cur, c_log)))
        cur, c_log = nxt, nxt[3]
    return out


def _geom(st: Stage, xin_shape, out_shape):
    """AliConvGeom of the stage's equivalent Conv2d (ConvT: roles of x / y swapped)."""
    B, H, W, C = xin_shape
    _, P, Q, K = out_shape
    m = st.mod
    if st.kind == "conv":
        return ops.geom(B, H, W, C, P, Q, K, m.kernel_size[0], m.kernel_size[1], m.stride[0], m.padding[0])
    if st.kind == "convT":   # x := convT output, y := convT input
        return ops.geom(B, P, Q, K, H, W, C, m.kernel_size[0], m.kernel_size[1], m.stride[0], m.padding[0])
    if flat_gemm(st):        # the whole map is one row of H*W*C channels
        return ops.geom(B, 1, 1, H * W * C, 1, 1, K, 1, 1, 1, 0)
    if st.kind == "flat":    # the (H, W) kernel covers the map once
        return ops.geom(B, H, W, C, 1, 1, K, H, W, 1, 0)
    # linear: 1x1 conv on the [B,1,1,I] map with O output channels
    return ops.geom(B, 1, 1, C, 1, 1, P * Q * K, 1, 1, 1, 0)


class Route(namedtuple("Route", "fwd wgrad wgrad_fold dgrad planes fold_ok bn_leave bn_reduce")):
    """Which kernels serve one stage: decided once by ``route`` from the stage, its input shape and its logical input
    channels, saved by the forward pass and read by the backward pass.  What only a call knows (a mask that was folded,
    a FoldQueue, strided or non-contiguous operands, the workspace size) stays at the call, once per fact.

    fwd         "head" (GEMV) | "tconv1" (direct one-channel kernel) | "scatter" (scatter form, one launch) |
                "scatter_gemm" (1x1 GEMM + col2im) | "convT" | "conv" (implicit GEMMs; a Linear is a 1x1 "conv", a
                Flatten + Linear an (h, w) "conv" on all three passes) | "flat_gemm" (Flatten + Linear on a map of more
                than 28 positions: a 1x1 "conv" over h*w*C channels, ``flat_gemm``; also its ``dgrad``).  Only
                the GEMMs have an epilogue: a "head" / "scatter*" stage that has to fold the next stage's mask or leave
                BatchNorm partials runs the GEMM of its kind instead.
    wgrad       (weight-gradient path, bias-gradient path): "head" | "first_direct" (ali_tconv1_wgrad over the <= 8
                input planes) | "conv" | "tconv1" | "convT_scatter" (pixel contraction; the GEMM when the operands or
                the workspace do not allow it) | "convT" | "linear" | "linear_repack" | "flat_repack" (computed in the
                "flat_gemm" pack's order, re-packed into the Linear's own layout right away); the bias gradient is "fused"
                into that launch, a "colsum" of its own, the "unflat" column sum in Unflatten order, or None (no bias).
    wgrad_fold  the same when the launches are deferred to a FoldQueue: a "first_direct" stage with 4-aligned channels
                then rides the pass's combined weight-gradient launch as one more GEMM job (its 200 x 32 GEMM fills gaps
                there and the bias gradient comes along: measured 7.15 -> 7.08 ms per MNIST iteration).
    dgrad       "tconv1" (direct; the "convT" GEMM when a mask or BatchNorm sits in front) | "convT" | "conv"
    planes      first stage asked for a few input planes only (``gx_planes``): "direct" (one ali_tconv1_fwd per plane) |
                "scatter" (scatter form, when the plane count allows it: ``_plane_grads``) | None (full data gradient)
    fold_ok     the forward may apply a lone Dropout2d mask of the next stage in its epilogue
    bn_leave    the forward GEMM may leave the partial sums of a BatchNorm behind it
    bn_reduce   the data-gradient GEMM may leave the partial sums of the BatchNorm backward in front of it"""


def route(st: Stage, in_shape, c_log: int) -> Route:
    """The stage's Route for an input [B,H,W,Cp] = ``in_shape`` with ``c_log`` real channels (B does not matter)."""
    m, Cp = st.mod, in_shape[3]
    taps = (1 if st.kind == "linear" else in_shape[1] * in_shape[2] if st.kind == "flat"
            else m.kernel_size[0] * m.kernel_size[1])
    if st.kind == "flat" and taps > FLAT_TAPS:
        return Route("flat_gemm", ("flat_repack", None if m.bias is None else "colsum"),
                     ("flat_repack", None if m.bias is None else "colsum"), dgrad="flat_gemm", planes=None,
                     fold_ok=st.act in (ACT_NONE, ACT_LEAKY), bn_leave=False, bn_reduce=False)
    # ConvTranspose2d(C -> 1), stride 1, no output padding: served by the direct one-channel kernels -- when all three
    # of them take the shape (ops.tconv1_route: the launches' own plan; e.g. no 128 channels x 16 taps, whose weight
    # gradient needs more accumulators than a thread has, and no rectangular kernel, which the forward refuses)
    tconv1 = (st.kind == "convT" and m.out_channels == 1 and m.stride[0] == 1 and m.output_padding[0] == 0
              and m.kernel_size[0] <= 5 and Cp in (32, 64, 128, 256))
    if tconv1:
        big = (in_shape[0], in_shape[1], in_shape[2], Cp, *m.kernel_size, m.padding[0])
        tconv1 = all(ops.tconv1_route(op, *big) is not None for op in ("fwd", "dgrad", "wgrad"))
    # first Conv2d of a stack (<= 8 real input channels, stride 1): per-channel direct weight gradient (ali_tconv1_wgrad
    # with the output gradient as the many-channel map) and single-plane data gradient (ali_tconv1_fwd), each when
    # its launch takes the shape
    first_direct = first_planes = (st.index == 0 and st.kind == "conv" and m.stride[0] == 1 and c_log <= 8
                                   and m.out_channels in (32, 64, 128, 256) and m.kernel_size[0] <= 5)
    if first_direct:
        (R, S), pad = m.kernel_size, m.padding[0]
        big = (in_shape[0], in_shape[1] + 2 * pad - R + 1, in_shape[2] + 2 * pad - S + 1, m.out_channels, R, S, pad)
        first_direct = ops.tconv1_route("wgrad", *big, nc=c_log) is not None
        first_planes = ops.tconv1_route("fwd", *big) is not None
    gemm = "convT" if st.kind == "convT" else "conv"
    if (st.kind == "conv" and m.out_channels == 1 and taps == 1 and m.stride[0] == 1 and m.padding[0] == 0
            and tuple(in_shape[1:3]) == (1, 1) and Cp % 4 == 0 and st.act == ACT_NONE):
        fwd = "head"      # Conv2d(C, 1, 1) on a 1x1 map without activation (the Discriminator's last layer, mnist.py:127)
    elif tconv1:          # (the register-blocked tconv1_fwd beats the scatter form on the MNIST tail by 17 us per launch)
        fwd = "tconv1"
    elif st.kind == "convT" and m.out_channels <= 2 and m.out_channels * taps <= 64 and Cp % 4 == 0:
        # one or two output channels that the direct kernels do not cover (stride 2 Generator tails of the spectrogram
        # models): per-input-pixel tap contributions by a 1x1 GEMM with N = Cout*R*S columns, then ali_col2im -- an
        # implicit GEMM over the output pixels would use 1/32 of every MFMA tile -- or, contributions kept in LDS per
        # output tile, one launch and no [pixels][taps] tensor
        fwd = "scatter" if ops.tconv_scatter_ok(Cp, m.out_channels, *m.kernel_size, m.stride[0]) else "scatter_gemm"
    else:
        fwd = gemm
    bias = None if m.bias is None else "colsum"
    if st.kind == "linear":
        wgrad = ("linear" if not st.unflat or st.unflat[1] * st.unflat[2] == 1 else "linear_repack",
                 bias and ("unflat" if st.unflat else "colsum"))
    elif st.kind == "convT":      # (one-channel stride-2 tail of 64 channels: ali_tconv_scatter_wgrad)
        wgrad = ("tconv1" if tconv1 else "convT_scatter" if (m.out_channels, Cp, c_log) == (1, 64, 64) else "convT", bias)
    else:   # Conv2d: the bias gradient is the column sum of the dense wgrad operand -> fused into that launch
        wgrad = ("head" if fwd == "head" else "conv", bias and "fused")
    wgrad_fold = wgrad
    if first_direct:
        wgrad = ("first_direct", bias)
        if Cp % 4 != 0:                   # (no GEMM job for the combined launch either)
            wgrad_fold = wgrad
    planes = None
    if st.index == 0 and st.bn is None and st.kind == "conv":
        planes = "direct" if first_planes else "scatter" if m.out_channels % 4 == 0 else None
    return Route(fwd, wgrad, wgrad_fold, dgrad="tconv1" if tconv1 else gemm, planes=planes,
                 fold_ok=st.kind != "linear" and st.act in (ACT_NONE, ACT_LEAKY) and not tconv1,
                 bn_leave=st.kind == "conv", bn_reduce=st.kind != "linear" and not tconv1)


_NBT = {"pending": None}


def _count_batch(bn):
    """num_batches_tracked += 1 (nn.BatchNorm2d training forward).  Inside a stepper iteration the increments are
    collected and applied by one multi-tensor launch (``flush_batch_counts``) instead of one launch per forward."""
    pend = _NBT["pending"]
    if pend is None:
        bn.num_batches_tracked += 1
    else:
        ent = pend.setdefault(id(bn), [bn.num_batches_tracked, 0])
        ent[1] += 1


def defer_batch_counts():
    _NBT["pending"] = {}


def drop_pending_batch_counts():
    if _NBT["pending"] is not None:
        _NBT["pending"] = {}


def abort_batch_counts():
    _NBT["pending"] = None


def flush_batch_counts(extra=()):
    """apply the collected num_batches_tracked increments (+ ``extra`` = [(int64 counter tensor, increment), ...]) in
    one launch"""
    pend, _NBT["pending"] = _NBT["pending"], None
    jobs = [(e[0], e[1]) for e in (pend or {}).values()] + list(extra)
    cuda = [(t, k) for t, k in jobs if t.is_cuda]
    for t, k in jobs:
        if not t.is_cuda:
            t += k
    if cuda:
        ops.add_i64_multi([t.reshape(1) if t.dim() == 0 else t for t, _ in cuda], [k for _, k in cuda])


class _Saved:
    """what the forward pass keeps of one stage for the backward pass"""
    __slots__ = ("x_in", "t", "y", "mask", "bn_stats", "bn", "pattern", "geom", "route", "c_log", "in_shape", "out_shape",
                 "training")


def slice_saved(saved, group: int, groups: int):
    """The saved state of one of the ``groups`` passes that ``chain_forward(..., groups=...)`` ran as one batch
    (contiguous row ranges of every activation, that pass's BatchNorm statistics)."""
    out = []
    for sv in saved:
        B = sv.in_shape[0] // groups
        lo, hi = group * B, (group + 1) * B
        s2 = _Saved()
        s2.x_in, s2.t, s2.y = sv.x_in[lo:hi], sv.t[lo:hi], sv.y[lo:hi]
        s2.mask = None if sv.mask is None else sv.mask[lo:hi]
        s2.bn, s2.pattern, s2.training, s2.route, s2.c_log = sv.bn, sv.pattern, sv.training, sv.route, sv.c_log
        s2.bn_stats = None if sv.bn_stats is None else (sv.bn_stats[group] if isinstance(sv.bn_stats, list)
                                                        else sv.bn_stats)
        s2.in_shape, s2.out_shape = (B,) + tuple(sv.in_shape[1:]), (B,) + tuple(sv.out_shape[1:])
        g = sv.geom
        s2.geom = ops.geom(B, g.H, g.W, g.C, g.P, g.Q, g.K, g.R, g.S, g.stride, g.pad)
        out.append(s2)
    return out


def _fwd_pack_strides(st: Stage):
    """Strides that make a 4-d conv weight's storage order the forward GEMM's pack ([N][R*S][Cin]: for a Conv2d weight
    torch's channels_last), or None when the stage's forward pack is not a permutation of the weight (padded input
    channels, one-channel / scatter tails, Linear)."""
    w = st.mod.weight
    if w.dim() != 4 or st.index == 0:      # (first layers: padded planes, direct / scatter kernels with their own packs)
        return None
    if st.kind == "conv":
        K, C, R, S = w.shape
        return (R * S * C, 1, S * C, C) if C % 4 == 0 else None
    if st.kind == "convT":
        Ci, Co, R, S = w.shape
        if Ci % 32 != 0 or route(st, (1, 1, 1, Ci), Ci).fwd != "convT":     # (H, W do not decide whether it is the GEMM)
            return None
        return (1, R * S * Ci, S * Ci, Ci)
    return None


def pack_layouts(plans):
    """{id(weight): strides} for FlatGroup(layouts=...): every conv weight whose forward pack is a permutation of it"""
    out = {}
    for pl in plans:
        for st in pl.stages:
            strides = _fwd_pack_strides(st)
            if strides is not None:
                out[id(st.mod.weight)] = strides
    return out


def _storage_view(w):
    """the dense storage range of a (possibly permuted) parameter as a contiguous 1-d tensor"""
    return torch.as_strided(w.detach(), (w.numel(),), (1,))


def join_ok(plan: ChainPlan) -> bool:
    """Can the chain's last stage write its output straight into a column range of a wider row-major buffer
    (``chain_forward(join=...)``) and take its output gradient from one (``chain_backward(gy_ld=...)``)?  A plain
    Conv2d GEMM ending in no activation / LeakyReLU (the ends of D.dx and D.dz, mnist.py:116-123)."""
    st = plan.stages[-1]
    return (len(plan.stages) > 1 and st.kind == "conv" and st.act in (ACT_NONE, ACT_LEAKY)
            and st.mod.out_channels % 4 == 0 and st.mod.in_channels % 4 == 0)


def drive(gen):
    """run a chain generator to its end on its own (every GEMM is launched where it is requested)"""
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


def run_parallel(*gens):
    """Advance independent chain generators in lock step, one GEMM each per round, and issue the GEMMs of a round as
    ONE multi-job launch per kernel variant (``ops.gemm_batch``).  A chain generator (``chain_forward_gen``,
    ``chain_backward_gen``, or a generator that ``yield from``-s several of them) yields right after each GEMM request
    and before anything that reads its result, so whatever else it launches between two yields only depends on GEMMs
    of earlier rounds.  The generators must not depend on each other.  Returns their return values."""
    res = [None] * len(gens)
    live = list(range(len(gens)))
    while live:
        nxt = []
        with ops.gemm_batch():
            for i in live:
                try:
                    next(gens[i])
                    nxt.append(i)
                except StopIteration as e:
                    res[i] = e.value
        live = nxt
    return res


def delayed(gen, rounds: int):
    """``gen`` entering ``run_parallel`` ``rounds`` rounds late (pairs a short chain's GEMMs with later, larger layers of
    its partner instead of with the partner's first one)"""
    for _ in range(rounds):
        yield
    return (yield from gen)


def chain_forward(*args, **kwargs):
    """``chain_forward_gen`` run on its own: returns (y_last, saved list)."""
    return drive(chain_forward_gen(*args, **kwargs))


def chain_backward(*args, **kwargs):
    """``chain_backward_gen`` run on its own: returns (gx or None, {param tensor id -> grad})."""
    return drive(chain_backward_gen(*args, **kwargs))


def _pre_ops(st: Stage, sv, bn_part, mask_applied: bool, groups: int):
    """What sits in front of the stage's convolution: the Dropout2d mask ``sv.mask`` (unless the producer applied it)
    and / or BatchNorm -- batch statistics from the partial sums ``bn_part`` = (partials, slots) the producing conv
    left behind, else by a pass of their own.  Sets ``sv.bn_stats`` and returns the convolution's input."""
    cur, mask, bn = sv.x_in, sv.mask, st.bn
    B, H, W, Cp = sv.in_shape
    rows = H * W
    sv.bn_stats = None
    if bn is None:
        return ops.rowmask_mul(cur, mask, B, rows, Cp) if (mask is not None and not mask_applied) else cur
    mask_in = mask if st.pattern == ["drop", "bn"] else None
    mask_post = mask if st.pattern == ["bn", "drop"] else None
    use_batch = sv.training or bn.running_mean is None
    momentum = bn.momentum          # (never None: ChainPlan refuses the cumulative average)
    if bn_part is not None:
        stg = ops.bn_stats_from_partials(bn_part[0], bn_part[1], groups, Cp, (B // groups) * rows, bn.weight.detach(),
                                         bn.bias.detach(), bn.running_mean, bn.running_var, momentum, bn.eps)
    else:                       # per-pass statistics / running-stat updates, one launch for all passes
        stg = ops.bn_stats(cur, mask_in, B, rows, Cp, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                           bn.running_var, momentum, bn.eps, use_batch, groups=groups)
    if use_batch and bn.num_batches_tracked is not None:
        for _ in range(groups):
            _count_batch(bn)
    sv.bn_stats = stg if groups == 1 else [stg[gi] for gi in range(groups)]
    return ops.bn_apply(cur, stg, mask_in, mask_post, B, rows, Cp, groups=groups)


def _for_next_stage(nxt: Stage, sv, groups: int, lane):
    """What this stage's GEMM epilogue does for the pre-ops of the next stage: (folded, early, bn_fwd).
    ``folded``: a lone Dropout2d in front of the next stage multiplies this stage's output by a per-(sample, channel)
    mask: the GEMM epilogue does it (act(.)*mask), so y is stored masked.  LeakyReLU'(y) only needs the sign of y,
    which the kept entries preserve and the dropped ones do not need (their gradient is masked to 0).
    ``bn_fwd``: the batch statistics of a BatchNorm behind this conv are column sums of this stage's output --
    accumulated per M-tile by the GEMM epilogue (times the Dropout2d mask ``early`` that may sit in between, which is
    drawn here for that), no extra pass."""
    B, P, Q, K = sv.out_shape
    draw = lambda: _dropout.next_mask(B, K, nxt.drop_p, sv.x_in.device, K, lane=lane)      # noqa: E731
    if sv.training and nxt.pattern == ["drop"] and sv.route.fold_ok:
        return draw(), None, None
    early = bn_fwd = None
    if nxt.bn is not None and sv.route.bn_leave and (sv.training or nxt.bn.running_mean is None):
        if sv.training and nxt.pattern == ["drop", "bn"]:
            early = draw()
        slots, tile_rows, pixel_major = ops.conv_mtiles(sv.geom, 0)
        rows_g = (B // groups) * (1 if pixel_major else P * Q)
        if slots > 0 and (groups == 1 or (B % groups == 0 and rows_g % tile_rows == 0
                                          and (not pixel_major or B % tile_rows == 0))):
            part = torch.empty(2 * K * slots, dtype=torch.float32, device=sv.x_in.device)
            bn_fwd = (part, groups, early, slots)
    return None, early, bn_fwd


def _launch_fwd(plan: ChainPlan, st: Stage, sv, folded, bn_fwd, out_ld: int, jmask, alloc):
    """The stage's convolution sv.t -> sv.y on the kernel of its route (generator: yields after a GEMM request)."""
    t, y, m, c_log = sv.t, sv.y, st.mod, sv.c_log
    B, H, W, Cp = sv.in_shape
    _, P, Q, K = sv.out_shape
    bias = plan.packed_bias(st)
    path = sv.route.fwd
    if path in ("head", "scatter", "scatter_gemm") and (folded is not None or bn_fwd is not None):
        path = st.kind                    # these kernels have no epilogue: the GEMM of the stage's kind does the work
    if path == "scatter" and not t.is_contiguous():
        path = "scatter_gemm"
    if path == "head":                    # (never the end of a join: join_ok needs K % 4 == 0, so out_ld == 0)
        ops.head_fwd(t.reshape(B, Cp), plan.packed(st, "fwd", Cp).reshape(-1), bias, y.reshape(B))
    elif path == "tconv1":
        ops.tconv1_fwd(t, plan.packed(st, "fwd", Cp), bias, y, B, H, W, Cp, m.kernel_size[0], m.kernel_size[1],
                       m.padding[0], 1, st.act, st.slope)
    elif path == "scatter":
        ops.tconv_scatter(t, plan.packed(st, "scatter", Cp), bias, y, B, H, W, Cp, P, Q, K, K, *m.kernel_size,
                          m.stride[0], m.padding[0], st.act, st.slope)
    elif path == "scatter_gemm":
        R, S = m.kernel_size
        contrib = (alloc(("contrib", st.index), (B, H, W, K * R * S)) if alloc is not None
                   else torch.empty(B, H, W, K * R * S, dtype=torch.float32, device=t.device))
        ops.conv_fwd(ops.geom(B, H, W, Cp, H, W, K * R * S, 1, 1, 1, 0), t, plan.packed(st, "scatter", Cp), contrib,
                     ops.epilogue(), live=(c_log, None))
        yield
        ops.col2im(contrib, K * R * S, bias, y, B, H, W, P, Q, K, K, R, S, m.stride[0], m.padding[0], st.act, st.slope)
    else:
        ep = ops.epilogue(bias=bias, act=st.act, slope=st.slope, mask=folded, bn_fwd=bn_fwd)
        if jmask is not None:
            ep.mask, ep.mask_ld = jmask.data_ptr(), jmask.stride(0)
            ep.refs["mask"] = jmask
        if st.index == 0 and st.kind == "conv" and c_log < Cp:
            ep.in_ch_live = c_log          # channel padding of a first layer: kernels that can skip it do
        if path == "flat_gemm":       # (unpadded: every one of the row's H*W*Cp channels carries data)
            Cp = c_log = H * W * Cp
        if path == "convT":
            ops.conv_bwd_data(sv.geom, t, plan.packed(st, "fwd", Cp), y, ep, live=(None, c_log))
        else:
            ops.conv_fwd(sv.geom, t, plan.packed(st, "fwd", Cp), y, ep, out_ld=out_ld, live=(c_log, None))
        yield


def chain_forward_gen(plan: ChainPlan, x: torch.Tensor, training: bool, c_log_in: int, save: bool, groups: int = 1,
                      join=None, first_mask_applied: bool = False, lane=None, alloc=None):
    """Generator form of the forward pass (see ``run_parallel``): yields after every GEMM request.
    x: NHWC [B,H,W,Cp] fp32 CUDA.  Returns (y_last, saved list).

    ``join`` = (joint [B, Ctot] fp32, column offset, mask [B, Ctot] or None): the last stage (``join_ok``; output map
    1x1) writes act(conv) * mask[:, off:off+K] into joint[:, off:off+K] instead of a tensor of its own -- the
    concatenation and the Dropout2d in front of the consuming chain cost no launch (mnist.py:152-154).
    ``first_mask_applied``: the input already carries the first stage's Dropout2d mask (it was folded into the
    producers that way); the mask is still drawn, in order, and saved for the backward pass.
    ``lane`` (dropout.Lane): the chain's Dropout2d masks are the requests of that lane (chains advanced side by side).
    ``alloc(tag, shape)``: where the stage outputs live instead of fresh tensors (persistent buffers of a forward pass
    that is computed ahead of its iteration, AliStepper.pipeline_reduce).

    ``groups`` > 1: the batch holds that many independent forward passes back to back (equal sample counts).  The
    convolutions run once over all of them; BatchNorm takes its batch statistics -- and updates the running ones --
    pass by pass, in order, exactly as separate calls would."""
    saved = []
    cur, c_log = x, c_log_in
    folded = None        # mask of the coming stage, already applied by the previous stage's GEMM epilogue
    early = None         # mask of the coming stage, requested early (its BatchNorm statistics needed it), not applied
    bn_fwd = None        # (partials, groups, early, slots) of the coming stage's BatchNorm, left by the previous GEMM
    for si, st in enumerate(plan.stages):
        B, H, W, Cp = cur.shape
        nxt = plan.stages[si + 1] if si + 1 < len(plan.stages) else None
        sv = _Saved()
        sv.x_in, sv.bn, sv.pattern, sv.training, sv.c_log = cur, st.bn, st.pattern, training, c_log
        if st.kind == "flat":
            resolve_flat(st, (B, H, W, Cp), c_log)
        sv.in_shape, sv.out_shape = (B, H, W, Cp), _out_shape(st, B, H, W, Cp)
        sv.geom, sv.route = _geom(st, sv.in_shape, sv.out_shape), route(st, sv.in_shape, c_log)
        sv.mask = folded if folded is not None else early
        if sv.mask is None and st.has_drop and training:
            sv.mask = _dropout.next_mask(B, c_log, st.drop_p, cur.device, Cp, lane=lane)
        sv.t = _pre_ops(st, sv, bn_fwd and (bn_fwd[0], bn_fwd[3]), folded is not None or (si == 0 and first_mask_applied),
                        groups)
        K = sv.out_shape[3]
        out_ld, jmask = 0, None
        if nxt is None and join is not None:
            joint, joff, jm = join
            if sv.out_shape[1:3] != (1, 1) or joint.shape[0] != B or not join_ok(plan):
                raise ValueError("chain_forward(join=...): the last stage must be a plain conv GEMM onto a 1x1 map")
            out_ld = joint.shape[1]
            sv.y = joint[:, joff:joff + K].unflatten(1, (1, 1, K))     # [B,1,1,K] view, rows out_ld apart
            jmask = None if jm is None else jm[:, joff:joff + K]
        else:
            sv.y = (alloc(("y", si), sv.out_shape) if alloc is not None
                    else torch.empty(sv.out_shape, dtype=torch.float32, device=cur.device))
        folded, early, bn_fwd = _for_next_stage(nxt, sv, groups, lane) if nxt is not None else (None, None, None)
        yield from _launch_fwd(plan, st, sv, folded, bn_fwd, out_ld, jmask, alloc)
        if save:
            saved.append(sv)
        cur, c_log = sv.y, K
    return cur, saved


def wgrad_geoms(plan: ChainPlan, saved):
    """Geometries for ``FoldQueue.expect`` (they set how far each weight gradient is split): one per stage that is not
    on the direct ``tconv1`` weight-gradient path.  This is the parent's over-count, kept on purpose (the list as it was
    before stages had routes): the "head", "first_direct" and "convT_scatter" paths launch no weight-gradient GEMM
    either, but dropping them changes the split and with it the summation order -- the bits -- of every weight gradient."""
    return [sv.geom for sv in saved if sv.route.wgrad[0] != "tconv1"]


def _head_bwd_ok(st: Stage, sv, ld: int) -> bool:
    """Does ``ops.head_bwd`` serve this stage's data gradient (and with it its parameter gradients)?  A GEMV head with
    dense operands, every channel real and no BatchNorm in front, fp32 (the kernel reproduces the fp32 MFMA's bits, not
    the fp16 one's) -- unless ALI_NO_HEAD_BWD=1 keeps it on the GEMM."""
    return (sv.route.fwd == "head" and sv.route.wgrad[0] == "head" and sv.bn is None and ld == 0
            and not ops._PRECISION["f16"]
            and sv.c_log == sv.in_shape[3] and sv.t.is_contiguous() and sv.x_in.is_contiguous()
            and (sv.mask is None or sv.mask.stride(1) == 1) and not ops.switched_off("ALI_NO_HEAD_BWD"))


def _param_grads(st: Stage, sv, g_pre, ld: int, grads, grad_dst, fold, head_later: bool = False):
    """Weight and bias gradient of the stage's module (nothing in the chain reads them: no yield) into ``grads``.
    ``head_later``: a "head" stage's launch is left to ``_data_grad`` (one launch for both); returns its (dw, db)."""
    m, g = st.mod, sv.geom
    B, H, W, Cp = sv.in_shape
    _, P, Q, K = sv.out_shape
    c_in = sv.c_log
    path, db_path = sv.route.wgrad if fold is None else sv.route.wgrad_fold
    fused_db = None
    if db_path == "unflat":
        Cc, hh, ww = st.unflat
        db = ops.colsum(B, hh * ww * Cc, hh * ww * Cc, g_pre).reshape(hh * ww, Cc).t().reshape(-1)
        grads[id(m.bias)] = grad_dst[id(m.bias)].copy_(db) if id(m.bias) in grad_dst else db
    elif db_path == "fused":
        fused_db = grad_dst.get(id(m.bias))
        if fused_db is None:
            fused_db = torch.empty(K, dtype=torch.float32, device=g_pre.device)
        grads[id(m.bias)] = fused_db
    elif db_path == "colsum":
        grads[id(m.bias)] = ops.colsum(B * P * Q, K, K, g_pre, out=grad_dst.get(id(m.bias)))
    dw = grads[id(m.weight)] = grad_dst[id(m.weight)] if id(m.weight) in grad_dst else torch.empty_like(m.weight)
    if path == "flat_repack":             # rows in the pack's t*C + c order, re-packed into [O][C*h*w] right away
        O, I, T = m.out_features, m.in_features, H * W
        tmp = torch.empty(O, I, device=dw.device)
        ops.conv_bwd_weight(g, sv.t, g_pre, tmp, I, O, I, 1, 0)      # (not deferred)
        ops.pack_weights(tmp, dw, O, I // T, T, T, I, 1, I // T)
        return
    if st.kind == "flat":                 # written in the view's layout [O][C][h][w] = the Linear's own [O][C*h*w]
        ops.conv_bwd_weight(g, sv.t, g_pre, dw, c_in, K, dw.stride(0), H * W, 1, db=fused_db, dy_ld=ld, defer=fold)
        return
    R, S = m.kernel_size if st.kind != "linear" else (1, 1)
    if path == "convT_scatter" and sv.t.is_contiguous() and g_pre.is_contiguous() and dw.stride(2) == S * dw.stride(3):
        # one-channel tail (stride 2): pixel-contraction kernel instead of a GEMM with one gathered channel
        if ops.tconv_scatter_wgrad(sv.t, g_pre, 1, dw, dw.stride(0), dw.stride(3), B, H, W, Cp, P, Q, R, S, m.stride[0],
                                   m.padding[0]) is not None:
            return
    if path == "head" and head_later:     # (the data gradient's launch writes them: _data_grad, head_bwd)
        return dw.reshape(-1), fused_db
    if path == "head":                    # (a head never joins: ld == 0)
        ops.head_wgrad(sv.t.reshape(B, Cp)[:, :c_in], g_pre.reshape(B), dw.reshape(-1), db=fused_db)
    elif path == "first_direct":
        # dW[k][c][tap] = sum big=g_pre[..,k] * small=t[..,c], all input channels in one launch
        ops.tconv1_wgrad(g_pre, sv.t, Cp, c_in, dw, c_in * R * S, 1, R * S, B, P, Q, K, R, S, m.padding[0])
    elif path == "conv":
        ops.conv_bwd_weight(g, sv.t, g_pre, dw, c_in, K, dw.stride(0), dw.stride(1), dw.stride(3), db=fused_db,
                            dy_ld=ld, defer=fold)
    elif path == "tconv1":
        ops.tconv1_wgrad(sv.t, g_pre, 1, 1, dw, R * S, 1, 0, B, H, W, Cp, R, S, m.padding[0])
    elif path in ("convT", "convT_scatter"):
        # gathered operand = convT output-grad (channels K), dense = convT input (channels Cp)
        ops.conv_bwd_weight(g, g_pre, sv.t, dw, K, c_in, dw.stride(0), dw.stride(1), dw.stride(3), defer=fold)
    elif path == "linear":
        ops.conv_bwd_weight(g, sv.t, g_pre, dw, m.in_features, m.out_features, m.in_features, 1, 0, defer=fold)
    else:                                 # Linear + Unflatten(C, h, w): rows in n' = t*C + co order, re-packed right away
        (O, I), (Cc, hh, ww) = m.weight.shape, st.unflat
        tmp = torch.empty(O, I, device=dw.device)
        ops.conv_bwd_weight(g, sv.t, g_pre, tmp, I, O, I, 1, 0)      # (not deferred)
        ops.pack_weights(tmp, dw, Cc, hh * ww, I, I, I, Cc * I, 1)


def _plane_grads(plan: ChainPlan, st: Stage, sv, g_pre, gx_planes):
    """First stage of the hand-scheduled step: only the input channels ``gx_planes`` of the data gradient, with the
    input's Dropout2d mask columns applied, as [B,H,W,len(gx_planes)] -- or None when the route has no plane form
    for them (generator: yields after a GEMM request)."""
    m, NP = st.mod, len(gx_planes)
    B, H, W, Cp = sv.in_shape
    _, P, Q, K = sv.out_shape
    R, S = m.kernel_size
    form = sv.route.planes
    # The scatter form's contribution tensor (planes * taps floats per pixel, written and read once) makes it HBM bound:
    # measured break-even with the implicit GEMM at about 6 planes of a 5x5 filter, a clear win below
    if form is None or (form == "scatter" and not (1 <= NP <= 8 and NP * R * S <= 128)):
        return None
    planes = torch.empty(B, H, W, NP, dtype=torch.float32, device=g_pre.device)
    if form == "direct":
        wd = plan.packed(st, "dgrad", Cp)                  # [Cpad][T][K]: row c is the [T][K] filter of plane c
        for j, c in enumerate(gx_planes):     # (the input's Dropout2d mask column scales the plane in the same launch)
            ops.tconv1_fwd(g_pre, wd[c], None, planes[..., j], B, P, Q, K, R, S, m.padding[0], NP, ACT_NONE, 0.0,
                           rowscale=None if sv.mask is None else sv.mask[:, c])
        return planes
    wd = plan.packed(st, ("scatter_dgrad", tuple(gx_planes)), Cp)
    if ops.tconv_scatter_ok(K, NP, R, S, m.stride[0]) and g_pre.is_contiguous():
        ops.tconv_scatter(g_pre, wd, None, planes, B, P, Q, K, H, W, NP, NP, R, S, m.stride[0], m.padding[0])
    else:
        contrib = torch.empty(B, P, Q, NP * R * S, dtype=torch.float32, device=g_pre.device)
        ops.conv_fwd(ops.geom(B, P, Q, K, P, Q, NP * R * S, 1, 1, 1, 0), g_pre, wd, contrib, ops.epilogue())
        yield
        ops.col2im(contrib, NP * R * S, None, planes, B, P, Q, H, W, NP, NP, R, S, m.stride[0], m.padding[0])
    if sv.mask is not None:
        cols = torch.cat([sv.mask[:, c:c + 1] for c in gx_planes], dim=1)
        planes = planes * cols.reshape(B, 1, 1, -1)
    return planes


def _data_grad(plan: ChainPlan, st: Stage, sv, g_pre, ld: int, pact, pslope, want: bool, need_params: bool, grads,
               grad_dst, head_pg=None):
    """Gradient of the pre-activation that produced the stage's input (activation ``pact``): the data-gradient GEMM
    folded with what sits between the two -- Dropout2d mask and act' in its epilogue, BatchNorm backward (whose
    parameter gradients go into ``grads``) fused with the LeakyReLU derivative.  Generator: yields after a GEMM
    request.  ``want`` False: only the BatchNorm parameter gradients are needed (returns None).
    A GEMV head (``_head_bwd_ok``) is an outer product, not a GEMM: ``ops.head_bwd`` writes it, and with ``head_pg`` =
    (dw, db) of ``_param_grads(head_later=True)`` the stage's parameter gradients in the same launch."""
    m, g, bn, rt = st.mod, sv.geom, sv.bn, sv.route
    B, H, W, Cp = sv.in_shape
    dact_y = sv.x_in if pact != ACT_NONE else None
    gt = torch.empty(sv.in_shape, dtype=torch.float32, device=g_pre.device)
    if _head_bwd_ok(st, sv, ld):
        dw, db = head_pg if head_pg is not None else (None, None)
        ops.head_bwd(g_pre.reshape(B), plan.packed(st, "fwd", Cp).reshape(-1), dact_y, pact, pslope, sv.mask,
                     gt.reshape(B, Cp), sv.t.reshape(B, Cp), dw, db)
        yield                             # (where the GEMM's request was: the rounds of run_parallel stay as they are)
        return gt
    bn_red = None
    if bn is None:
        ep = ops.epilogue(mask=sv.mask, dact_y=dact_y, dact=pact, dslope=pslope)
    else:
        # BatchNorm backward needs sum(g~ * xhat) and sum(g~) of the gradient this GEMM produces: its epilogue
        # accumulates them per M-tile while the values are in registers
        mask_in = sv.mask if sv.pattern == ["drop", "bn"] else None
        mask_pre = sv.mask if sv.pattern == ["bn", "drop"] else None
        slots = ops.conv_mtiles(g, 0 if rt.dgrad == "convT" else 1)[0] if rt.bn_reduce else 0
        if slots > 0:
            bn_red = (torch.empty(2 * Cp * slots, dtype=torch.float32, device=g_pre.device), slots)
            ep = ops.epilogue(bn_bwd=(bn_red[0], sv.x_in, sv.bn_stats[0], sv.bn_stats[1], mask_in, mask_pre, slots))
        else:
            ep = ops.epilogue()
    if rt.dgrad == "tconv1" and bn is None and sv.mask is None:
        ops.tconv1_dgrad(g_pre, 1, plan.packed(st, "fwd", Cp), dact_y, pact, pslope, gt, B, H, W, Cp, m.kernel_size[0],
                         m.kernel_size[1], m.padding[0])
    elif st.kind == "convT":
        ops.conv_fwd(g, g_pre, plan.packed(st, "dgrad", Cp), gt, ep, live=(None, sv.c_log))
        yield
    else:
        wc = H * W * Cp if rt.dgrad == "flat_gemm" else Cp          # (flat_gemm: the map is one unpadded row)
        ops.conv_bwd_data(g, g_pre, plan.packed(st, "dgrad", wc), gt, ep, in_ld=ld,
                          live=(wc if rt.dgrad == "flat_gemm" else sv.c_log, None))
        yield
    if bn is None:
        return gt
    use_batch = sv.training or bn.running_mean is None
    slope = pslope if pact == ACT_LEAKY else -1.0
    out = dict(want_gx=want, out_dgamma=grad_dst.get(id(bn.weight)) if need_params else None,
               out_dbeta=grad_dst.get(id(bn.bias)) if need_params else None)
    if bn_red is not None:
        dgam, dbet, gprev = ops.bn_bwd_from_partials(bn_red[0], bn_red[1], sv.x_in, gt, mask_in, mask_pre, sv.bn_stats,
                                                     bn.weight.detach(), B, H * W, Cp, use_batch, slope, **out)
    else:
        dgam, dbet, gprev = ops.bn_bwd(sv.x_in, gt, mask_in, mask_pre, sv.bn_stats, bn.weight.detach(), B, H * W, Cp,
                                       use_batch, slope, **out)
    if need_params:
        grads[id(bn.weight)], grads[id(bn.bias)] = dgam, dbet
    if pact == ACT_TANH and gprev is not None:
        gprev = ops.act_bwd(gprev, sv.x_in, ACT_TANH, 0.0)
    return gprev


def chain_backward_gen(plan: ChainPlan, saved, gy: torch.Tensor, c_log_in: int, need_gx: bool, need_params: bool = True,
                       grad_dst=None, gx_planes=None, gy_ld: int = 0, gy_pre: bool = False, in_act=None, fold=None):
    """Generator form of the backward pass (see ``run_parallel``): yields after every data-gradient GEMM request (the
    weight gradients are deferred to ``fold`` or launched at once: nothing in the chain reads them).
    Returns (gx or None, {param tensor id -> grad}).  ``c_log_in``: the forward pass's.  ``grad_dst`` optionally maps
    id(param) to a preallocated destination (a view of a flat gradient buffer) that the kernels write directly.
    ``gx_planes`` (hand-scheduled step only): instead of the full input gradient return only these input
    channels of it, as a [B,H,W,len(gx_planes)] tensor -- the first layer's data gradient is consumed one plane
    at a time (image plane towards G, embedding plane towards the digit table).
    ``gy_ld`` > 0 (needs ``join_ok``): ``gy`` is a column range (strided view, rows ``gy_ld`` floats apart) of a wider
    buffer; ``gy_pre``: it already is the gradient of the last stage's PRE-activation.  ``in_act`` = (act, slope) of the
    activation that produced this chain's input ``x`` (the ends of the chains whose outputs were joined): the returned
    gradient is then the one of their pre-activations, computed by the first stage's data-gradient epilogue.
    ``fold`` (ops.FoldQueue): the weight-gradient launches leave their slab reductions to ``fold.flush()`` -- the
    parameter gradients are complete only after the caller has flushed."""
    grads = {}
    grad_dst = grad_dst or {}
    n = len(plan.stages)
    last = plan.stages[-1]
    assert saved[0].c_log == c_log_in, "chain_backward: c_log_in differs from the forward pass's"
    if gy_ld:
        if not (gy_pre or last.act == ACT_NONE) or not join_ok(plan):
            raise ValueError("chain_backward(gy_ld=...): needs join_ok(plan) and a pre-activation gradient")
        g_pre = gy
    else:
        gy = gy.contiguous()
        g_pre = gy if (gy_pre or last.act == ACT_NONE) else ops.act_bwd(gy, saved[-1].y, last.act, last.slope)
    for i in range(n - 1, -1, -1):
        st, sv = plan.stages[i], saved[i]
        assert not isinstance(sv.bn_stats, list), "grouped forward state: backpropagate slice_saved(saved, g, groups)"
        ld = gy_ld if i == n - 1 else 0          # pixel pitch of g_pre (0 = dense)
        head_pg = None
        if need_params:       # (a head's own gradients ride in its data-gradient launch when there is one)
            head_pg = _param_grads(st, sv, g_pre, ld, grads, grad_dst, fold,
                                   head_later=i > 0 and _head_bwd_ok(st, sv, ld))
        if i > 0:
            g_pre = yield from _data_grad(plan, st, sv, g_pre, ld, plan.stages[i - 1].act, plan.stages[i - 1].slope, True,
                                          need_params, grads, grad_dst, head_pg)
    # ---- the first stage's data gradient: a few planes of it, none of it, or all of it
    gx = (yield from _plane_grads(plan, st, sv, g_pre, gx_planes)) if gx_planes is not None else None
    if gx is None and (need_gx or sv.bn is not None):
        gx = yield from _data_grad(plan, st, sv, g_pre, ld, *(in_act or (ACT_NONE, 0.0)), need_gx, need_params, grads,
                                   grad_dst)
    return gx, grads


# ---------------------------------------------------------------------- gradient of a gradient norm (WGAN-GP)
# A stack of convolutions and LeakyReLUs (no BatchNorm, no Dropout) is piecewise linear in its input.  With a_l the
# activations, h_l = act'(a_l) * g_l the pre-activation gradients of a backward pass and g0 its input gradient, the
# gradient of any f(g0) with respect to the weights is one more FORWARD pass of the tangent v = df/dg0 through the same
# convolutions, u_l = act'(a_l) * conv(W_l, u_{l-1}) (no bias), and then dW_l = bwd_weight(x = u_{l-1}, dy = h_l):
# g_{l-1} is linear in W_l and the masks act'(a_l) are piecewise constant.  Biases and the input get zero.
def _plain_stack(plan: ChainPlan, what: str):
    for st in plan.stages:
        if st.pre or st.kind not in ("conv", "flat") or st.act not in (ACT_NONE, ACT_LEAKY):
            raise NotImplementedError(f"ali_hip.chain.{what}: needs a stack of Conv2d / Flatten + Linear stages with "
                                      f"LeakyReLU or no activation and nothing in front of them (stage {st.index}: "
                                      f"{st.kind}, pre-ops {st.pattern}, activation {st.act})")


def saved_rows(saved, lo: int, hi: int):
    """The saved state of the samples [lo, hi) of a forward pass over a stack without BatchNorm (rows of a batch are
    independent there: contiguous row ranges of every activation)."""
    out = []
    for sv in saved:
        assert sv.bn is None and sv.bn_stats is None, "saved_rows: BatchNorm statistics couple the rows of a batch"
        s2 = _Saved()
        s2.x_in, s2.t, s2.y = sv.x_in[lo:hi], sv.t[lo:hi], sv.y[lo:hi]
        s2.mask = None if sv.mask is None else sv.mask[lo:hi]
        s2.bn, s2.bn_stats, s2.pattern, s2.training, s2.route, s2.c_log = None, None, sv.pattern, sv.training, sv.route, sv.c_log
        s2.in_shape, s2.out_shape = (hi - lo,) + tuple(sv.in_shape[1:]), (hi - lo,) + tuple(sv.out_shape[1:])
        g = sv.geom
        s2.geom = ops.geom(hi - lo, g.H, g.W, g.C, g.P, g.Q, g.K, g.R, g.S, g.stride, g.pad)
        out.append(s2)
    return out


def chain_backward_keep_gen(plan: ChainPlan, saved, gy: torch.Tensor, c_log_in: int, need_gx: bool = True,
                            gx_planes=None, first_rows=None):
    """The data-gradient half of ``chain_backward_gen`` over a plain stack, KEEPING every stage's pre-activation
    gradient: returns (gx or None, [h_0 .. h_{n-1}]), h_l the gradient of stage l's convolution output (what its
    weight gradient contracts with).  No parameter gradients.  ``first_rows`` = (lo, hi): the first stage's data
    gradient -- the largest map -- only for those samples; ``gx_planes`` as in ``chain_backward_gen``."""
    _plain_stack(plan, "chain_backward_keep")
    n = len(plan.stages)
    last = plan.stages[-1]
    assert saved[0].c_log == c_log_in, "chain_backward_keep: c_log_in differs from the forward pass's"
    gy = gy.contiguous()
    g_pre = gy if last.act == ACT_NONE else ops.act_bwd(gy, saved[-1].y, last.act, last.slope)
    hs = [None] * n
    for i in range(n - 1, -1, -1):
        hs[i] = g_pre
        if i > 0:
            g_pre = yield from _data_grad(plan, plan.stages[i], saved[i], g_pre, 0, plan.stages[i - 1].act,
                                          plan.stages[i - 1].slope, True, False, {}, {})
    if not need_gx:
        return None, hs
    st, sv = plan.stages[0], saved[0]
    if first_rows is not None:
        sv, g_pre = saved_rows(saved[:1], *first_rows)[0], g_pre[first_rows[0]:first_rows[1]]
    gx = (yield from _plane_grads(plan, st, sv, g_pre, gx_planes)) if gx_planes is not None else None
    if gx is None:
        gx = yield from _data_grad(plan, st, sv, g_pre, 0, ACT_NONE, 0.0, True, False, {}, {})
        if gx_planes is not None:
            gx = torch.stack([gx[..., c] for c in gx_planes], dim=-1)
    return gx, hs


def chain_tangent_gen(plan: ChainPlan, saved, u0: torch.Tensor):
    """The tangent pass over the saved activations of a plain stack: u_0 = ``u0`` (NHWC, the forward input's shape),
    u_l = act'(a_l) * conv(W_l, u_{l-1}) without bias -- one forward GEMM per stage with the activation derivative as
    its epilogue.  Returns [u_0 .. u_{n-1}], the inputs of the n stages (the last stage's own output is not needed for
    the weight gradients).  Generator: yields after every GEMM request."""
    _plain_stack(plan, "chain_tangent")
    if tuple(u0.shape) != tuple(saved[0].in_shape):
        raise ValueError(f"chain_tangent: u0 {tuple(u0.shape)} is not the forward input's shape {tuple(saved[0].in_shape)}")
    us = [u0.contiguous()]
    for st, sv in zip(plan.stages[:-1], saved[:-1]):
        Cp = sv.in_shape[3]
        u = torch.empty(sv.out_shape, dtype=torch.float32, device=u0.device)
        ep = ops.epilogue(dact_y=sv.y if st.act != ACT_NONE else None, dact=st.act, dslope=st.slope)
        if st.index == 0 and sv.c_log < Cp:
            ep.in_ch_live = sv.c_log
        flat = sv.route.fwd == "flat_gemm"                        # (the map is one unpadded row of geom.C channels)
        ops.conv_fwd(sv.geom, us[-1], plan.packed(st, "fwd", sv.geom.C if flat else Cp), u, ep,
                     live=(sv.geom.C if flat else sv.c_log, None))
        yield
        us.append(u)
    return us


def tangent_param_grads(plan: ChainPlan, saved, us, hs, grad_dst=None, head_ones: bool = False):
    """{id(weight): dW_l = bwd_weight(x = u_{l-1}, dy = h_l)} of every stage (``chain_tangent_gen``'s ``us``,
    ``chain_backward_keep_gen``'s ``hs``), written into ``grad_dst`` {id(param): view} where it names the weight.
    Biases get nothing (their gradient is zero).  ``head_ones``: the backward pass started from gy = 1, so the
    weight gradient of a Flatten + Linear(., 1) head on a 1x1 map is the column sum of its tangent input."""
    grad_dst = grad_dst or {}
    out = {}
    for st, sv, u, h in zip(plan.stages, saved, us, hs):
        w = st.mod.weight
        B, H, W, Cp = sv.in_shape
        if (head_ones and st.kind == "flat" and st.index == len(plan.stages) - 1 and H * W == 1 and w.shape[0] == 1
                and Cp == sv.c_log and st.act == ACT_NONE):
            dw = grad_dst[id(w)] if id(w) in grad_dst else torch.empty_like(w)
            ops.colsum(B, Cp, Cp, u, out=dw.view(-1))
            out[id(w)] = dw
            continue
        s2 = _Saved()
        for name in _Saved.__slots__:
            if hasattr(sv, name):
                setattr(s2, name, getattr(sv, name))
        s2.t = s2.x_in = u
        tmp = {}
        _param_grads(st, s2, h, 0, tmp, {id(w): grad_dst[id(w)]} if id(w) in grad_dst else {}, None)
        out[id(w)] = tmp[id(w)]
    return out


def chain_param_grads(plan: ChainPlan, saved, hs, grad_dst=None):
    """The parameter-gradient half that ``chain_backward_keep_gen`` leaves out: weight and bias gradients of every stage
    from its saved input and its pre-activation gradient ``hs[l]`` (both may be row ranges: ``saved_rows``).  Returns
    {id(param): grad}; ``grad_dst`` as in ``chain_backward_gen``."""
    grads = {}
    for st, sv, h in zip(plan.stages, saved, hs):
        _param_grads(st, sv, h, 0, grads, grad_dst or {}, None)
    return grads


def chain_backward_keep(*args, **kwargs):
    return drive(chain_backward_keep_gen(*args, **kwargs))


def chain_tangent(*args, **kwargs):
    return drive(chain_tangent_gen(*args, **kwargs))


class ChainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan: ChainPlan, training: bool, c_log_in: int, x, *params):
        need_grad = any(ctx.needs_input_grad[3:])
        y, saved = chain_forward(plan, x, training, c_log_in, save=need_grad)
        ctx.plan, ctx.saved_stages, ctx.c_log_in = plan, saved, c_log_in
        ctx.param_ids = [id(p) for p in plan.params()]
        return y

    @staticmethod
    def backward(ctx, gy):
        need_gx = ctx.needs_input_grad[3]
        need_params = any(ctx.needs_input_grad[4:])
        gx, grads = chain_backward(ctx.plan, ctx.saved_stages, gy, ctx.c_log_in, need_gx, need_params)
        ctx.saved_stages = None
        pg = tuple(grads.get(pid) if need else None for pid, need in zip(ctx.param_ids, ctx.needs_input_grad[4:]))
        return (None, None, None, gx) + pg


_PLANS = weakref.WeakKeyDictionary()   # nn.Sequential -> ChainPlan; kept OUT of the module so that the reference's
#                                        checkpoint style torch.save({'E': E, ...}) (train_mnist_image_scm.py:61-67) still pickles


def get_plan(seq: nn.Sequential) -> ChainPlan:
    plan = _PLANS.get(seq)
    if plan is None or plan.seq() is not seq:
        plan = ChainPlan(seq)
        _PLANS[seq] = plan
    return plan


def run_chain(seq: nn.Sequential, x: torch.Tensor, c_log_in: Optional[int] = None) -> torch.Tensor:
    """Execute ``seq`` on NHWC ``x`` through the HIP kernels (autograd aware)."""
    if not x.is_cuda:
        raise RuntimeError("ali_hip.chain.run_chain needs CUDA tensors")
    plan = get_plan(seq)
    x = x.contiguous()
    if c_log_in is None:
        c_log_in = x.shape[-1]
    return ChainFn.apply(plan, seq.training, c_log_in, x, *plan.params())
