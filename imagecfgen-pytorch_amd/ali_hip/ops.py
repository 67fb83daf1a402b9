"""Tensor-level wrappers over the C ABI (device pointers from ``tensor.data_ptr()``,
stream from ``torch.cuda.current_stream()``).  PyTorch is plumbing here: memory,
streams, autograd bookkeeping.  Every function requires CUDA fp32 contiguous
tensors and raises otherwise -- there is no fallback path.
"""
import collections
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import torch

from . import _lib
from ._lib import ACT_LEAKY, ACT_NONE, ACT_TANH, AliConvGeom, AliEpilogue  # noqa: F401

_WS = {}
_WS_BYTES = 256 << 20


def set_workspace_bytes(n: int):
    global _WS_BYTES
    _WS_BYTES = int(n)
    _WS.clear()


def workspace(device, slot: int = 0) -> torch.Tensor:
    """One scratch slab per device, reused stream-ordered by every kernel.  Zero-filled once: its first 4 KiB are the
    split-K arrival counters of the GEMM kernels, which every launch leaves at zero (include/ali_hip.h).
    ``slot`` > 0: the additional slabs the jobs of a multi-job GEMM launch use (one each: ``gemm_batch``)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), slot)
    ws = _WS.get(key)
    if ws is None or ws.numel() < _WS_BYTES:
        ws = torch.zeros(_WS_BYTES, dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, name="tensor"):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous fp32 CUDA tensor, got {t.dtype} {t.device} "
                         f"contiguous={t.is_contiguous()}")
    return c_void_p(t.data_ptr())


def _opt(t, name="tensor"):
    return None if t is None else _chk(t, name)


_PRECISION = {"f16": False}
_DACT16 = {"on": __import__("os").environ.get("ALI_NO_DACT16", "0") in ("", "0")}   # (A/B switch of AliEpilogue.dact_y16)


class precision:
    """``with ops.precision("f16"):`` -- the GEMMs launched inside run their contraction on fp16 MFMA
    (v_mfma_f32_32x32x16_f16, fp32 accumulation; include/ali_hip.h: AliEpilogue.mfma_f16) where their fast path
    applies; "f32" (default) is the exact fp32 MFMA everywhere."""

    def __init__(self, name):
        if name not in ("f32", "f16"):
            raise ValueError(f"precision must be 'f32' or 'f16', got {name!r}")
        self.f16 = name == "f16"

    def __enter__(self):
        self.prev, _PRECISION["f16"] = _PRECISION["f16"], self.f16
        return self

    def __exit__(self, *exc):
        _PRECISION["f16"] = self.prev


def geom(B, H, W, C, P, Q, K, R, S, stride, pad) -> AliConvGeom:
    return AliConvGeom(B, H, W, C, P, Q, K, R, S, stride, pad)


def epilogue(bias=None, act=ACT_NONE, slope=0.0, mask=None, dact_y=None, dact=ACT_NONE, dslope=0.0,
             bn_fwd=None, bn_bwd=None) -> AliEpilogue:
    """``bn_fwd`` = (part, groups, stat_mask or None[, slots]): also leave the per-tile (sum, sum of squares) of the
    output; ``bn_bwd`` = (part, x, mean, invstd, mask_in or None, mask_pre or None[, slots]): per-tile (sum g~*xhat,
    sum g~) of a data gradient (include/ali_hip.h, AliEpilogue).  ``slots`` = the slot count ``part`` was sized for
    (``conv_mtiles``): the launch refuses to run when its own M-tile count differs."""
    ep = AliEpilogue()
    # (python-side references of the operands behind the raw pointers: keeps them alive, lets a launch hook see them)
    ep.refs = {"bias": bias, "mask": mask, "dact_y": dact_y, "bn_fwd": bn_fwd, "bn_bwd": bn_bwd}
    ep.bias = _opt(bias, "bias")
    ep.act, ep.slope = act, slope
    ep.mask = _opt(mask, "mask")
    ep.mask_ld = mask.shape[1] if mask is not None else 0
    ep.dact_y = _opt(dact_y, "dact_y")
    ep.dact, ep.dslope = dact, dslope
    tw = getattr(dact_y, "_ali16", None) if (dact_y is not None and _PRECISION["f16"] and _DACT16["on"]) else None
    if tw is not None and tw.shape == dact_y.shape and tw.is_contiguous():
        ep.dact_y16 = c_void_p(tw.data_ptr())     # act' from the fp16 twin: half the bytes of the epilogue's read
        ep.refs["dact_y16"] = tw
    ep.mfma_f16 = int(_PRECISION["f16"])
    if bn_fwd is not None:
        part, groups, smask = bn_fwd[:3]
        ep.bn_slots = int(bn_fwd[3]) if len(bn_fwd) > 3 else 0
        ep.bn_part, ep.bn_mode, ep.bn_groups = _chk(part, "bn_part"), 1, groups
        ep.bn_stat_mask = _opt(smask, "bn_stat_mask")
        ep.bn_mask_ld = smask.shape[1] if smask is not None else 0
    elif bn_bwd is not None:
        part, x, mean, invstd, m_in, m_pre = bn_bwd[:6]
        ep.bn_slots = int(bn_bwd[6]) if len(bn_bwd) > 6 else 0
        ep.bn_part, ep.bn_mode, ep.bn_groups = _chk(part, "bn_part"), 2, 1
        ep.bn_x, ep.bn_mean, ep.bn_invstd = _chk(x, "bn_x"), c_void_p(mean.data_ptr()), c_void_p(invstd.data_ptr())
        ep.bn_mask_in, ep.bn_mask_pre = _opt(m_in, "bn_mask_in"), _opt(m_pre, "bn_mask_pre")
        m = m_in if m_in is not None else m_pre
        ep.bn_mask_ld = m.shape[1] if m is not None else 0
    return ep


_MTILES = {}


def reload_tuning():
    """Make the library re-read its developer tuning variables (ALI_BM, ALI_BN, ALI_SPLITK, ALI_TILE_M_SCALE, ...:
    csrc/ali_common.h) and drop every host-side cache that was derived under the old ones (M-tile counts, dispatch-order
    tables, deferrable flags).  Tests and sweeps only; never while a captured graph that used the old tuning is alive."""
    _lib.load().ali_reload_tuning()
    _MTILES.clear()
    _TILE_ORDER.clear()
    _DEFERRABLE.clear()


class tuning:
    """``with ops.tuning(ALI_BM=128, ALI_BN=128): ...`` -- set tuning variables for the block, restore them after."""

    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        import os
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        reload_tuning()
        return self

    def __exit__(self, *exc):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        reload_tuning()


def conv_mtiles(g: AliConvGeom, which: int):
    """(M-tiles, tile rows, rows ordered (pixel, image)?) of the launch ali_conv_fwd (0) / ali_conv_bwd_data (1) makes."""
    f16 = int(_PRECISION["f16"])
    key = (which, f16) + tuple(getattr(g, n) for n, _ in AliConvGeom._fields_)
    hit = _MTILES.get(key)
    if hit is None:
        rows, pm = ctypes.c_int32(0), ctypes.c_int32(0)
        n = _lib.load().ali_conv_mtiles(byref(g), which, f16, byref(rows), byref(pm))
        hit = _MTILES[key] = (n, rows.value, bool(pm.value))
    return hit


ConvPlan = collections.namedtuple("ConvPlan", [n for n, _ in _lib.AliConvPlan._fields_])


def conv_plan(g: AliConvGeom, which: int, ep: AliEpilogue = None, ws_bytes=None, as_job=False) -> ConvPlan:
    """What ali_conv_fwd (0) / ali_conv_bwd_data (1) would launch for ``g`` and ``ep`` (default: a plain epilogue of the
    current ``precision``) with a workspace of ``ws_bytes`` (default: the size ``workspace`` allocates), recorded as a
    ``gemm_batch`` job when ``as_job`` (include/ali_hip.h: AliConvPlan).  Host side only: nothing is launched."""
    if ep is None:
        ep = AliEpilogue(mfma_f16=int(_PRECISION["f16"]))
    ws_bytes = _WS_BYTES if ws_bytes is None else int(ws_bytes)
    plan = _lib.AliConvPlan()
    _lib.check(_lib.load().ali_conv_plan(byref(g), which, byref(ep), ws_bytes, int(ws_bytes > 0), int(bool(as_job)),
                                         byref(plan)), "ali_conv_plan")
    return ConvPlan(*(getattr(plan, n) for n in ConvPlan._fields))


class KernelProfile:
    """Live timing of the GEMM / direct kernel launches of ONE eager iteration with HIP events on the launch stream
    (bench.py's roofline leg).  Every launch is timed once, where it runs in the iteration: ``[e0] k [e1]``.

    What makes that interval the kernel's duration as a rocprofv3 kernel trace reports it (checked against the trace of
    the same process: 4.764 vs 4.770 ms for the 88 GEMM launches of a MorphoMNIST iteration):
      * the caller keeps the stream busy with real work (graph replays of the same iteration) while the host enqueues
        the instrumented one, so its launches execute back to back -- as in a replay -- and at the clocks of the timed
        region (behind an idle or spin-waiting stream the chip clocks down: the same kernels then ran 10 % longer);
      * ``calibrate()`` measures what an ``[e0] k [e1]`` interval contains besides the kernel -- event markers plus
        dispatch latency -- as the zero-length intercept of spin kernels of two known lengths timed the same way, and
        that overhead is subtracted from every record (3.4 us plain, 5.7 us under rocprofv3).
    (An event pair attached to the dispatch itself, hipExtLaunchKernelGGL, was tried instead: its interval is 4.5 us
    LONGER than the trace's duration per launch, and it needs library support; dropped.)
    Each record: (family, algorithmic flops, algorithmic bytes, (e0, e1), shape)."""

    def __init__(self):
        self.records = []
        self.overhead_ms = 0.0
        self.spin_cycles_per_ms = None

    @staticmethod
    def _spin_pair(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
        return e0, e1

    def spin_rate(self):
        if self.spin_cycles_per_ms is None:
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            torch.cuda._sleep(20_000_000)
            t1.record()
            torch.cuda.synchronize()
            self.spin_cycles_per_ms = 20_000_000 / max(t0.elapsed_time(t1), 1e-3)
        return self.spin_cycles_per_ms

    def calibrate(self, busy=None, reps=24):
        """overhead_ms = the part of an ``[e0] k [e1]`` interval that is not the kernel.  ``busy()`` (optional) enqueues
        real work first, so that the pairs are measured behind a busy stream like the iteration itself."""
        rate = self.spin_rate()
        short, long_ = int(0.02 * rate), int(0.10 * rate)          # 20 us, 100 us
        if busy is not None:
            busy()
        else:
            torch.cuda._sleep(int(20.0 * rate))
        pairs = [(self._spin_pair(short), self._spin_pair(long_)) for _ in range(reps)]
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for (a, b), _ in pairs)[reps // 2]
        tl = sorted(a.elapsed_time(b) for _, (a, b) in pairs)[reps // 2]
        slope = (tl - ts) / (long_ - short)                       # ms per spin cycle
        self.overhead_ms = max(ts - slope * short, 0.0)
        return self.overhead_ms

    def hold(self, ms):
        """park the current stream for about ``ms`` milliseconds behind a spin kernel (fallback when the caller has no
        real work to keep the stream busy with: the chip clocks down meanwhile)"""
        torch.cuda._sleep(int(ms * self.spin_rate()))

    def _ms(self, ev):
        e0, e1 = ev
        return max(e0.elapsed_time(e1) - self.overhead_ms, 1e-4)

    def _table(self, key):
        torch.cuda.synchronize()
        tab = {}
        for name, flops, nbytes, ev, desc in self.records:
            f = tab.setdefault(key(name, desc), {"launches": 0, "flops": 0.0, "ms": 0.0, "bytes": 0.0})
            f["launches"] += 1
            f["flops"] += flops
            f["bytes"] += nbytes
            f["ms"] += self._ms(ev)
        return tab

    def summary(self):
        return self._table(lambda name, desc: name)

    def by_shape(self):
        return self._table(lambda name, desc: (name,) + desc)


_PROFILE = None


def set_profile(p):
    global _PROFILE
    _PROFILE = p


_HOOK = None


class launch_hook:
    """``with ops.launch_hook(obj):`` -- tests only.  Every GEMM launch made inside the block is reported to ``obj``
    right after it has been issued (``obj.scatter(...)`` for ``tconv_scatter``):
    ``obj.gemm(kind, g, a, w, out, ep, in_ld, out_ld)`` for ``conv_fwd`` ("fwd") /
    ``conv_bwd_data`` ("bwd_data") and ``obj.wgrad(g, x, dy, dst, cg_log, cd_log, strides, db, dy_ld)`` for
    ``conv_bwd_weight`` -- the latter returns a callable (or None) that is run once the result is final (at once, or
    after ``FoldQueue.flush`` for deferred launches).  tests/launch_audit.py re-computes each launch with torch on the
    CPU from the very operands the kernel read."""

    def __init__(self, obj):
        self.obj = obj

    def __enter__(self):
        global _HOOK
        self.prev, _HOOK = _HOOK, self.obj
        return self.obj

    def __exit__(self, *exc):
        global _HOOK
        _HOOK = self.prev


def _geom_cost(g: AliConvGeom, live=None):
    """(algorithmic FLOP, algorithmic bytes, shape key) of one GEMM launch: 2*B*P*Q*K*C*R*S and both activations + the
    weights once, fp32.  ``live`` = (c, k): the channels of x / y that carry data where a channel stride is padded
    (5 of 8 image planes, 771 of 800 Generator inputs) -- multiplications by the zero padding are not algorithmic work."""
    c = live[0] if (live and live[0]) else g.C
    k = live[1] if (live and live[1]) else g.K
    return (2.0 * g.B * g.P * g.Q * k * c * g.R * g.S,
            4.0 * (g.B * g.H * g.W * c + g.B * g.P * g.Q * k + k * c * g.R * g.S),
            (g.B, g.H, g.W, g.C, g.P, g.Q, g.K, g.R, g.stride, g.pad))


_NO_SHAPE = (0,) * 10


def _launch(name, cost, fn):
    """Run one kernel launch; under a KernelProfile bracket it with two event records (see KernelProfile).
    ``cost`` = (algorithmic flops, algorithmic bytes, shape key)."""
    if _PROFILE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    _PROFILE.records.append((name, cost[0], cost[1], (e0, e1), cost[2]))


PAIR_GEMMS = True          # tests / A-B measurements: False = ``gemm_batch`` launches every GEMM on its own, at once
_GEMM_BATCH = None
GEMM_BATCH_SLOTS = 4


class gemm_batch:
    """``with ops.gemm_batch():`` -- the ``conv_fwd`` / ``conv_bwd_data`` calls made inside are RECORDED (include/ali_hip.h:
    AliGemmJob) and issued together when the block ends: one launch per kernel variant instead of one per call.  The
    calls of one block must be mutually independent and nothing inside the block may read a result of one of them
    (``chain.run_parallel`` advances independent layer chains one GEMM at a time under such a block).  Each recorded
    job works in a workspace slab of its own.  Launches of a kind no multi-job kernel exists for go out at once."""

    def __init__(self):
        self.jobs, self.keep, self.after = [], [], []
        self.flops = self.bytes = 0.0

    def __enter__(self):
        global _GEMM_BATCH
        self.prev, _GEMM_BATCH = _GEMM_BATCH, (self if PAIR_GEMMS else None)
        return self

    def __exit__(self, *exc):
        global _GEMM_BATCH
        _GEMM_BATCH = self.prev
        if exc[0] is None:
            self.flush()

    def flush(self):
        if self.jobs:
            n = len(self.jobs)
            arr = (_lib.AliGemmJob * n)(*self.jobs)

            def go():
                _lib.check(_lib.load().ali_gemm_launch_multi(n, arr, _stream()), "ali_gemm_launch_multi")
            _launch("gconv", (self.flops, self.bytes, _NO_SHAPE), go)
        todo = self.after
        self.jobs, self.keep, self.after, self.flops, self.bytes = [], [], [], 0.0, 0.0
        for fn in todo:
            fn()


def _gemm(which, name, g, a, w_packed, out, ep, in_ld, out_ld, live):
    """one forward (which = 0) / data-gradient (1) GEMM: launched, or recorded into the open ``gemm_batch``"""
    lib = _lib.load()
    ep.in_ld, ep.out_ld = in_ld, out_ld
    _f16_operands(g, which, a, w_packed, out, ep)
    _set_tile_order(g, which, ep, a.device)
    cost = _geom_cost(g, live)
    kind = "fwd" if which == 0 else "bwd_data"
    hook = _HOOK
    b = _GEMM_BATCH
    if b is not None and len(b.jobs) >= GEMM_BATCH_SLOTS:
        b.flush()
    if b is None:
        ws = workspace(a.device)
        fn = lib.ali_conv_fwd if which == 0 else lib.ali_conv_bwd_data

        def go():
            _lib.check(fn(byref(g), _view_ptr(a, in_ld, "a"), _chk(w_packed, "w"), _view_ptr(out, out_ld, "out"),
                          byref(ep), c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_conv_" + kind)
        _launch(name, cost, go)
        if hook is not None:
            hook.gemm(kind, g, a, w_packed, out, ep, in_ld, out_ld)
        return out
    ws = workspace(a.device, 1 + len(b.jobs))
    job = _lib.AliGemmJob()
    fn = lib.ali_conv_fwd_job if which == 0 else lib.ali_conv_bwd_data_job
    ev = None
    if _PROFILE is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _lib.check(fn(byref(g), _view_ptr(a, in_ld, "a"), _chk(w_packed, "w"), _view_ptr(out, out_ld, "out"), byref(ep),
                  c_void_p(ws.data_ptr()), ws.numel(), byref(job), _stream()), "ali_conv_" + kind + "_job")
    if job.opaque[0] == 1:
        b.jobs.append(job)
        b.keep.append((a, w_packed, out, ep, ws))
        b.flops += cost[0]
        b.bytes += cost[1]
        if hook is not None:
            b.after.append(lambda: hook.gemm(kind, g, a, w_packed, out, ep, in_ld, out_ld))
    else:                               # a launch of another kind: it went out right away
        if ev is not None:
            ev[1].record()
            _PROFILE.records.append((name, cost[0], cost[1], ev, cost[2]))
        if hook is not None:
            hook.gemm(kind, g, a, w_packed, out, ep, in_ld, out_ld)
    return out


def shadow16(t):
    """the fp16 twin a tensor carries (set by the fp16-MFMA launch that produced it, or by ``ensure_shadow16``)"""
    h = getattr(t, "_ali16", None)
    if h is not None and (h.shape != t.shape or h.device != t.device):
        return None
    return h


_TWIN_OF = {}          # data_ptr of a packed-weight tensor -> weakref of its fp16 twin (the pack kernel writes both)
_TWIN_WRITTEN = set()  # data_ptrs whose twin the pending / last pack launch wrote: no separate re-rounding needed


def ensure_shadow16(t):
    """fp16 twin of a (weight) tensor, created once and kept on the tensor object; ``refresh_shadow16`` re-rounds it
    in place after the tensor changed (fixed addresses: captured graphs stay valid)."""
    import weakref
    h = shadow16(t)
    if h is None:
        h = t.detach().to(torch.float16)
        t._ali16 = h
        if len(_TWIN_OF) > 4096:
            for k in [k for k, r in _TWIN_OF.items() if r() is None]:
                del _TWIN_OF[k]
        _TWIN_OF[t.data_ptr()] = weakref.ref(h)
    return h


def refresh_shadow16(t):
    h = shadow16(t)
    if h is None:
        return
    if t.data_ptr() in _TWIN_WRITTEN:          # the pack launch that rewrote t wrote the twin as well
        _TWIN_WRITTEN.discard(t.data_ptr())
        return
    h.copy_(t.detach())


def _twin_for_pack(dst):
    r = _TWIN_OF.get(dst.data_ptr())
    h = r() if r is not None else None
    if h is not None and h.numel() == dst.numel() and h.device == dst.device:
        return h
    return None


def _f16_operands(g, which, x, w_packed, y, ep):
    """fp16 twins for a precision("f16") launch: read them where both operands have one, leave one of the output.
    (Column-range operands -- in_ld / out_ld -- neither read nor leave twins.)"""
    if not _PRECISION["f16"]:
        return
    x16, w16 = (None if ep.in_ld else shadow16(x)), shadow16(w_packed)
    if x16 is not None and w16 is not None:
        ep.in16, ep.w16 = c_void_p(x16.data_ptr()), c_void_p(w16.data_ptr())
    if not ep.out_ld and _lib.load().ali_conv_writes_out16(byref(g), which):
        y16 = shadow16(y)                # (a persistent output buffer keeps its twin: fixed addresses for captured graphs)
        if y16 is None or y16.dtype != torch.float16:
            y16 = torch.empty(y.shape, dtype=torch.float16, device=y.device)
        ep.out16 = c_void_p(y16.data_ptr())
        y._ali16 = y16


_TILE_ORDER = {}


def conv_tile_order(g: AliConvGeom, which: int, device):
    """Cached device table of the launch's M-tile ids, longest k-loop first (include/ali_hip.h: ali_conv_tile_order),
    or None when every tile costs the same.  Built on the host: a miss while the stream is capturing returns None
    (the eager warm-up iteration in front of every capture fills the cache)."""
    f16 = int(_PRECISION["f16"])
    key = (device.index, which, f16) + tuple(getattr(g, n) for n, _ in AliConvGeom._fields_)
    if key in _TILE_ORDER:
        return _TILE_ORDER[key]
    if torch.cuda.is_current_stream_capturing():
        return None
    cap = 1 << 16
    buf = (ctypes.c_int32 * cap)()
    n = _lib.load().ali_conv_tile_order(byref(g), which, f16, ctypes.cast(buf, c_void_p), cap)
    tab = torch.tensor(list(buf[:n]), dtype=torch.int32, device=device) if n > 0 else None
    _TILE_ORDER[key] = tab
    return tab


def _set_tile_order(g, which, ep, device):
    tab = conv_tile_order(g, which, device)
    if tab is not None:
        ep.tile_order, ep.tile_order_n = tab.data_ptr(), tab.numel()


def _view_ptr(t, ld, name):
    """pointer of a dense tensor (ld == 0) or of a column range of rows ``ld`` floats apart (a strided view)"""
    return _ptr(t) if ld else _chk(t, name)


def conv_fwd(g: AliConvGeom, x, w_packed, y, ep: AliEpilogue, in_ld=0, out_ld=0, live=None):
    """``in_ld`` / ``out_ld`` > 0: ``x`` / ``y`` are column ranges (strided views) of wider row-major buffers whose
    pixels are that many floats apart (AliEpilogue.in_ld / out_ld).  ``live`` = (channels of x, channels of y) that
    carry data when a stride is padded: accounting only (``_geom_cost``)."""
    return _gemm(0, "gconv", g, x, w_packed, y, ep, in_ld, out_ld, live)


def conv_bwd_data(g: AliConvGeom, dy, w_packed, dx, ep: AliEpilogue, in_ld=0, out_ld=0, live=None):
    return _gemm(1, "gconv_t", g, dy, w_packed, dx, ep, in_ld, out_ld, live)


_PIXTAB = {}


def wgrad_pixtab(g: AliConvGeom, device):
    """Cached per-geometry pixel table of the weight-gradient kernel (include/ali_hip.h: ali_wgrad_pixtab)."""
    key = (device.index, g.B, g.H, g.W, g.C, g.P, g.Q, g.stride, g.pad)
    tab = _PIXTAB.get(key)
    if tab is None:
        if len(_PIXTAB) > 256:
            _PIXTAB.clear()
        tab = torch.empty(2 * g.B * g.P * g.Q, dtype=torch.int32, device=device)
        _lib.check(_lib.load().ali_wgrad_pixtab(byref(g), c_void_p(tab.data_ptr()), _stream()), "ali_wgrad_pixtab")
        _PIXTAB[key] = tab
    return tab


_DEFERRABLE = {}


def wgrad_deferrable(g: AliConvGeom) -> int:
    f16 = int(_PRECISION["f16"])
    key = (f16,) + tuple(getattr(g, n) for n, _ in AliConvGeom._fields_)
    hit = _DEFERRABLE.get(key)
    if hit is None:
        hit = _DEFERRABLE[key] = int(_lib.load().ali_wgrad_deferrable(byref(g), f16))
    return hit


DEFER_WGRAD_LAUNCH = True     # tests / A-B measurements: False = every weight-gradient GEMM is its own launch


class FoldQueue:
    """Deferred slab reductions of the weight-gradient launches of one backward pass (include/ali_hip.h: AliWgradFold):
    ``conv_bwd_weight(..., defer=queue)`` gives each launch its own region of the queue's arena and skips the second
    (reduction) launch; ``flush()`` folds them all at once.  The arena is allocated once per device and shared (one
    backward pass is in flight at a time; captured graphs keep pointing into it)."""
    _arena = {}
    arena_bytes = 512 << 20

    def __init__(self, device):
        self.device = device
        self.jobs = []          # deferred slab reductions
        self.launches = []      # deferred GEMM launches (AliWgradJob) ...
        self.keep = []          # ... and the tensors they read / write, alive until flush
        self.off = 0
        self.flops = 0.0
        self.bytes = 0.0
        self.n_jobs = 1         # deferrable launches of the pass in progress (expect()): what a combined launch will hold
        self.after_flush = []   # launch_hook callbacks of deferred weight gradients (tests)

    def arena(self):
        a = FoldQueue._arena.get(self.device.index)
        if a is None or a.numel() * 4 < FoldQueue.arena_bytes:
            a = FoldQueue._arena[self.device.index] = torch.zeros(FoldQueue.arena_bytes // 4, dtype=torch.float32,
                                                                   device=self.device)
        return a

    def expect(self, geoms):
        """Called before a pass's first weight gradient with the geometries of all of them: the number of launches the
        pass will combine decides how far each is split (a function of the pass alone -- not of what ran before)."""
        self.n_jobs = max(1, sum(wgrad_deferrable(g) for g in geoms))

    def abandon(self):
        """forget recorded work without launching it (an iteration that raised half-way)"""
        self.jobs, self.launches, self.keep, self.flops, self.bytes, self.off = [], [], [], 0.0, 0.0, 0
        self.after_flush = []

    def split_target(self):
        """blocks a deferred GEMM should split into: about 2048 in the whole combined launch"""
        return max(256, min(1024, 2048 // self.n_jobs))

    def flush(self):
        if self.launches:
            arr = (_lib.AliWgradJob * len(self.launches))(*self.launches)
            n = len(self.launches)

            def go_l():
                _lib.check(_lib.load().ali_wgrad_launch_multi(n, arr, _stream()), "ali_wgrad_launch_multi")
            _launch("wgrad_multi", (self.flops, self.bytes, _NO_SHAPE), go_l)
        self.launches, self.keep, self.flops, self.bytes = [], [], 0.0, 0.0
        if self.jobs:
            arr = (_lib.AliWgradFold * len(self.jobs))(*self.jobs)
            n = len(self.jobs)

            def go():
                _lib.check(_lib.load().ali_wgrad_fold_multi(n, arr, _stream()), "ali_wgrad_fold_multi")
            _launch("wgrad_fold", (0.0, 0.0, _NO_SHAPE), go)
        self.jobs, self.off = [], 0
        todo, self.after_flush = self.after_flush, []
        for fn in todo:
            fn()


def conv_bwd_weight(g: AliConvGeom, x, dy, dst, cg_log, cd_log, s_dc, s_gc, s_tap, db=None, dy_ld=0, defer=None):
    """``db`` (optional, [cd_log]): also produce the column sums of ``dy`` (Conv2d bias gradient) in the same launch.
    ``dy_ld`` > 0: ``dy`` is a column range (a strided view) of rows that are ``dy_ld`` floats apart.
    ``defer`` (FoldQueue): leave the slab reduction of a split launch to ``defer.flush()``."""
    lib = _lib.load()
    ws = workspace(x.device)
    tab = wgrad_pixtab(g, x.device) if (g.C % 4 == 0 and g.K % 4 == 0) else None
    f16 = int(_PRECISION["f16"])
    x16, dy16 = (shadow16(x), shadow16(dy)) if (f16 and not dy_ld) else (None, None)
    if x16 is None or dy16 is None:
        x16 = dy16 = None
    ws_ptr, ws_n, job, lj = ws.data_ptr(), ws.numel(), None, None
    if defer is not None:
        arena = defer.arena()
        left = arena.numel() * 4 - defer.off
        if left >= (32 << 20):                    # a region of its own (else: the shared workspace, immediate fold)
            ws_ptr, ws_n, job = arena.data_ptr() + defer.off, left, _lib.AliWgradFold()
            if DEFER_WGRAD_LAUNCH:
                lj = _lib.AliWgradJob()

    def go():
        _lib.check(lib.ali_conv_bwd_weight(byref(g), _chk(x, "x"), _ptr(dy) if dy_ld else _chk(dy, "dy"),
                                           _ptr(dst), cg_log, cd_log,        # (dst: any strides, see s_dc / s_gc / s_tap)
                                           s_dc, s_gc, s_tap, _opt(db, "db"),
                                           None if tab is None else c_void_p(tab.data_ptr()), f16,
                                           None if x16 is None else c_void_p(x16.data_ptr()),
                                           None if dy16 is None else c_void_p(dy16.data_ptr()), dy_ld,
                                           None if job is None else byref(job), None if lj is None else byref(lj),
                                           0 if lj is None else defer.split_target(),
                                           c_void_p(ws_ptr), ws_n, _stream()), "ali_conv_bwd_weight")
    cost = _geom_cost(g, (cg_log, cd_log))
    if lj is None:
        _launch("wgrad", cost, go)
    else:                     # records the job, or -- a launch of another kind (large tiles, fp16) -- runs it right away
        ev = None
        if _PROFILE is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        go()
        if lj.opaque[0] == 1:
            defer.launches.append(lj)
            defer.keep.append((x, dy, dst, db, tab))
            defer.flops += cost[0]
            defer.bytes += cost[1]
        elif ev is not None:
            ev[1].record()
            _PROFILE.records.append(("wgrad", cost[0], cost[1], ev, cost[2]))
    deferred = job is not None and job.S > 0
    if deferred:
        defer.jobs.append(job)
        defer.off += (int(job.ws_used) + 255) // 256 * 256
    if _HOOK is not None:
        done = _HOOK.wgrad(g, x, dy, dst, cg_log, cd_log, (s_dc, s_gc, s_tap), db, dy_ld)
        if done is not None:
            if deferred or (lj is not None and lj.opaque[0] == 1):
                defer.after_flush.append(done)
            else:
                done()
    return dst


def _ptr(t):
    """raw pointer of a (possibly strided) fp32 CUDA view"""
    if not (t.is_cuda and t.dtype == torch.float32):
        raise ValueError("need an fp32 CUDA tensor")
    return c_void_p(t.data_ptr())


def tconv1_fwd(big, w_tk, bias, out, B, P, Q, K, R, S, pad, ostride, act, slope, rowscale=None):
    """``rowscale``: optional [B] view (any stride) of per-sample factors applied to the output."""
    lib = _lib.load()

    def go():
        _lib.check(lib.ali_tconv1_fwd(_chk(big, "big"), _chk(w_tk, "w"), None if bias is None else _ptr(bias),
                                      _ptr(out), B, P, Q, K, R, S, pad, ostride, act, slope,
                                      None if rowscale is None else _ptr(rowscale),
                                      0 if rowscale is None else rowscale.stride(0), _stream()),
                   "ali_tconv1_fwd")
    _launch("tconv1_fwd", (2.0 * B * P * Q * K * R * S, 4.0 * B * (P * Q * K + (P + R - 1 - 2 * pad) * (Q + S - 1 - 2 * pad)), _NO_SHAPE), go)
    return out


def tconv1_dgrad(small, sstride, w_tk, dact_y, dact, dslope, gbig, B, P, Q, K, R, S, pad):
    lib = _lib.load()

    def go():
        _lib.check(lib.ali_tconv1_dgrad(_ptr(small), sstride, _chk(w_tk, "w"), _opt(dact_y), dact, dslope,
                                        _chk(gbig, "gbig"), B, P, Q, K, R, S, pad, _stream()), "ali_tconv1_dgrad")
    _launch("tconv1_dgrad", (2.0 * B * P * Q * K * R * S, 4.0 * B * (2 * P * Q * K + (P + R - 1 - 2 * pad) * (Q + S - 1 - 2 * pad)), _NO_SHAPE), go)
    return gbig


def tconv1_wgrad(big, small, sstride, nc, dw, s_k, s_tap, s_c, B, P, Q, K, R, S, pad):
    lib = _lib.load()
    ws = workspace(big.device)

    def go():
        _lib.check(lib.ali_tconv1_wgrad(_chk(big, "big"), _ptr(small), sstride, nc, _ptr(dw), s_k, s_tap, s_c, B, P,
                                        Q, K, R, S, pad, c_void_p(ws.data_ptr()), ws.numel(), _stream()),
                   "ali_tconv1_wgrad")
    _launch("tconv1_wgrad", (2.0 * B * P * Q * K * R * S * nc, 4.0 * B * (P * Q * K + nc * (P + R - 1 - 2 * pad) * (Q + S - 1 - 2 * pad)), _NO_SHAPE), go)
    return dw


_T1_OPS = {"fwd": 0, "dgrad": 1, "wgrad": 2}


def tconv1_route(op, B, P, Q, K, R, S, pad, nc=1, ws_bytes=None):
    """The kernel ``tconv1_fwd`` / ``tconv1_dgrad`` / ``tconv1_wgrad`` (``op``: "fwd", "dgrad", "wgrad") launches for a
    shape, by the instantiation's name -- "fwd_mfma<2,4>", "fwd<16,4>", "dgrad_band<9>", "dgrad<25>", "wgrad_mfma<1,8>",
    "wgrad_rb<5,3>", "wgrad<7>" -- or None when the launch refuses the shape (ALI_T1_* of include/ali_hip.h).  ``nc``
    and ``ws_bytes`` (default: the workspace every launch gets) matter to the weight gradient only.  Host arithmetic of
    the library: needs no GPU."""
    ws_bytes = _WS_BYTES if ws_bytes is None else int(ws_bytes)
    code = _lib.load().ali_tconv1_route(_T1_OPS[op], B, P, Q, K, R, S, pad, nc, ws_bytes)
    if code < 0:
        return None
    fam, arg = divmod(code, 1000)
    if fam == 1:
        return f"fwd_mfma<{arg // 10},{arg % 10}>"
    if fam == 2:
        return f"fwd<{arg * arg},{arg}>"
    if fam in (3, 4):
        return f"{'dgrad_band' if fam == 3 else 'dgrad'}<{arg}>"
    if fam == 5:
        return f"wgrad_mfma<{arg},8>"
    if fam == 6:
        return f"wgrad_rb<{arg // 10},{arg % 10}>"
    if fam == 7:
        return f"wgrad<{arg}>"
    raise ValueError(f"ali_tconv1_route: unknown route code {code}")


_PACK_BATCH = None
_PACK_AFTER = []          # callbacks to run once the pending pack jobs have been launched (fp16 twins of the packs)


def after_packs(fn):
    """Run ``fn`` now, or -- inside ``batched_packs`` -- right after the collected pack jobs have been launched."""
    if _PACK_BATCH is None:
        fn()
    else:
        _PACK_AFTER.append(fn)


class batched_packs:
    """Collect the ``pack_weights`` calls issued inside the block and run them as ONE launch (at most 40 jobs per
    launch; a job that reads the destination of a pending job flushes first)."""

    def __enter__(self):
        global _PACK_BATCH
        self.prev, _PACK_BATCH = _PACK_BATCH, []
        return self

    def __exit__(self, *exc):
        global _PACK_BATCH
        _flush_packs()
        _PACK_BATCH = self.prev
        if self.prev is None:
            todo, _PACK_AFTER[:] = list(_PACK_AFTER), []
            for fn in todo:
                fn()


def _launch_packs(jobs):
    """jobs: (src, dst, N, T, C, Cpad, s_n, s_tap, s_c) tuples; one launch per 40 (include/ali_hip.h)."""
    lib = _lib.load()
    for lo in range(0, len(jobs), 40):
        part = jobs[lo:lo + 40]
        n = len(part)
        twins = [_twin_for_pack(j[1]) for j in part]
        srcs = (c_void_p * n)(*[j[0].data_ptr() for j in part])
        dsts = (c_void_p * n)(*[j[1].data_ptr() for j in part])
        d16 = (c_void_p * n)(*[None if h is None else h.data_ptr() for h in twins])
        dims = (ctypes.c_int32 * (4 * n))(*[v for j in part for v in j[2:6]])
        strides = (ctypes.c_int64 * (3 * n))(*[v for j in part for v in j[6:9]])
        _lib.check(lib.ali_pack_weights_multi(n, srcs, dsts, d16, dims, strides, _stream()), "ali_pack_weights_multi")
        for j, h in zip(part, twins):
            if h is not None:
                _TWIN_WRITTEN.add(j[1].data_ptr())


def _flush_packs():
    jobs = _PACK_BATCH
    if not jobs:
        return
    _launch_packs(jobs)
    jobs.clear()


def pack_weights(src, dst, N, T, C, Cpad, s_n, s_tap, s_c):
    _chk(src, "src"), _chk(dst, "dst")
    if _PACK_BATCH is not None:
        if any(j[1].data_ptr() == src.data_ptr() for j in _PACK_BATCH):
            _flush_packs()
        _PACK_BATCH.append((src, dst, N, T, C, Cpad, s_n, s_tap, s_c))
        return dst
    _launch_packs([(src, dst, N, T, C, Cpad, s_n, s_tap, s_c)])
    return dst


def head_fwd(x2d, w, bias, y):
    """y[b] = bias + x2d[b, :] @ w  (the Discriminator's Conv2d(C, 1, 1) head; include/ali_hip.h: ali_head_fwd)"""
    B, C = x2d.shape
    _lib.check(_lib.load().ali_head_fwd(_ptr(x2d), x2d.stride(0), _chk(w, "w"), _opt(bias, "bias"), _chk(y, "y"), B, C,
                                        _stream()), "ali_head_fwd")
    return y


def head_wgrad(x2d, g, dw, db=None):
    """dw[c] = sum_b g[b] * x2d[b, c], db = sum_b g[b]  (include/ali_hip.h: ali_head_wgrad)"""
    B, C = x2d.shape
    _lib.check(_lib.load().ali_head_wgrad(_ptr(x2d), x2d.stride(0), _chk(g, "g"), _chk(dw, "dw"), _opt(db, "db"), B, C,
                                          _stream()), "ali_head_wgrad")
    return dw


def switched_off(name: str) -> bool:
    """Is the A/B switch ``name`` (ALI_NO_HEAD_BWD, ALI_NO_GZ_CHAIN: routes chosen on the Python side)
    set?  Read from the environment at every decision, so ``ops.tuning(ALI_NO_HEAD_BWD=1)`` holds for its block."""
    import os
    return os.environ.get(name, "0") not in ("", "0")


def head_bwd(gl, w, y_prev, dact, dslope, mask, g, x2d=None, dw=None, db=None):
    """The head's backward pass in one launch (include/ali_hip.h: ali_head_bwd): g[b, c] = gl[b] * w[c] * mask[b, c] *
    act'(y_prev[b, c]) into the dense [B, C] ``g``; with ``dw`` also dw[c] = sum_b gl[b] * x2d[b, c] and db = sum_b gl[b].
    ``mask`` ([B, C]) and ``x2d`` may be column ranges of wider buffers (any row stride); ``y_prev`` (dense [B, C];
    needed when ``dact`` is an activation) and ``mask`` may be None."""
    B, C = g.shape
    if gl.numel() != B or w.numel() != C or (y_prev is not None and y_prev.numel() != B * C):
        raise ValueError("head_bwd: operand shapes do not match g [B, C]")
    if dw is not None and (x2d is None or tuple(x2d.shape) != (B, C) or x2d.stride(1) != 1 or dw.numel() != C):
        raise ValueError("head_bwd: dw needs x2d [B, C] with unit column stride and C weights")
    if mask is not None and (mask.shape[0] != B or mask.shape[1] < C or mask.stride(1) != 1):
        raise ValueError("head_bwd: mask must be [B, >= C] with unit column stride")
    ws = workspace(g.device)
    _lib.check(_lib.load().ali_head_bwd(_chk(gl, "gl"), _chk(w, "w"), _opt(y_prev, "y_prev"), dact, dslope,
                                        None if mask is None else _ptr(mask), 0 if mask is None else mask.stride(0),
                                        _chk(g, "g"),
                                        None if dw is None else _ptr(x2d), 0 if dw is None else x2d.stride(0),
                                        _opt(dw, "dw"), _opt(db, "db"), B, C, c_void_p(ws.data_ptr()), ws.numel(),
                                        _stream()), "ali_head_bwd")
    return g


def copy_multi(pairs):
    """[(dst, src), ...]: dst.copy_(src) for all pairs -- same-dtype contiguous CUDA pairs share one launch
    (include/ali_hip.h: ali_copy_multi), anything else falls back to Tensor.copy_."""
    fast = []
    for dst, src in pairs:
        if (dst.is_cuda and src.is_cuda and dst.device == src.device and dst.dtype == src.dtype and dst.shape == src.shape
                and dst.is_contiguous() and src.is_contiguous() and dst.element_size() % 4 == 0 and dst.numel() > 0):
            fast.append((dst, src))
        else:
            dst.copy_(src)
    if fast:
        n = len(fast)
        srcs = (c_void_p * n)(*[s_.data_ptr() for _, s_ in fast])
        dsts = (c_void_p * n)(*[d_.data_ptr() for d_, _ in fast])
        sizes = (ctypes.c_int64 * n)(*[d_.numel() * d_.element_size() for d_, _ in fast])
        _lib.check(_lib.load().ali_copy_multi(n, srcs, dsts, sizes, _stream()), "ali_copy_multi")


def act_bwd(gy, y, act, slope, out=None):
    lib = _lib.load()
    out = torch.empty_like(gy) if out is None else out
    _lib.check(lib.ali_act_bwd(_chk(gy, "gy"), _chk(y, "y"), _chk(out), gy.numel(), act, slope, _stream()),
               "ali_act_bwd")
    return out


def colsum(x2d_rows, C, ld, x, out=None):
    lib = _lib.load()
    ws = workspace(x.device)
    out = torch.empty(C, dtype=torch.float32, device=x.device) if out is None else out
    _lib.check(lib.ali_colsum(_chk(x, "x"), x2d_rows, C, ld, _chk(out), c_void_p(ws.data_ptr()), ws.numel(),
                              _stream()), "ali_colsum")
    return out


def rowmask_mul(x, mask, B, rows_per_img, C, out=None):
    lib = _lib.load()
    out = torch.empty_like(x) if out is None else out
    _lib.check(lib.ali_rowmask_mul(_chk(x, "x"), _chk(mask, "mask"), _chk(out), B, rows_per_img, C, _stream()),
               "ali_rowmask_mul")
    return out


def _rng_args(seed, ctr, offset=0):
    """(seed, counter pointer, offset) as the launchers of the counter RNG take them (csrc/ali_rng.h): seed and offset
    reduced to 64 bits, the counter None or a one-element int64 CUDA tensor"""
    if ctr is not None and not (torch.is_tensor(ctr) and ctr.is_cuda and ctr.dtype == torch.int64 and ctr.numel() == 1):
        raise ValueError("need a one-element int64 CUDA tensor as device counter")
    return int(seed) & (2 ** 64 - 1), None if ctr is None else c_void_p(ctr.data_ptr()), int(offset) & (2 ** 64 - 1)


def dropout_mask(seed, offset, p, B, C, device, dev_counter=None):
    seed, ctr, offset = _rng_args(seed, dev_counter, offset)
    out = torch.empty(B, C, dtype=torch.float32, device=device)
    _lib.check(_lib.load().ali_dropout_mask(seed, offset, ctr, p, _chk(out), out.numel(), _stream()), "ali_dropout_mask")
    return out


def dropout_mask_multi(seed, dev_counter, seg_end, seg_p, seg_clog, seg_cpad, out):
    """one launch for all masks of an iteration; seg_* are host lists (see ali_hip.h)."""
    n = len(seg_end)
    ends = (ctypes.c_int64 * n)(*seg_end)
    ps = (ctypes.c_float * n)(*seg_p)
    cl = (ctypes.c_int32 * n)(*seg_clog)
    cp = (ctypes.c_int32 * n)(*seg_cpad)
    _lib.check(_lib.load().ali_dropout_mask_multi(*_rng_args(seed, dev_counter)[:2], ends, ps, cl, cp, n, _chk(out),
                                                  _stream()), "ali_dropout_mask_multi")
    return out


def normal_fill(seed, out, dev_counter=None, offset=0):
    """out (contiguous fp32 CUDA, any shape, 4-byte aligned: slices are fine) <- N(0,1) draws ``offset .. offset +
    numel`` of the latent stream keyed by (seed, *dev_counter) (include/ali_hip.h: ali_normal_fill;
    ``ali_hip.source.normal_reference`` gives the same values on the host)."""
    _lib.check(_lib.load().ali_normal_fill(*_rng_args(seed, dev_counter, offset), _chk(out, "out"), out.numel(),
                                           _stream()), "ali_normal_fill")
    return out


def batch_gather(images, attrs, n_cls, index, lo, hi, out=None):
    """One batch of a device-resident data set: rows ``index`` ([B] int64 CUDA) of ``images`` [N, H*W] (uint8 or fp32)
    and ``attrs`` [N, n_cls + n_cont] fp32, scaled like ``image_scms.mnist._scale_batch`` -- (images [B, H*W], one-hot
    rows [B, n_cls], idx [B, 1] int32, cont [B, n_cont] or None), one launch (include/ali_hip.h: ali_batch_gather).
    ``out``: the same four tensors to write into."""
    for t, dt, name in ((images, (torch.uint8, torch.float32), "images"), (attrs, (torch.float32,), "attrs"),
                        (index, (torch.int64,), "index")):
        if not (t.is_cuda and t.is_contiguous() and t.dtype in dt):
            raise ValueError(f"batch_gather: {name} must be a contiguous CUDA tensor of dtype {dt}, got {t.dtype} "
                             f"{t.device}")
    N, HW = images.shape
    B, n_cont = index.numel(), attrs.shape[1] - n_cls
    if attrs.shape[0] != N or n_cls < 1 or n_cont < 0 or (n_cont and (lo.numel() != n_cont or hi.numel() != n_cont)):
        raise ValueError("batch_gather: attrs / lo / hi do not fit the images and n_cls")
    dev = images.device
    if out is None:
        out = (torch.empty(B, HW, dtype=torch.float32, device=dev), torch.empty(B, n_cls, dtype=torch.float32, device=dev),
               torch.empty(B, 1, dtype=torch.int32, device=dev),
               torch.empty(B, n_cont, dtype=torch.float32, device=dev) if n_cont else None)
    x, onehot, idx, cont = out
    _lib.check(_lib.load().ali_batch_gather(
        c_void_p(images.data_ptr()), int(images.dtype == torch.uint8), _chk(attrs, "attrs"), attrs.shape[1],
        c_void_p(index.data_ptr()), _chk(lo, "lo") if n_cont else None, _chk(hi, "hi") if n_cont else None, N, HW, n_cls,
        n_cont, B, _chk(x, "out images"), _chk(onehot, "out one-hot"), c_void_p(idx.data_ptr()), _opt(cont, "out cont"),
        _stream()), "ali_batch_gather")
    return x, onehot, idx, cont


def bn_stats(x, mask, B, rows_per_img, C, gamma, beta, running_mean, running_var, momentum, eps, training, groups=1):
    """Returns st [4, C] (mean, invstd, sc, sh), or [groups, 4, C] for ``groups`` batched passes."""
    lib = _lib.load()
    ws = workspace(x.device)
    st = torch.empty(groups, 4, C, dtype=torch.float32, device=x.device)
    _lib.check(lib.ali_bn_stats(_chk(x, "x"), _opt(mask), B, rows_per_img, C, _opt(gamma), _opt(beta),
                                _opt(running_mean), _opt(running_var), momentum, eps, int(training),
                                c_void_p(st[0, 0].data_ptr()), c_void_p(st[0, 1].data_ptr()),
                                c_void_p(st[0, 2].data_ptr()), c_void_p(st[0, 3].data_ptr()), groups, 4 * C,
                                c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_bn_stats")
    return st[0] if groups == 1 else st


def bn_stats_from_partials(part, slots, groups, C, count, gamma, beta, running_mean, running_var, momentum, eps):
    """bn_stats (training mode) from the per-tile partial sums a convolution epilogue left in ``part``."""
    lib = _lib.load()
    st = torch.empty(groups, 4, C, dtype=torch.float32, device=part.device)
    _lib.check(lib.ali_bn_stats_from_partials(_chk(part, "part"), slots, groups, C, count, _opt(gamma), _opt(beta),
                                              _opt(running_mean), _opt(running_var), momentum, eps,
                                              c_void_p(st[0, 0].data_ptr()), c_void_p(st[0, 1].data_ptr()),
                                              c_void_p(st[0, 2].data_ptr()), c_void_p(st[0, 3].data_ptr()), 4 * C,
                                              _stream()), "ali_bn_stats_from_partials")
    return st[0] if groups == 1 else st


def bn_bwd_from_partials(part, slots, x, g, mask_in, mask_pre, st, gamma, B, rows_per_img, C, batch_stats, slope,
                         want_gx=True, out_dgamma=None, out_dbeta=None):
    """bn_bwd from the per-tile partial sums the data-gradient GEMM's epilogue left in ``part``."""
    lib = _lib.load()
    if out_dgamma is None or out_dbeta is None:
        dg = torch.empty(2, C, dtype=torch.float32, device=x.device)
        out_dgamma, out_dbeta = dg[0], dg[1]
    gx = torch.empty_like(x) if want_gx else None
    _lib.check(lib.ali_bn_bwd_from_partials(_chk(part, "part"), slots, _chk(x, "x"), _chk(g, "g"), _opt(mask_in),
                                            _opt(mask_pre), c_void_p(st[0].data_ptr()), c_void_p(st[1].data_ptr()),
                                            _opt(gamma), B, rows_per_img, C, int(batch_stats), float(slope),
                                            _chk(out_dgamma, "dgamma"), _chk(out_dbeta, "dbeta"), _opt(gx), _stream()),
               "ali_bn_bwd_from_partials")
    return out_dgamma, out_dbeta, gx


def bn_apply(x, st, mask_in, mask_post, B, rows_per_img, C, out=None, groups=1):
    lib = _lib.load()
    out = torch.empty_like(x) if out is None else out
    st0 = st if groups == 1 else st[0]
    _lib.check(lib.ali_bn_apply(_chk(x, "x"), c_void_p(st0[2].data_ptr()), c_void_p(st0[3].data_ptr()), _opt(mask_in),
                                _opt(mask_post), _chk(out), B, rows_per_img, C, groups, 4 * C, _stream()),
               "ali_bn_apply")
    return out


def bn_bwd(x, g, mask_in, mask_pre, st, gamma, B, rows_per_img, C, batch_stats, slope, want_gx=True, out_dgamma=None,
           out_dbeta=None):
    """returns (dgamma, dbeta, gx); out_dgamma / out_dbeta: optional contiguous [C] destinations."""
    lib = _lib.load()
    ws = workspace(x.device)
    if out_dgamma is None or out_dbeta is None:
        dg = torch.empty(2, C, dtype=torch.float32, device=x.device)
        out_dgamma, out_dbeta = dg[0], dg[1]
    gx = torch.empty_like(x) if want_gx else None
    _lib.check(lib.ali_bn_bwd(_chk(x, "x"), _chk(g, "g"), _opt(mask_in), _opt(mask_pre), c_void_p(st[0].data_ptr()),
                              c_void_p(st[1].data_ptr()), _opt(gamma), B, rows_per_img, C, int(batch_stats),
                              float(slope), _chk(out_dgamma, "dgamma"), _chk(out_dbeta, "dbeta"), _opt(gx),
                              c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_bn_bwd")
    return out_dgamma, out_dbeta, gx


_EW_OPS = {"bn_stats": 0, "bn_apply": 1, "bn_bwd": 2, "bn_bwd_from_partials": 3, "colsum": 4, "act_bwd": 5}


def ew_plan(op, rows_per_group, rows_per_img, C, ld=None, groups=1, aligned=True):
    """(route, reduce_blocks, apply_blocks) the entry ``ali_<op>`` launches for a shape (include/ali_hip.h:
    ali_ew_plan): route "vec" (float4 kernels) or "scalar", reduction blocks per group and blocks of the element-wise
    pass (0 where the entry runs no such pass) -- or None when the launch refuses the shape.  ``ld`` (colsum's row
    stride) defaults to C; ``aligned``: every tensor operand the entry names is 16-byte aligned.  Host arithmetic of the
    library: needs no GPU."""
    blocks = (ctypes.c_int32 * 2)(0, 0)
    code = _lib.load().ali_ew_plan(_EW_OPS[op], rows_per_group, rows_per_img, C, C if ld is None else ld, groups,
                                   int(bool(aligned)), blocks)
    if code < 0:
        return None
    return ("vec" if code == 1 else "scalar"), blocks[0], blocks[1]


def plane_table_grad(g, g_ch, x0, x_ch, idx, idx_col, n_rows, out=None, table=None):
    """Embedding-table gradient from the gradient ``g`` [B,H,W,Cg] of the assembled planes ``x0`` [B,H,W,Cx]
    (include/ali_hip.h: ali_plane_table_grad).  Returns / fills ``out`` [n_rows, 256].  ``table`` [n_rows, 256]: take
    the plane values from the table instead of ``x0`` (which may then be None, or carry a Dropout2d mask)."""
    lib = _lib.load()
    B, H, W, Cg = g.shape
    if out is None:
        out = torch.empty(n_rows, 256, dtype=torch.float32, device=g.device)
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()):
        raise ValueError("idx must be a contiguous int32 CUDA tensor")
    _lib.check(lib.ali_plane_table_grad(_chk(g, "g"), Cg, g_ch, None if table is not None else _chk(x0, "x0"),
                                        0 if table is not None else x0.shape[3], x_ch,
                                        c_void_p(idx.data_ptr()), idx.shape[1], idx_col, B, H, W, n_rows, _chk(out, "out"),
                                        _opt(table, "table"), _stream()), "ali_plane_table_grad")
    return out


def col2im(contrib, ldc, bias, out, B, H, W, Hout, Wout, NC, ostride, R, S, stride, pad, act=ACT_NONE, slope=0.0):
    """Gather half of a scatter-form transposed convolution (include/ali_hip.h: ali_col2im)."""
    lib = _lib.load()
    _lib.check(lib.ali_col2im(_chk(contrib, "contrib"), ldc, _opt(bias, "bias"), _chk(out, "out"), B, H, W, Hout, Wout,
                              NC, ostride, R, S, stride, pad, act, float(slope), _stream()), "ali_col2im")
    return out


def tconv_scatter_ok(C, NC, R, S, stride):
    return bool(_lib.load().ali_tconv_scatter_ok(C, NC, R, S, stride))


def tconv_scatter(x, w_nc, bias, out, B, H, W, C, Hout, Wout, NC, ostride, R, S, stride, pad, act=ACT_NONE, slope=0.0):
    """Scatter-form transposed convolution to 1-2 channels in one launch (include/ali_hip.h: ali_tconv_scatter)."""
    lib = _lib.load()

    def go():
        _lib.check(lib.ali_tconv_scatter(_chk(x, "x"), _chk(w_nc, "w"), _opt(bias, "bias"), _ptr(out), B, H, W, C, Hout,
                                         Wout, NC, ostride, R, S, stride, pad, act, float(slope), _stream()),
                   "ali_tconv_scatter")
    _launch("tconv_scatter", (2.0 * B * H * W * C * NC * R * S, 4.0 * B * (H * W * C + Hout * Wout * NC), _NO_SHAPE), go)
    if _HOOK is not None and hasattr(_HOOK, "scatter"):
        _HOOK.scatter(x, w_nc, bias, out, (B, H, W, C, Hout, Wout, NC, ostride, R, S, stride, pad), act, slope)
    return out


def tconv_scatter_wgrad(big, small, sstride, dw, s_k, s_tap, B, P, Q, K, H, W, R, S, stride, pad):
    """Weight gradient of a strided ConvTranspose2d(64 -> 1) in one launch + slab fold (include/ali_hip.h:
    ali_tconv_scatter_wgrad); returns None when the shape / workspace does not allow it (caller: conv_bwd_weight)."""
    lib = _lib.load()
    need = int(lib.ali_tconv_scatter_wgrad_ws(B, P, Q, K, R, S, stride))
    ws = workspace(big.device)
    if need == 0 or ws.numel() < need:
        return None

    def go():
        _lib.check(lib.ali_tconv_scatter_wgrad(_chk(big, "big"), _ptr(small), sstride, _ptr(dw), s_k, s_tap, B, P, Q, K, H,
                                               W, R, S, stride, pad, c_void_p(ws.data_ptr()), ws.numel(), _stream()),
                   "ali_tconv_scatter_wgrad")
    _launch("tconv_scatter_wgrad", (2.0 * B * P * Q * K * R * S, 4.0 * B * (P * Q * K + H * W), _NO_SHAPE), go)
    return dw


ScatterPlan = collections.namedtuple("ScatterPlan", "name lds blocks nt obh obw rb bands ws")


def tconv_scatter_plan(op, B, H, W, C, Hout, Wout, R, S, stride, pad, NC=1, ostride=None):
    """The launch plan of ``tconv_scatter`` (``op`` "fwd") / ``tconv_scatter_wgrad`` ("wgrad") for a shape, or None
    where the launch refuses it (include/ali_hip.h: ali_tconv_scatter_plan; ``_lib.load().ali_last_error()`` says why).
    B, H, W, C: the 64-channel map (the weight gradient's B, P, Q, K); Hout x Wout: the 1-2 channel map; ``ostride``: its
    element stride (default NC).  ``name`` is "scatter<NT;OBHxOBW>" -- tconv_scatter_kernel<NT> on OBH x OBW output tiles
    -- or "scatter_wgrad<NT;rbRB>" -- tconvs_wgrad_mfma_kernel<NT,4> on bands of RB rows; ``lds`` the dynamic LDS bytes,
    ``blocks`` the grid, ``ws`` the weight gradient's workspace bytes.  Host arithmetic of the library: needs no GPU."""
    out = (ctypes.c_int64 * 6)()
    rc = _lib.load().ali_tconv_scatter_plan({"fwd": 0, "wgrad": 1}[op], B, H, W, C, Hout, Wout, NC,
                                            NC if ostride is None else ostride, R, S, stride, pad, out)
    if rc != 0:
        return None
    if op == "fwd":
        return ScatterPlan(f"scatter<{out[0]};{out[1]}x{out[2]}>", out[3], out[4], out[0], out[1], out[2], 0, 0, 0)
    return ScatterPlan(f"scatter_wgrad<{out[0]};rb{out[1]}>", out[3], out[4], out[0], 0, 0, out[1], out[2], out[5])


def spect_post(y, B, T, F, out, mean=None, std=None, clip_k=3.0):
    lib = _lib.load()
    _lib.check(lib.ali_spect_post(_chk(y, "y"), B, T, F, _opt(mean, "mean"), _opt(std, "std"), float(clip_k),
                                  _chk(out, "out"), _stream()), "ali_spect_post")
    return out


GL_SRC_IMAGE, GL_SRC_LOG, GL_SRC_SPEC = 0, 1, 2


def gl_check(n_fft, win, hop, T, length=0):
    """the window-envelope condition of ``torch.istft`` for T frames (include/ali_hip.h: ali_gl_check; host only):
    True / False, ``ValueError`` unless 0 < hop <= win <= n_fft"""
    rc = _lib.load().ali_gl_check(n_fft, win, hop, T, int(length or 0))
    if rc < 0:
        msg = _lib.load().ali_last_error()
        raise ValueError(msg.decode() if msg else "ali_gl_check: bad argument")
    return bool(rc)


def gl_init(src, mode, mag, X, power=2.0, mean=None, std=None, stds_kept=3.0, angles0=None, rand_init=True, seed=0,
            dev_counter=None, offset=0):
    """src [B,F,T] -> mag [B*T,F], X [B*T,2F] (include/ali_hip.h: ali_gl_init); ``angles0`` = (re, im) planes [B,F,T]"""
    B, F, T = src.shape
    re, im = (None, None) if angles0 is None else angles0
    _lib.check(_lib.load().ali_gl_init(_chk(src, "src"), B, F, T, mode, _opt(mean, "mean"), _opt(std, "std"),
                                       float(stds_kept), float(power), _opt(re, "angles0.re"), _opt(im, "angles0.im"),
                                       int(bool(rand_init)), *_rng_args(seed, dev_counter, offset), _chk(mag, "mag"),
                                       _chk(X, "X"), _stream()), "ali_gl_init")
    return mag, X


def gl_ola(fr, renv, n_fft, hop, length, out, final=False, frames_per_block=0, advance=None):
    """fr [B,T,win] inverse frames -> the next transform's frames [B,T,win] or (``final``) the waveform [B,length]
    (include/ali_hip.h: ali_gl_ola)"""
    B, T, win = fr.shape
    _lib.check(_lib.load().ali_gl_ola(_chk(fr, "fr"), _chk(renv, "renv"), renv.numel(), B, T, n_fft, win, hop, int(length),
                                      int(bool(final)), _chk(out, "out"), int(frames_per_block), _rng_args(0, advance)[1],
                                      _stream()), "ali_gl_ola")
    return out


def gl_phase(Y, tprev, mag, m, X):
    """X = (Y - m*tprev) / (|.| + 1e-16) * mag over [rows,2F] spectra (include/ali_hip.h: ali_gl_phase)"""
    rows, F = mag.shape
    _lib.check(_lib.load().ali_gl_phase(_chk(Y, "Y"), _opt(tprev, "tprev"), _chk(mag, "mag"), float(m), rows, F,
                                        _chk(X, "X"), _stream()), "ali_gl_phase")
    return X


def ssim_fwd(X, Y, win, C1, C2, want_maps=False):
    """SSIM of the [planes,H,W] pairs X, Y (include/ali_hip.h: ali_ssim_fwd), ``win`` the 1-D window on the device.
    Returns (ssim_pc [planes], maps [3,planes,Hm,Wm] = A, Bq, Cq for ``ssim_bwd``, or None)."""
    lib = _lib.load()
    planes, H, W = X.shape
    n = win.numel()
    if Y.shape != X.shape:
        raise ValueError(f"ssim_fwd: shapes differ: {tuple(X.shape)} vs {tuple(Y.shape)}")
    pc = torch.empty(planes, dtype=torch.float32, device=X.device)
    maps = torch.empty((3, planes, max(H - n + 1, 0), max(W - n + 1, 0)), dtype=torch.float32,
                       device=X.device) if want_maps else None
    m = [None] * 3 if maps is None else [c_void_p(maps[i].data_ptr()) for i in range(3)]
    ws = workspace(X.device)
    _lib.check(lib.ali_ssim_fwd(_chk(X, "X"), _chk(Y, "Y"), planes, H, W, _chk(win, "win"), n, float(C1), float(C2),
                                _chk(pc), m[0], m[1], m[2], c_void_p(ws.data_ptr()), ws.numel(), _stream()),
               "ali_ssim_fwd")
    return pc, maps


def ssim_bwd(X, Y, maps, gpc, win, out=None):
    """d sum(gpc * ssim_pc) / dY from the maps ``ssim_fwd(X, Y, ..., want_maps=True)`` left; gpc [planes] on the device."""
    lib = _lib.load()
    planes, H, W = X.shape
    out = torch.empty_like(Y) if out is None else out
    _lib.check(lib.ali_ssim_bwd(_chk(X, "X"), _chk(Y, "Y"), c_void_p(maps[0].data_ptr()), c_void_p(maps[1].data_ptr()),
                                c_void_p(maps[2].data_ptr()), _chk(gpc, "gpc"), planes, H, W, _chk(win, "win"),
                                win.numel(), _chk(out, "out"), _stream()), "ali_ssim_bwd")
    return out


def bce_logits(logit, target, gscale=1.0, want_grad=True):
    """returns (out2 = [loss, mean sigmoid] device tensor, glogit or None)."""
    lib = _lib.load()
    B = logit.numel()
    out2 = torch.empty(2, dtype=torch.float32, device=logit.device)
    gl = torch.empty_like(logit) if want_grad else None
    _lib.check(lib.ali_bce_logits(_chk(logit, "logit"), B, float(target), float(gscale), _chk(out2), _opt(gl),
                                  _stream()), "ali_bce_logits")
    return out2, gl


def bce_logits_pair(logit, B, target_a, target_b, gscale=1.0, want_grad=True):
    """BCE of two passes batched along the rows ([0,B) vs target_a, [B,2B) vs target_b) in one launch.
    Returns (out3 = [(loss_a+loss_b)/2, mean sigmoid(a), mean sigmoid(b)], glogit [2B,1] or None)."""
    lib = _lib.load()
    assert logit.numel() == 2 * B
    out3 = torch.empty(3, dtype=torch.float32, device=logit.device)
    gl = torch.empty_like(logit) if want_grad else None
    _lib.check(lib.ali_bce_logits_pair(_chk(logit, "logit"), B, float(target_a), float(target_b), float(gscale),
                                       _chk(out3), _opt(gl), _stream()), "ali_bce_logits_pair")
    return out3, gl


def _rows2d(t, name):
    """(pointer, B, P) of a contiguous fp32 CUDA tensor read as [B][P] rows (B = its first dimension)"""
    if t.dim() < 1 or t.numel() == 0:
        raise ValueError(f"{name}: need a non-empty tensor with a batch dimension")
    return _chk(t, name), t.shape[0], t.numel() // t.shape[0]


def gp_mix(x_real, x_fake, eps=None, seed=0, dev_counter=None, offset=0, out=None):
    """xhat = eps * x_real + (1 - eps) * x_fake with one eps per image (include/ali_hip.h: ali_gp_mix).  ``eps`` [B]
    given, or None: drawn on the device, uniform in [0, 1), from the counter stream keyed (seed, *dev_counter) at
    element ``offset + b`` (``ali_hip.source.uniform_reference``).  Returns (xhat, eps used [B])."""
    if x_real.shape != x_fake.shape:
        raise ValueError(f"gp_mix: x_real {tuple(x_real.shape)} and x_fake {tuple(x_fake.shape)} differ in shape")
    pr, B, P = _rows2d(x_real, "x_real")
    out = torch.empty_like(x_real) if out is None else out
    if eps is not None and eps.numel() != B:
        raise ValueError(f"gp_mix: eps holds {eps.numel()} values for {B} images")
    eps_out = torch.empty(B, dtype=torch.float32, device=x_real.device)
    _lib.check(_lib.load().ali_gp_mix(pr, _chk(x_fake, "x_fake"), _opt(eps, "eps"), *_rng_args(seed, dev_counter, offset),
                                      B, P, _chk(out, "xhat"), _chk(eps_out), _stream()), "ali_gp_mix")
    return out, eps_out


def gp_penalty(g0, weight=1.0, want_v=True, out=None):
    """Per-image 2-norm n_b of ``g0`` [B, ...]: returns (out2 = [mean (n_b - 1)^2, mean n_b] device tensor,
    v = weight * (2 / B) * (1 - 1 / n_b) * g0 or None); ``out`` may be ``g0`` itself (include/ali_hip.h:
    ali_gp_penalty)."""
    pg, B, P = _rows2d(g0, "g0")
    out2 = torch.empty(2, dtype=torch.float32, device=g0.device)
    v = (torch.empty_like(g0) if out is None else out) if want_v else None
    if v is not None and v.shape != g0.shape:
        raise ValueError("gp_penalty: out must have g0's shape")
    ws = workspace(g0.device)
    _lib.check(_lib.load().ali_gp_penalty(pg, B, P, float(weight), _chk(out2), _opt(v, "v"), c_void_p(ws.data_ptr()),
                                          ws.numel(), _stream()), "ali_gp_penalty")
    return out2, v


def wgan_critic(d_fake, d_real, gscale=1.0, want_grad=True, g_fake=None, g_real=None):
    """returns (out3 = [mean d_fake - mean d_real, mean d_fake, mean d_real] device tensor, g_fake, g_real): the
    gradients gscale / B and -gscale / B (None for absent logits or ``want_grad=False``); ``g_fake`` / ``g_real``:
    where to write them (include/ali_hip.h: ali_wgan_critic)."""
    some = d_fake if d_fake is not None else d_real
    if some is None:
        raise ValueError("wgan_critic: needs d_fake or d_real")
    B = some.numel()
    if d_fake is not None and d_real is not None and d_real.numel() != B:
        raise ValueError("wgan_critic: d_fake and d_real differ in length")
    out3 = torch.empty(3, dtype=torch.float32, device=some.device)
    if want_grad:
        g_fake = g_fake if (g_fake is not None or d_fake is None) else torch.empty_like(d_fake)
        g_real = g_real if (g_real is not None or d_real is None) else torch.empty_like(d_real)
    else:
        g_fake = g_real = None
    for g, d in ((g_fake, d_fake), (g_real, d_real)):
        if g is not None and (d is None or g.numel() != B):
            raise ValueError("wgan_critic: a gradient buffer needs its logits and their length")
    _lib.check(_lib.load().ali_wgan_critic(_opt(d_fake, "d_fake"), _opt(d_real, "d_real"), B, float(gscale), _chk(out3),
                                           _opt(g_fake, "g_fake"), _opt(g_real, "g_real"), _stream()),
               "ali_wgan_critic")
    return out3, g_fake, g_real


FLOW_THETA = 75
FLOW_SKIP, FLOW_FORWARD, FLOW_INVERSE = 0, 1, 2


def _col(t, name):
    """(pointer, rows, row stride in floats) of an fp32 CUDA column, [N] or [N, 1]; it may be a strided view (one
    column of an attribute table)"""
    if not (t.is_cuda and t.dtype == torch.float32 and (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1))
            and t.shape[0] >= 1):
        raise ValueError(f"{name}: need a non-empty fp32 CUDA column [N] or [N, 1], got {t.dtype} {t.device} "
                         f"{tuple(t.shape)}")
    N = t.shape[0]
    stride = t.stride(0) if N > 1 else 1
    if stride < 1:
        raise ValueError(f"{name}: rows must lie at a positive stride, got {stride}")
    return c_void_p(t.data_ptr()), N, stride


def _flow_vec(t, n, name):
    if t.numel() != n:
        raise ValueError(f"{name}: need {n} floats, got {t.numel()}")
    return _chk(t, name)


def flow_stats(t, moving=None, momentum=0.1, out=None):
    """out2 = [mean, unbiased variance] of log ``t`` (a column, see ``_col``); ``moving`` (2 floats: mean, variance) is
    moved by ``momentum`` towards them in the same launch and then needs N >= 2 (include/ali_hip.h: ali_flow_stats)."""
    pt, N, st = _col(t, "t")
    out = torch.empty(2, dtype=torch.float32, device=t.device) if out is None else out
    ws = workspace(t.device)
    _lib.check(_lib.load().ali_flow_stats(pt, st, N, _flow_vec(out, 2, "out2"),
                                          None if moving is None else _flow_vec(moving, 2, "moving"), float(momentum),
                                          c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_flow_stats")
    return out


def flow_nll(t, i, s, theta, cst, stats, wgt=None, gscale=1.0, want_lp=True, want_out4=True, want_grad=False,
             gtheta=None):
    """The three log-densities of the MorphoMNIST attribute SCM for rows (t, i, s) -- columns, see ``_col`` -- under
    ``theta`` [75], ``cst`` [4] and ``stats`` [2] (include/ali_hip.h: ali_flow_nll).  Returns (lp [N, 3] or None,
    out4 = [-mean(sum lp), mean lp_t, mean lp_i, mean lp_s] or None, gtheta [75] or None): gtheta = sum wgt * d lp /
    d theta with ``wgt`` [N, 3], or the constant ``gscale`` / N when ``wgt`` is None; ``gtheta``: where to write it."""
    pt, N, st = _col(t, "t")
    pi, Ni, si = _col(i, "i")
    ps, Ns, ss = _col(s, "s")
    if not N == Ni == Ns:
        raise ValueError(f"flow_nll: the columns hold {N}, {Ni} and {Ns} rows")
    dev = t.device
    lp = torch.empty(N, 3, dtype=torch.float32, device=dev) if want_lp else None
    out4 = torch.empty(4, dtype=torch.float32, device=dev) if want_out4 else None
    if gtheta is None and want_grad:
        gtheta = torch.empty(FLOW_THETA, dtype=torch.float32, device=dev)
    if wgt is not None and tuple(wgt.shape) != (N, 3):
        raise ValueError(f"flow_nll: wgt must be [{N}, 3], got {tuple(wgt.shape)}")
    ws = workspace(dev)
    _lib.check(_lib.load().ali_flow_nll(pt, st, pi, si, ps, ss, N, _flow_vec(theta, FLOW_THETA, "theta"),
                                        _flow_vec(cst, 4, "cst"), _flow_vec(stats, 2, "stats"), _opt(wgt, "wgt"),
                                        float(gscale), _opt(lp), _opt(out4),
                                        None if gtheta is None else _flow_vec(gtheta, FLOW_THETA, "gtheta"),
                                        c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_flow_nll")
    return lp, out4, gtheta


def flow_map(rows, theta, cst, stats_inv, stats_fwd, modes=(FLOW_SKIP, FLOW_SKIP, FLOW_SKIP), cf_mask=None, val=None,
             want_noise=False, out=None):
    """The mechanisms elementwise on ``rows`` [N, 3] (thickness, intensity, slant): per column skip / forward (noise ->
    value) / inverse (value -> noise), or -- ``cf_mask`` not None -- the counterfactual of observed rows with the
    columns of the bit mask replaced by ``val`` [N, 3] (include/ali_hip.h: ali_flow_map).  Returns (out [N, 3], the
    abducted noise [N, 3] or None); ``out`` may be ``rows``."""
    if rows.dim() != 2 or rows.shape[1] != 3 or rows.shape[0] < 1:
        raise ValueError(f"flow_map: need [N, 3] rows, got {tuple(rows.shape)}")
    N = rows.shape[0]
    out = torch.empty_like(rows) if out is None else out
    cf = cf_mask is not None
    if val is not None and val.shape != rows.shape:
        raise ValueError("flow_map: val must have the rows' shape")
    if out.shape != rows.shape:
        raise ValueError("flow_map: out must have the rows' shape")
    noise = torch.empty_like(rows) if (cf and want_noise) else None
    _lib.check(_lib.load().ali_flow_map(_chk(rows, "rows"), _opt(val, "val"), _chk(out, "out"), _opt(noise), N,
                                        int(modes[0]), int(modes[1]), int(modes[2]), int(cf), int(cf_mask or 0),
                                        _flow_vec(theta, FLOW_THETA, "theta"), _flow_vec(cst, 4, "cst"),
                                        _flow_vec(stats_inv, 2, "stats_inv"), _flow_vec(stats_fwd, 2, "stats_fwd"),
                                        _stream()), "ali_flow_map")
    return out, noise


def gumbel_posterior(logits, y, g=None, seed=0, dev_counter=None, offset=0, want_g=False):
    """Gumbel-max posterior noise [N, C] of observed classes ``y`` [N] (int64) under ``logits`` [N, C], so that
    ``argmax(logits + noise) == y`` (include/ali_hip.h: ali_gumbel_posterior).  ``g`` [N, C] given, or None: drawn on
    the device from the counter stream keyed (seed, *dev_counter) at elements ``offset + n * C + c``
    (``ali_hip.source.gumbel_reference``).  Returns (noise, the g used or None)."""
    if logits.dim() != 2:
        raise ValueError(f"gumbel_posterior: need [N, C] logits, got {tuple(logits.shape)}")
    N, C = logits.shape
    if not (y.is_cuda and y.dtype == torch.int64 and y.is_contiguous() and y.numel() == N):
        raise ValueError(f"gumbel_posterior: y must be {N} contiguous int64 CUDA values")
    if g is not None and g.shape != logits.shape:
        raise ValueError("gumbel_posterior: g must have the logits' shape")
    noise = torch.empty_like(logits)
    g_out = torch.empty_like(logits) if want_g else None
    _lib.check(_lib.load().ali_gumbel_posterior(_chk(logits, "logits"), c_void_p(y.data_ptr()), _opt(g, "g"),
                                                *_rng_args(seed, dev_counter, offset), N, C, _chk(noise), _opt(g_out),
                                                _stream()), "ali_gumbel_posterior")
    return noise, g_out


# ---- the AudioMNIST attribute SCM (csrc/cat.hip) ---------------------------------------------------------------------
CAT_LOGITS, CAT_SAMPLE, CAT_DIFFER, CAT_ABDUCT, CAT_CF = range(5)
CAT_ENTRY_NLL, CAT_ENTRY_GRAD, CAT_ENTRY_MAP = range(3)
CAT_TRIES = 64
CatPlan = collections.namedtuple("CatPlan", "grid threads tile_rows tiles tiles_per_block grid2 threads2 lds_bytes ws_bytes")


def cat_plan(N, Cc, Cn, Ca, entry=CAT_ENTRY_GRAD) -> CatPlan:
    """how ``entry`` runs N rows of an AudioMNIST graph with (Cc, Cn, Ca) classes: grid, row tile, workspace bytes
    (include/ali_hip.h: ali_cat_plan).  A host query; the launches use the same function."""
    pl = _lib.AliCatPlan()
    _lib.check(_lib.load().ali_cat_plan(int(N), int(Cc), int(Cn), int(Ca), int(entry), byref(pl)), "ali_cat_plan")
    return CatPlan(*(int(getattr(pl, f)) for f in CatPlan._fields))


def cat_sizes(Cc, Cn, Ca):
    """(floats of theta, floats of the tower buffer) in the layouts of include/ali_hip.h; raises outside [1, 64]"""
    lib = _lib.load()
    n = lib.ali_cat_theta_size(int(Cc), int(Cn), int(Ca), 0), lib.ali_cat_theta_size(int(Cc), int(Cn), int(Ca), 1)
    if not n[0]:
        raise ValueError(f"cat: class counts ({Cc}, {Cn}, {Ca}) outside [1, 64]")
    return n


def _cat_rows(t, name, N=None):
    """(pointer, rows, classes, row stride) of fp32 CUDA rows [N, C]; a column range of a wider table passes"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] >= 1
            and t.shape[1] >= 1 and (t.shape[1] == 1 or t.stride(1) == 1)):
        raise ValueError(f"{name}: need non-empty fp32 CUDA rows [N, C] with unit column stride")
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if ld < t.shape[1] or (N is not None and t.shape[0] != N):
        raise ValueError(f"{name}: {tuple(t.shape)} rows at stride {ld}" + ("" if N is None else f", {N} rows expected"))
    return c_void_p(t.data_ptr()), t.shape[0], t.shape[1], ld


def _cat_i64(t, N, name):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == N):
        raise ValueError(f"{name}: need {N} contiguous int64 CUDA values")
    return t.data_ptr()


def cat_nll(theta, towers, country, native, accent, index=None, wgt=None, gscale=1.0, want_lp=True, want_out3=True,
            want_grad=False, gtheta=None):
    """The log-probabilities of native_speaker and accent given their parents (include/ali_hip.h: ali_cat_nll).
    ``country`` / ``native`` / ``accent``: fp32 rows (see ``_cat_rows``) of one row count; ``index`` (int64 [N]): row n
    reads source row index[n].  Returns (lp [N, 2] or None, out3 = [-mean(lp_n + lp_a), mean lp_n, mean lp_a] or None,
    gtheta or None): gtheta = gscale * sum_n wgt[n] . d lp[n] / d theta, ``wgt`` [N, 2] or, None, 1 / N each."""
    pc, R, Cc, sc = _cat_rows(country, "country")
    pn, _, Cn, sn = _cat_rows(native, "native", R)
    pa, _, Ca, sa = _cat_rows(accent, "accent", R)
    nth, ntw = cat_sizes(Cc, Cn, Ca)
    N = R if index is None else index.numel()
    ix = _cat_i64(index, N, "index")
    dev = country.device
    lp = torch.empty(N, 2, dtype=torch.float32, device=dev) if want_lp else None
    out3 = torch.empty(3, dtype=torch.float32, device=dev) if want_out3 else None
    if gtheta is None and want_grad:
        gtheta = torch.empty(nth, dtype=torch.float32, device=dev)
    if wgt is not None and tuple(wgt.shape) != (N, 2):
        raise ValueError(f"cat_nll: wgt must be [{N}, 2], got {tuple(wgt.shape)}")
    ws = workspace(dev)
    _lib.check(_lib.load().ali_cat_nll(_flow_vec(theta, nth, "theta"), _flow_vec(towers, ntw, "towers"), Cc, Cn, Ca,
                                       pc, sc, pn, sn, pa, sa, ix, R, N, _opt(wgt, "wgt"), float(gscale), _opt(lp),
                                       _opt(out3), None if gtheta is None else _flow_vec(gtheta, nth, "gtheta"),
                                       c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_cat_nll")
    return lp, out3, gtheta


def cat_map(mode, theta, towers, country, Cn, Ca, country_cf=None, native_rows=None, y=(None, None), v=(None, None),
            node=0, cf_mask=0, seed=0, dev_counter=None, offset=0, want_logits=False, want_g=False, want_noise=False):
    """The three mechanisms row-wise in one launch (include/ali_hip.h: ali_cat_map).  ``y`` / ``v``: pairs (native_speaker,
    accent) of int64 [N] classes or None.  Returns a dict: "out" (pair of int64 [N], None where the mode writes none),
    "status" (int32 [N], CAT_DIFFER), "logits" / "g" / "noise" (the stored intermediates, on request; "noise" always for
    CAT_ABDUCT)."""
    pc, N, Cc, sc = _cat_rows(country, "country")
    nth, ntw = cat_sizes(Cc, Cn, Ca)
    dev, Ct = country.device, Cn + Ca
    a = _lib.AliCatMapArgs()
    a.country, a.country_ld = pc, sc
    if country_cf is not None:
        a.country_cf, _, Ccf, a.country_cf_ld = _cat_rows(country_cf, "country_cf", N)
        if Ccf != Cc:
            raise ValueError("cat_map: country_cf must have country's width")
    if native_rows is not None:
        a.native_rows, _, Cnr, a.native_ld = _cat_rows(native_rows, "native_rows", N)
        if Cnr != Cn:
            raise ValueError(f"cat_map: native_rows must be [{N}, {Cn}]")
    for j in range(2):
        a.y[j] = _cat_i64(y[j], N, "y")
        a.v[j] = _cat_i64(v[j], N, "v")
    a.node, a.cf_mask = int(node), int(cf_mask)
    res = {"out": [None, None], "status": None, "logits": None, "g": None, "noise": None}
    if mode in (CAT_SAMPLE, CAT_DIFFER, CAT_CF):
        for j in range(2):
            if mode == CAT_CF or y[j] is None:
                res["out"][j] = torch.empty(N, dtype=torch.int64, device=dev)
                a.out[j] = res["out"][j].data_ptr()
    if mode == CAT_DIFFER:
        res["status"] = torch.empty(N, dtype=torch.int32, device=dev)
        a.status = res["status"].data_ptr()
    if want_logits or mode == CAT_LOGITS:
        res["logits"] = torch.empty((2, N, Ct) if mode == CAT_CF else (N, Ct), dtype=torch.float32, device=dev)
        a.logits_out = res["logits"].data_ptr()
    if want_g and mode != CAT_LOGITS:
        shape = (CAT_TRIES, N, Ca if node else Cn) if mode == CAT_DIFFER else (N, Ct)
        res["g"] = torch.zeros(shape, dtype=torch.float32, device=dev)
        a.g_out = res["g"].data_ptr()
    if mode == CAT_ABDUCT or (want_noise and mode == CAT_CF):
        res["noise"] = torch.empty(N, Ct, dtype=torch.float32, device=dev)
        a.noise_out = res["noise"].data_ptr()
    _lib.check(_lib.load().ali_cat_map(int(mode), _flow_vec(theta, nth, "theta"), _flow_vec(towers, ntw, "towers"), Cc,
                                       Cn, Ca, N, byref(a), *_rng_args(seed, dev_counter)[:2],
                                       int(offset) & (2 ** 64 - 1), _stream()), "ali_cat_map")
    res["out"] = tuple(res["out"])
    return res


def softmax_xent(logit, target, gscale=1.0, want_grad=True, want_pred=False, hits_accum=None):
    """Cross-entropy of [B, C] logits against probability rows, gradient, arg-max and hit count in one launch
    (include/ali_hip.h: ali_softmax_xent).  Returns (out2 = [mean loss, hits] device tensor, glogit or None,
    pred int32 [B] or None); ``hits_accum`` (one-element int64 device tensor) += hits on the device."""
    lib = _lib.load()
    if logit.dim() != 2 or target.shape != logit.shape:
        raise ValueError(f"softmax_xent: need [B, C] logits and targets of one shape, got {tuple(logit.shape)} and "
                         f"{tuple(target.shape)}")
    B, C = logit.shape
    if hits_accum is not None and not (hits_accum.is_cuda and hits_accum.dtype == torch.int64
                                       and hits_accum.numel() == 1):
        raise ValueError("softmax_xent: hits_accum must be a one-element int64 CUDA tensor")
    out2 = torch.empty(2, dtype=torch.float32, device=logit.device)
    gl = torch.empty_like(logit) if want_grad else None
    pred = torch.empty(B, dtype=torch.int32, device=logit.device) if want_pred else None
    ws = workspace(logit.device)
    _lib.check(lib.ali_softmax_xent(_chk(logit, "logit"), _chk(target, "target"), B, C, float(gscale), _chk(out2),
                                    _opt(gl), None if pred is None else c_void_p(pred.data_ptr()),
                                    None if hits_accum is None else c_void_p(hits_accum.data_ptr()),
                                    c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_softmax_xent")
    return out2, gl, pred


def _attr_arrays(tensors):
    """ctypes views of a list of [B, n] one-hot tensors (fp32 or int32, contiguous CUDA)."""
    n = len(tensors)
    for t in tensors:
        if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.float32, torch.int32) and t.dim() == 2):
            raise ValueError(f"categorical attribute: need a contiguous [B, n] fp32 / int32 CUDA tensor, got "
                             f"{t.dtype} {tuple(t.shape)}")
    ptrs = (c_void_p * max(n, 1))(*[t.data_ptr() for t in tensors])
    ncls = (ctypes.c_int32 * max(n, 1))(*[t.shape[1] for t in tensors])
    isint = (ctypes.c_int32 * max(n, 1))(*[int(t.dtype == torch.int32) for t in tensors])
    return ptrs, ncls, isint


def attr_pack(cats, conts, B, device):
    """arg-max class of every categorical attribute -> idx [B, n_cat] int32; continuous attributes ([B] / [B,1] fp32)
    -> cont [B, n_cont] (or None).  One launch (include/ali_hip.h: ali_attr_pack)."""
    lib = _lib.load()
    ptrs, ncls, isint = _attr_arrays(cats)
    idx = torch.empty(B, max(len(cats), 1), dtype=torch.int32, device=device)
    for t in conts:
        _chk(t, "continuous attribute")
    cptr = (c_void_p * max(len(conts), 1))(*[t.data_ptr() for t in conts])
    cont = torch.empty(B, len(conts), dtype=torch.float32, device=device) if conts else None
    _lib.check(lib.ali_attr_pack(ptrs, ncls, isint, len(cats), cptr, len(conts), B, c_void_p(idx.data_ptr()),
                                 None if cont is None else c_void_p(cont.data_ptr()), _stream()), "ali_attr_pack")
    return idx, cont


def g_input(z, onehots, tables, cont, ld, out=None):
    """Generator input rows [B, ld] = [z | onehot_j @ table_j | cont | 0] in one launch (ali_g_input)."""
    lib = _lib.load()
    B, zdim = z.shape
    ptrs, ncls, isint = _attr_arrays(onehots)
    for t in tables:
        _chk(t, "embedding table")
    tptr = (c_void_p * max(len(tables), 1))(*[t.data_ptr() for t in tables])
    if out is None:
        out = torch.empty(B, ld, dtype=torch.float32, device=z.device)
    _lib.check(lib.ali_g_input(_chk(z, "z"), zdim, ptrs, ncls, isint, tptr, len(tables), _opt(cont, "cont"),
                               0 if cont is None else cont.shape[1], B, ld, _chk(out), _stream()), "ali_g_input")
    return out


def g_input_table_grad(onehot, g, off, out):
    """out [n_classes, 256] = onehot^T @ g[:, off:off+256]  (ali_g_input_table_grad)."""
    lib = _lib.load()
    ptrs, ncls, isint = _attr_arrays([onehot])
    _lib.check(lib.ali_g_input_table_grad(c_void_p(onehot.data_ptr()), isint[0], ncls[0], _chk(g, "g"), g.shape[1], off,
                                          g.shape[0], _chk(out, "out"), _stream()), "ali_g_input_table_grad")
    return out


def adam(p, g, m, v, lr, beta1, beta2, eps, step, dev_step=None, grad_scale=1.0, arrive=None, p16=None):
    """One torch.optim.Adam step over a flat fp32 segment; the gradient is read as ``grad_scale * g``.
    Step conventions (include/ali_hip.h: ali_adam):
    - ``dev_step`` None: ``step`` is the 1-based number of this step (>= 1);
    - ``dev_step`` without ``arrive``: the int32 device scalar holds the 1-based number of this step and is left as it
      is.  It must be >= 1: a count of completed steps (0 before the first) would give bias correction 1 - beta1^0 = 0;
    - ``dev_step`` with ``arrive`` (zeroed int32 device tensor, left at zero): ``dev_step`` counts COMPLETED steps, the
      launch runs step ``dev_step + 1`` and stores that value back itself.
    ``p16`` (fp16, same numel): the launch also leaves the fp16 twin of the updated parameters."""
    lib = _lib.load()
    ds = ar = None
    if dev_step is not None:
        assert dev_step.is_cuda and dev_step.dtype == torch.int32
        ds = c_void_p(dev_step.data_ptr())
    if arrive is not None:
        assert arrive.is_cuda and arrive.dtype == torch.int32 and dev_step is not None
        ar = c_void_p(arrive.data_ptr())
    _lib.check(lib.ali_adam(_chk(p, "p"), _chk(g, "g"), _chk(m, "m"), _chk(v, "v"), p.numel(), lr, beta1, beta2, eps,
                            step, ds, ar, grad_scale, None if p16 is None else c_void_p(p16.data_ptr()), _stream()),
               "ali_adam")


def add_i64_multi(counters, incs):
    """counters[i] += incs[i] for int64 device scalars, one launch per 16 counters (include/ali_hip.h:
    ali_add_i64_multi); a counter named twice receives both increments"""
    n = len(counters)
    if n == 0:
        return
    for t in counters:
        if not (t.is_cuda and t.dtype == torch.int64 and t.numel() == 1):
            raise ValueError("add_i64_multi: need one-element int64 CUDA tensors")
    ptrs = (c_void_p * n)(*[t.data_ptr() for t in counters])
    inc = (ctypes.c_int64 * n)(*[int(v) for v in incs])
    _lib.check(_lib.load().ali_add_i64_multi(n, ptrs, inc, _stream()), "ali_add_i64_multi")


def assemble_planes(X, idx, tables, cont, B, H, W, Cpad, out=None, mask=None):
    """X [B,H,W] fp32; idx [B,n_emb] int32; tables: list of [n,256] fp32; cont [B,n_cont] or None.
    ``out``: optional contiguous [B,H,W,Cpad] destination (e.g. one half of a batched-pass buffer).
    ``mask`` [B, >= Cpad] (any row stride): multiply the planes by it per (sample, channel)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(B, H, W, Cpad, dtype=torch.float32, device=X.device)
    n_emb = len(tables)
    arr = (c_void_p * max(n_emb, 1))(*[t.data_ptr() for t in tables])
    for t in tables:
        _chk(t, "embedding table")
    if idx is not None and not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()):
        raise ValueError("idx must be a contiguous int32 CUDA tensor")
    n_cont = 0 if cont is None else cont.shape[1]
    _lib.check(lib.ali_assemble_planes(_chk(X, "X"), None if idx is None else c_void_p(idx.data_ptr()),
                                       ctypes.cast(arr, ctypes.POINTER(c_void_p)), n_emb, _opt(cont), n_cont,
                                       _chk(out), B, H, W, Cpad, None if mask is None else _ptr(mask),
                                       0 if mask is None else mask.stride(0), _stream()), "ali_assemble_planes")
    return out


# ---- the DeepSCM conditional VAE between its conv stacks (csrc/vae.hip) ----------------------------------------------
def _row_view(t, cols, name):
    """a [rows, cols] fp32 CUDA view whose rows are ``stride(0)`` floats apart (a column range of a wider buffer)"""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == cols and t.stride(0) >= cols
            and (cols == 1 or t.stride(1) == 1)):
        raise ValueError(f"{name}: need a [rows, {cols}] fp32 CUDA view with unit column stride, got {t.dtype} "
                         f"{tuple(t.shape)} strides {tuple(t.stride())}")
    return c_void_p(t.data_ptr())


def vae_latent_fwd(mean, log_var, S, out, k=0.5, eps=None, seed=0, dev_counter=None, offset=0, want_eps=False,
                   onehots=None, tables=None, cont=None, want_kl=True):
    """Decoder input rows of S latent draws (include/ali_hip.h: ali_vae_latent_fwd): out [S*B, ld] columns 0..L become
    mean + eps * exp(k * log_var); ``onehots`` / ``tables`` / ``cont`` given (lists, may be empty): the columns behind
    become [onehot_j @ table_j | cont | 0] in the same launch, else they are left alone.  ``mean`` / ``log_var``:
    [B, L] views of one row stride.  ``eps`` [S, B, L], or None: drawn in the kernel from the stream of ``normal_fill``
    keyed (seed, dev_counter) at ``offset`` (``want_eps``: returned).  Returns (kl_sum [1] or None, eps or None)."""
    lib = _lib.load()
    B, L = mean.shape
    if log_var.shape != mean.shape or log_var.stride(0) != mean.stride(0):
        raise ValueError("vae_latent_fwd: mean and log_var must be [B, L] views of one row stride")
    if out.dim() != 2 or out.shape[0] != S * B or out.shape[1] < L:
        raise ValueError(f"vae_latent_fwd: out must be [S*B, ld >= L], got {tuple(out.shape)}")
    ld = out.shape[1]
    eps_out = None
    if eps is not None:
        if eps.numel() != S * B * L:
            raise ValueError(f"vae_latent_fwd: eps must hold S*B*L = {S * B * L} values, got {tuple(eps.shape)}")
        _chk(eps, "eps")
    elif want_eps:
        eps_out = torch.empty(S, B, L, dtype=torch.float32, device=mean.device)
    write_cond = onehots is not None
    onehots, tables = list(onehots or []), list(tables or [])
    if len(onehots) != len(tables):
        raise ValueError("vae_latent_fwd: one table per one-hot attribute")
    for t in onehots:
        if t.shape[0] != B:
            raise ValueError("vae_latent_fwd: the attributes are per sample ([B, n]); the S draws share them")
    for t, oh in zip(tables, onehots):
        _chk(t, "embedding table")
        if t.shape != (oh.shape[1], 256):
            raise ValueError(f"vae_latent_fwd: table {tuple(t.shape)} does not match its attribute's {oh.shape[1]} classes")
    if cont is not None and cont.shape[0] != B:
        raise ValueError("vae_latent_fwd: cont must be [B, n_cont]")
    ptrs, ncls, isint = _attr_arrays(onehots)
    tptr = (c_void_p * max(len(tables), 1))(*[t.data_ptr() for t in tables])
    kl = torch.empty(1, dtype=torch.float32, device=mean.device) if want_kl else None
    ws = workspace(mean.device)
    _lib.check(lib.ali_vae_latent_fwd(
        _row_view(mean, L, "mean"), _row_view(log_var, L, "log_var"), mean.stride(0),
        None if eps is None else c_void_p(eps.data_ptr()), None if eps_out is None else c_void_p(eps_out.data_ptr()),
        *_rng_args(seed, dev_counter, offset), S, B, L, float(k), ptrs, ncls, isint, tptr, len(tables),
        _opt(cont, "cont"), 0 if cont is None else cont.shape[1], int(write_cond), ld, _chk(out, "out"), _opt(kl),
        c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_vae_latent_fwd")
    return kl, (eps if eps is not None else eps_out)


def vae_loglik(x, xhat, S, log_var=-5.0, kl_sum=None, kl_weight=1.0, gscale=1.0, want_grad=True):
    """Gaussian log-likelihood of x [B, P] under xhat [S*B, P] (include/ali_hip.h: ali_vae_loglik).  Returns
    (out3 = [logp, loss = -(logp - kl_weight * kl_sum / B), kl_sum / B] device tensor, gxhat [S*B, P] or None)."""
    lib = _lib.load()
    B, P = x.shape
    if xhat.shape != (S * B, P):
        raise ValueError(f"vae_loglik: xhat must be [S*B, P] = {(S * B, P)}, got {tuple(xhat.shape)}")
    out3 = torch.empty(3, dtype=torch.float32, device=x.device)
    g = torch.empty_like(xhat) if want_grad else None
    ws = workspace(x.device)
    _lib.check(lib.ali_vae_loglik(_chk(x, "x"), _chk(xhat, "xhat"), B, S, P, float(log_var), _opt(kl_sum, "kl_sum"),
                                  float(kl_weight), float(gscale), _chk(out3), _opt(g), c_void_p(ws.data_ptr()),
                                  ws.numel(), _stream()), "ali_vae_loglik")
    return out3, g


def vae_latent_bwd(gin, eps, mean, log_var, S, gmean, glog_var, k=0.5, kl_weight=1.0, kl_scale=None, ncond=0):
    """Head gradient from the decoder input gradient gin [S*B, ld] (include/ali_hip.h: ali_vae_latent_bwd), written
    into the [B, L] views ``gmean`` / ``glog_var`` (one row stride); ``ncond`` > 0: also returns gcond [B, ncond], the
    sum over the S draws of gin's columns L .. L + ncond.  ``kl_scale``: one-element device tensor multiplying the KL
    terms (autograd's incoming gradient)."""
    lib = _lib.load()
    B, L = mean.shape
    if gin.dim() != 2 or gin.shape[0] != S * B or gin.shape[1] < L + ncond:
        raise ValueError(f"vae_latent_bwd: gin must be [S*B, ld >= L + ncond], got {tuple(gin.shape)}")
    if eps.numel() != S * B * L:
        raise ValueError("vae_latent_bwd: eps must hold S*B*L values")
    if log_var.stride(0) != mean.stride(0) or gmean.stride(0) != glog_var.stride(0):
        raise ValueError("vae_latent_bwd: mean / log_var and gmean / glog_var must each share a row stride")
    gcond = torch.empty(B, ncond, dtype=torch.float32, device=gin.device) if ncond else None
    _lib.check(lib.ali_vae_latent_bwd(_chk(gin, "gin"), gin.shape[1], _chk(eps, "eps"), _row_view(mean, L, "mean"),
                                      _row_view(log_var, L, "log_var"), mean.stride(0), S, B, L, float(k),
                                      float(kl_weight), _opt(kl_scale, "kl_scale"), _row_view(gmean, L, "gmean"),
                                      _row_view(glog_var, L, "glog_var"), gmean.stride(0), ncond, _opt(gcond),
                                      _stream()), "ali_vae_latent_bwd")
    return gcond


# ---------------------------------------------------------------------- the counterfactual explainers (csrc/explain.hip)
DIST_L1, DIST_L2 = 0, 1
CF_COPY, CF_TANH, CF_SOFTMAX = 0, 1, 2
CF_EMB = 256


def _i32(t, name, n=None):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and (n is None or t.numel() == n)):
        raise ValueError(f"{name}: need a contiguous int32 CUDA tensor" + ("" if n is None else f" of {n} elements"))
    return c_void_p(t.data_ptr())


def row_dist(x, y, mode=DIST_L1, out=None):
    """out[s] = mean_n |y[s, n] - x[s or 0, n]| (``DIST_L1``) or the mean of the squares (``DIST_L2``); x: [1 or S, ...],
    y: [S, ...], rows flattened (include/ali_hip.h: ali_row_dist)."""
    lib = _lib.load()
    S = y.shape[0]
    N = y.numel() // max(S, 1)
    if x.shape[0] not in (1, S) or x.numel() != x.shape[0] * N:
        raise ValueError(f"row_dist: x {tuple(x.shape)} is neither one row nor one row per row of y {tuple(y.shape)}")
    if out is None:
        out = torch.empty(S, dtype=torch.float32, device=y.device)
    ws = workspace(y.device)
    _lib.check(lib.ali_row_dist(_chk(x, "x"), x.shape[0], _chk(y, "y"), S, N, int(mode), _chk(out, "out"),
                                c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_row_dist")
    return out


def cf_hinge(logit, target, m, c, orig_pred=None, want_grad=True, out=None, glogit=None):
    """Per-row loss of the hinge explainer (include/ali_hip.h: ali_cf_hinge): logit [B, C], target [B] int32 (< 0: the
    row compares with ``orig_pred`` [B, C] instead), m [B].  Returns (out [B, 3] = (c*h + m, h, m), glogit or None)."""
    lib = _lib.load()
    if logit.dim() != 2:
        raise ValueError(f"cf_hinge: need [B, C] logits, got {tuple(logit.shape)}")
    B, C = logit.shape
    if orig_pred is not None and orig_pred.shape != logit.shape:
        raise ValueError("cf_hinge: orig_pred must have the logits' shape")
    if m.numel() != B:
        raise ValueError("cf_hinge: one m per row")
    if out is None:
        out = torch.empty(B, 3, dtype=torch.float32, device=logit.device)
    if glogit is None and want_grad:
        glogit = torch.empty_like(logit)
    _lib.check(lib.ali_cf_hinge(_chk(logit, "logit"), _i32(target, "target", B), _opt(orig_pred, "orig_pred"),
                                _chk(m, "m"), float(c), B, C, _chk(out, "out"), _opt(glogit, "glogit"), _stream()),
               "ali_cf_hinge")
    return out, glogit


def cf_join(gx_clf, x_cf, x, out=None):
    """gy [B, N] = gx_clf[..., 0] + sign(x_cf - x) / N: the classifier's NHWC input gradient [B, H, W, Cpad] joined with
    the gradient of mean |x - x_cf| (include/ali_hip.h: ali_cf_join); x: [B or 1, N]."""
    lib = _lib.load()
    B = x_cf.shape[0]
    N = x_cf.numel() // B
    if gx_clf.numel() % (B * N) or x.numel() not in (N, B * N):
        raise ValueError(f"cf_join: gx_clf {tuple(gx_clf.shape)}, x_cf {tuple(x_cf.shape)} and x {tuple(x.shape)} "
                         "do not belong together")
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=x_cf.device)
    _lib.check(lib.ali_cf_join(_chk(gx_clf, "gx_clf"), gx_clf.numel() // (B * N), _chk(x_cf, "x_cf"), _chk(x, "x"),
                               x.numel() // N, B, N, _chk(out, "out"), _stream()), "ali_cf_join")
    return out


class CfLayout:
    """The segment table of ``cf_input_fwd`` / ``cf_input_step`` (include/ali_hip.h: AliCfSegment): ``segments`` is a
    list of (kind, width, src_off, dst_off, table index or -1, attr_off or -1); ``tables`` the embedding tables
    ([width, 256] fp32 CUDA) the indices name; ``n_log`` / ``ld`` the logical and padded width of the generator's
    input row.  The widths of the raw, given and attribute rows follow from the segments."""

    def __init__(self, segments, tables, n_log, ld):
        self.segments = [tuple(int(v) for v in s) for s in segments]
        self.tables = list(tables)
        self.n_log, self.ld = int(n_log), int(ld)
        self.raw_ld = max([s[2] + s[1] for s in self.segments if s[0] != CF_COPY], default=0)
        self.given_ld = max([s[2] + s[1] for s in self.segments if s[0] == CF_COPY], default=0)
        self.attrs_ld = max([s[5] + s[1] for s in self.segments if s[5] >= 0], default=0)
        self._segs = (_lib.AliCfSegment * max(len(self.segments), 1))(*[_lib.AliCfSegment(*s) for s in self.segments])
        for t in self.tables:
            _chk(t, "embedding table")
        for s in self.segments:
            if s[4] >= 0 and (s[4] >= len(self.tables) or tuple(self.tables[s[4]].shape) != (s[1], CF_EMB)):
                raise ValueError(f"CfLayout: segment {s} needs table {s[4]} of shape ({s[1]}, {CF_EMB})")
        self._tabs = (c_void_p * max(len(self.tables), 1))(*[t.data_ptr() for t in self.tables])


def _rows(t, ld, name, B=None):
    if t is None:
        if ld:
            raise ValueError(f"{name}: the layout needs {ld} columns")
        return None
    if t.dim() != 2 or t.shape[1] != ld or (B is not None and t.shape[0] != B):
        raise ValueError(f"{name}: need [B, {ld}] rows, got {tuple(t.shape)}")
    return _chk(t, name)


def cf_input_fwd(lay: CfLayout, raw, given, rows=None, attrs=None):
    """Raw variables [B, raw_ld] (and the given columns [B, given_ld]) -> (generator input rows [B, ld], transformed
    attribute rows [B, attrs_ld]) in one launch (include/ali_hip.h: ali_cf_input_fwd)."""
    lib = _lib.load()
    some = raw if raw is not None else given
    B = some.shape[0]
    if rows is None:
        rows = torch.empty(B, lay.ld, dtype=torch.float32, device=some.device)
    if attrs is None:
        attrs = torch.empty(B, lay.attrs_ld, dtype=torch.float32, device=some.device)
    _lib.check(lib.ali_cf_input_fwd(_rows(raw, lay.raw_ld, "raw", B), lay.raw_ld, _rows(given, lay.given_ld, "given", B),
                                    lay.given_ld, lay._segs, len(lay.segments), lay._tabs, len(lay.tables), B, lay.n_log,
                                    lay.ld, _rows(rows, lay.ld, "rows", B), _rows(attrs, lay.attrs_ld, "attrs", B),
                                    lay.attrs_ld, _stream()), "ali_cf_input_fwd")
    return rows, attrs


def cf_input_step(lay: CfLayout, g_rows, rows, attrs, raw, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, graw=None):
    """Backward of ``cf_input_fwd`` from the input rows' gradient and torch.optim.Adam's update of ``raw`` (moments
    ``m`` / ``v``, per-row int32 counters ``step`` of completed steps) in one launch (include/ali_hip.h:
    ali_cf_input_step).  ``graw`` (optional [B, raw_ld]) receives the gradient of the trained columns."""
    lib = _lib.load()
    B = raw.shape[0]
    _lib.check(lib.ali_cf_input_step(_rows(g_rows, lay.ld, "g_rows", B), lay.ld, _rows(rows, lay.ld, "rows", B),
                                     _rows(attrs, lay.attrs_ld, "attrs", B), lay.attrs_ld, lay._segs, len(lay.segments),
                                     lay._tabs, len(lay.tables), B, _rows(raw, lay.raw_ld, "raw", B),
                                     _rows(m, lay.raw_ld, "m", B), _rows(v, lay.raw_ld, "v", B), lay.raw_ld, lay.given_ld,
                                     _i32(step, "step", B), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                     None if graw is None else _rows(graw, lay.raw_ld, "graw", B), _stream()),
               "ali_cf_input_step")


def cf_select(logit, metric, target, pred=None, order=None, n_hit=None):
    """Tail of the mixture sweep (include/ali_hip.h: ali_cf_select): logit [S, C], metric [S], target a one-element
    int32 device tensor.  Returns (pred [S], order [S], n_hit [1]) int32 device tensors: the first-maximum class per
    row, the rows with pred == target by ascending metric (stable) followed by the other rows, and their number."""
    lib = _lib.load()
    if logit.dim() != 2 or metric.numel() != logit.shape[0]:
        raise ValueError(f"cf_select: need [S, C] logits and S metric values, got {tuple(logit.shape)} and "
                         f"{tuple(metric.shape)}")
    S, C = logit.shape
    dev = logit.device
    pred = torch.empty(S, dtype=torch.int32, device=dev) if pred is None else pred
    order = torch.empty(S, dtype=torch.int32, device=dev) if order is None else order
    n_hit = torch.empty(1, dtype=torch.int32, device=dev) if n_hit is None else n_hit
    _lib.check(lib.ali_cf_select(_chk(logit, "logit"), _chk(metric, "metric"), _i32(target, "target", 1), S, C,
                                 _i32(pred, "pred", S), _i32(order, "order", S), _i32(n_hit, "n_hit", 1), _stream()),
               "ali_cf_select")
    return pred, order, n_hit


# ---------------------------------------------------------------------- expected gradients (csrc/attrib.hip)
def _eg_layout(lay: CfLayout, A, name):
    if lay.attrs_ld > A or any(s[0] != CF_COPY for s in lay.segments):
        raise ValueError(f"{name}: the layout must copy the columns of a [., {A}] attribute row (ALI_CF_COPY segments)")


def eg_input(lay: CfLayout, latent, x, bg, S, n_draws, idx=None, t=None, z=None, seed=0, dev_counter=None, offset=0,
             want_draws=False):
    """Explained rows x [R, A] and background bg [Nb, A] -> (generator input rows [R*S*n_draws, ld], delta [R, S, A],
    idx used [R, S] int32 or None, t used [R, S] or None) in one launch (include/ali_hip.h: ali_eg_input).  ``lay``: COPY
    segments from attribute columns (src_off) to row columns (dst_off), z in the row's first ``latent`` columns.  idx
    [R, S] int32, t [R, S], z [R, S, n_draws, latent]: given, or None: drawn under (seed, *dev_counter), ``offset``
    explained rows in (``ali_hip.rng.eg_index_reference`` / ``eg_t_reference`` / ``normal_reference``)."""
    lib = _lib.load()
    if x.dim() != 2 or bg.dim() != 2 or bg.shape[1] != x.shape[1]:
        raise ValueError(f"eg_input: need x [R, A] and bg [Nb, A], got {tuple(x.shape)} and {tuple(bg.shape)}")
    R, A = x.shape
    _eg_layout(lay, A, "eg_input")
    S, n_draws, latent = int(S), int(n_draws), int(latent)
    if idx is not None and tuple(idx.shape) != (R, S):
        raise ValueError(f"eg_input: idx must be [{R}, {S}], got {tuple(idx.shape)}")
    if t is not None and tuple(t.shape) != (R, S):
        raise ValueError(f"eg_input: t must be [{R}, {S}], got {tuple(t.shape)}")
    if z is not None and z.numel() != R * S * n_draws * latent:
        raise ValueError(f"eg_input: z must hold [{R}, {S}, {n_draws}, {latent}] values, got {tuple(z.shape)}")
    dev = x.device
    rows = torch.empty(R * S * n_draws, lay.ld, dtype=torch.float32, device=dev)
    delta = torch.empty(R, S, A, dtype=torch.float32, device=dev)
    idx_out = torch.empty(R, S, dtype=torch.int32, device=dev) if want_draws else None
    t_out = torch.empty(R, S, dtype=torch.float32, device=dev) if want_draws else None
    _lib.check(lib.ali_eg_input(_chk(x, "x"), _chk(bg, "bg"), None if idx is None else _i32(idx, "idx", R * S),
                                _opt(t, "t"), _opt(z, "z"), *_rng_args(seed, dev_counter, offset), lay._segs,
                                len(lay.segments), lay._tabs, len(lay.tables), R, S, n_draws, bg.shape[0], A, latent,
                                lay.n_log, lay.ld, _chk(rows), _chk(delta),
                                None if idx_out is None else c_void_p(idx_out.data_ptr()), _opt(t_out), _stream()),
               "ali_eg_input")
    return rows, delta, idx_out, t_out


def eg_seed(logit, c, scale, want_p=False, glogit=None):
    """glogit [N, K] = scale * p_c * ((k == c) - p_k) of the rows' softmax p, and p itself when asked (include/ali_hip.h:
    ali_eg_seed).  Returns (glogit, p or None)."""
    lib = _lib.load()
    if logit.dim() != 2:
        raise ValueError(f"eg_seed: need [N, K] logits, got {tuple(logit.shape)}")
    N, K = logit.shape
    if glogit is None:
        glogit = torch.empty_like(logit)
    p = torch.empty_like(logit) if want_p else None
    _lib.check(lib.ali_eg_seed(_chk(logit, "logit"), N, K, int(c), float(scale), _chk(glogit, "glogit"), _opt(p),
                               _stream()), "ali_eg_seed")
    return glogit, p


def eg_reduce(lay: CfLayout, g_rows, delta, n_draws, phi, c):
    """phi[:, c, :] ([R, C, A]) <- sum over (sample, draw) of delta [R, S, A] times the attribute gradient of the input
    rows' gradient g_rows [R*S*n_draws, ld] (include/ali_hip.h: ali_eg_reduce); the other classes stay as they are."""
    lib = _lib.load()
    R, S, A = delta.shape
    _eg_layout(lay, A, "eg_reduce")
    if phi.dim() != 3 or phi.shape[0] != R or phi.shape[2] != A:
        raise ValueError(f"eg_reduce: phi must be [{R}, C, {A}], got {tuple(phi.shape)}")
    ws = workspace(delta.device)
    _lib.check(lib.ali_eg_reduce(_rows(g_rows, lay.ld, "g_rows", R * S * int(n_draws)), lay.ld, _chk(delta, "delta"),
                                 lay._segs, len(lay.segments), lay._tabs, len(lay.tables), R, S, int(n_draws), A,
                                 phi.shape[1], int(c), _chk(phi, "phi"), c_void_p(ws.data_ptr()), ws.numel(), _stream()),
               "ali_eg_reduce")
    return phi


# ---------------------------------------------------------------------- the contrastive family (csrc/contrast.hip)
def _ct_f32(t, n, name):
    if t.numel() != n:
        raise ValueError(f"{name}: need {n} elements, got {tuple(t.shape)}")
    return _chk(t, name)


def ct_attack(logit, B, t0=None, c=None, kappa=0.0, eval_off=0, grad_off=0, seed_ld=None):
    """Evaluation and attack seed of B search rows (include/ali_hip.h: ali_ct_attack): logit [R, C]; row eval_off + b is
    evaluated (first arg-max, success against t0 [B] int32), row grad_off + b attacked under c [B] and ``kappa``.
    Returns (seed [B, seed_ld], A [B], pred [B] int32, succ [B] int32); ``t0`` None: (None, None, pred, None)."""
    lib = _lib.load()
    if logit.dim() != 2:
        raise ValueError(f"ct_attack: need [R, C] logits, got {tuple(logit.shape)}")
    R, C = logit.shape
    B = int(B)
    dev = logit.device
    pred = torch.empty(B, dtype=torch.int32, device=dev)
    seed = A = succ = None
    ld = C if seed_ld is None else int(seed_ld)
    if t0 is not None:
        seed = torch.empty(B, ld, dtype=torch.float32, device=dev)
        A = torch.empty(B, dtype=torch.float32, device=dev)
        succ = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.ali_ct_attack(_chk(logit, "logit"), R, C, B, int(eval_off), int(grad_off),
                                 None if t0 is None else _i32(t0, "t0", B), None if t0 is None else _ct_f32(c, B, "c"),
                                 float(kappa), _opt(seed), ld, _opt(A), _i32(pred, "pred"),
                                 None if succ is None else _i32(succ, "succ"), _stream()), "ali_ct_attack")
    return seed, A, pred, succ


def ct_book(v, dist, succ, pred, it, K, best, best_dist, best_label, found, round_succ, ctab, copied=None):
    """Best-so-far and, at it == K, the binary search on c (include/ali_hip.h: ali_ct_book): v, best [B, N]; ctab
    [3, B] = (c, c_lo, c_hi).  Returns copied [B] int32: the rows whose v went into best in this launch."""
    lib = _lib.load()
    B = v.shape[0]
    N = v.numel() // B
    if tuple(ctab.shape) != (3, B) or best.shape != v.shape:
        raise ValueError(f"ct_book: v {tuple(v.shape)}, best {tuple(best.shape)} and ctab {tuple(ctab.shape)} (need "
                         f"[3, {B}]) do not belong together")
    if copied is None:
        copied = torch.empty(B, dtype=torch.int32, device=v.device)
    _lib.check(lib.ali_ct_book(_chk(v, "v"), _ct_f32(dist, B, "dist"), _i32(succ, "succ", B), _i32(pred, "pred", B),
                               _i32(it, "it", B), int(K), B, N, _chk(best, "best"), _ct_f32(best_dist, B, "best_dist"),
                               _i32(best_label, "best_label", B), _i32(found, "found", B),
                               _i32(round_succ, "round_succ", B), _chk(ctab[0], "c"), _chk(ctab[1], "c_lo"),
                               _chk(ctab[2], "c_hi"), _i32(copied, "copied", B), _stream()), "ali_ct_book")
    return copied


def _ct_gx(gx, B, N, name):
    if gx.numel() % (B * N):
        raise ValueError(f"{name}: gx {tuple(gx.shape)} is no [B, N, channels] gradient of {B} rows of {N} pixels")
    return _chk(gx, "gx"), gx.numel() // (B * N)


def ct_cem_update(gx, v, y, x0, lo, hi, it, rnd, K, lr, beta, clip, l1, l2, dist, gnorm):
    """One FISTA step of the pertinent-negative search on every row, or the start of the next round where it == K
    (include/ali_hip.h: ali_ct_cem_update): gx the classifier's input gradient at y ([B, N] or NHWC [B, H, W, Cpad],
    plane 0), v / y / x0 [B, N], everything else [B].  In place."""
    lib = _lib.load()
    B = v.shape[0]
    N = v.numel() // B
    g, gs = _ct_gx(gx, B, N, "ct_cem_update")
    _lib.check(lib.ali_ct_cem_update(g, gs, _chk(v, "v"), _ct_f32(y, B * N, "y"), _ct_f32(x0, B * N, "x0"),
                                     _ct_f32(lo, B, "lo"), _ct_f32(hi, B, "hi"), _i32(it, "it", B), _i32(rnd, "rnd", B),
                                     int(K), float(lr), float(beta), float(clip), B, N, _ct_f32(l1, B, "l1"),
                                     _ct_f32(l2, B, "l2"), _ct_f32(dist, B, "dist"), _ct_f32(gnorm, B, "gnorm"),
                                     _stream()), "ali_ct_cem_update")


def ct_pp_attack(logit, B, t0, c, kappa=0.0, eval_off=0, grad_off=0, seed_ld=None):
    """``ct_attack`` of the pertinent-positive search (include/ali_hip.h: ali_ct_pp_attack): succ = (pred == t0), the
    hinge max(0, other - own + kappa) and its seed c * (e_other - e_t0).  t0 is required.  Returns (seed [B, seed_ld],
    A [B], pred [B] int32, succ [B] int32)."""
    lib = _lib.load()
    if logit.dim() != 2:
        raise ValueError(f"ct_pp_attack: need [R, C] logits, got {tuple(logit.shape)}")
    R, C = logit.shape
    B = int(B)
    dev = logit.device
    ld = C if seed_ld is None else int(seed_ld)
    seed = torch.empty(B, ld, dtype=torch.float32, device=dev)
    A = torch.empty(B, dtype=torch.float32, device=dev)
    pred = torch.empty(B, dtype=torch.int32, device=dev)
    succ = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.ali_ct_pp_attack(_chk(logit, "logit"), R, C, B, int(eval_off), int(grad_off), _i32(t0, "t0", B),
                                    _ct_f32(c, B, "c"), float(kappa), _chk(seed, "seed"), ld, _chk(A, "A"),
                                    _i32(pred, "pred"), _i32(succ, "succ"), _stream()), "ali_ct_pp_attack")
    return seed, A, pred, succ


def ct_pp_update(gx, v, y, x0, background, it, rnd, K, lr, beta, clip, l1, l2, dist, gnorm):
    """One FISTA step of the pertinent-positive search on every row, or the start of the next round (v = y = the
    background) where it == K (include/ali_hip.h: ali_ct_pp_update): gx the classifier's input gradient at y ([B, N]
    or NHWC [B, H, W, Cpad], plane 0), v / y / x0 [B, N], ``background`` a float (used as fp32), everything else [B].
    In place."""
    lib = _lib.load()
    B = v.shape[0]
    N = v.numel() // B
    g, gs = _ct_gx(gx, B, N, "ct_pp_update")
    _lib.check(lib.ali_ct_pp_update(g, gs, _chk(v, "v"), _ct_f32(y, B * N, "y"), _ct_f32(x0, B * N, "x0"),
                                    float(background), _i32(it, "it", B), _i32(rnd, "rnd", B), int(K), float(lr),
                                    float(beta), float(clip), B, N, _ct_f32(l1, B, "l1"), _ct_f32(l2, B, "l2"),
                                    _ct_f32(dist, B, "dist"), _ct_f32(gnorm, B, "gnorm"), _stream()),
               "ali_ct_pp_update")


def ct_ce_update(gx, v, x0, lo, hi, m, v2, it, rnd, K, lr, gamma, clip, l1, gnorm, betas=(0.9, 0.999), eps=1e-8):
    """One Adam step of the counterfactual search on every row, or the start of the next round where it == K
    (include/ali_hip.h: ali_ct_ce_update): gx the classifier's input gradient at v, v / x0 / m / v2 [B, N].  In place."""
    lib = _lib.load()
    B = v.shape[0]
    N = v.numel() // B
    g, gs = _ct_gx(gx, B, N, "ct_ce_update")
    _lib.check(lib.ali_ct_ce_update(g, gs, _chk(v, "v"), _ct_f32(x0, B * N, "x0"), _ct_f32(lo, B, "lo"),
                                    _ct_f32(hi, B, "hi"), _ct_f32(m, B * N, "m"), _ct_f32(v2, B * N, "v2"),
                                    _i32(it, "it", B), _i32(rnd, "rnd", B), int(K), float(lr), float(gamma), float(clip),
                                    float(betas[0]), float(betas[1]), float(eps), B, N, _ct_f32(l1, B, "l1"),
                                    _ct_f32(gnorm, B, "gnorm"), _stream()), "ali_ct_ce_update")


# ---------------------------------------------------------------------- the counterfactual metrics (csrc/cfmetrics.hip)
def mse(y, x, gscale=1.0, want_grad=True, tanh_out=False):
    """``mean((y - x)^2)`` over all elements as a 0-d device tensor, and its gradient with respect to ``y`` times
    ``gscale`` -- with ``tanh_out`` times ``1 - y^2``: the gradient of the pre-activation of the tanh that produced
    ``y`` -- in one launch (include/ali_hip.h: ali_mse).  Returns (loss, grad or None)."""
    lib = _lib.load()
    if y.shape != x.shape or y.numel() == 0:
        raise ValueError(f"mse: need two non-empty tensors of one shape, got {tuple(y.shape)} and {tuple(x.shape)}")
    loss = torch.empty(1, dtype=torch.float32, device=y.device)
    grad = torch.empty_like(y) if want_grad else None
    ws = workspace(y.device)
    _lib.check(lib.ali_mse(_chk(y, "y"), _chk(x, "x"), y.numel(), float(gscale), int(bool(tanh_out)), _chk(loss),
                           _opt(grad), c_void_p(ws.data_ptr()), ws.numel(), _stream()), "ali_mse")
    return loss.reshape(()), grad


def cf_recon(x, recon, orig, target, out=None):
    """The reconstruction columns of morphomnist_cf_metrics.py for B rows (include/ali_hip.h: ali_cf_recon): x [B, N],
    recon [A, B, N] (any plane and row strides, unit element stride; plane A - 1 is the all-classes autoencoder), orig
    and target int32 [B].  Returns [B, 4] = (l1, o_rec, t_rec, all_rec); a label outside [0, A - 1) gives NaN."""
    lib = _lib.load()
    if x.dim() != 2 or recon.dim() != 3 or tuple(recon.shape[1:]) != tuple(x.shape) or recon.shape[0] < 2:
        raise ValueError(f"cf_recon: need x [B, N] and recon [A >= 2, B, N], got {tuple(x.shape)} and "
                         f"{tuple(recon.shape)}")
    A, B, N = recon.shape
    if recon.stride(2) != 1 and N > 1:
        raise ValueError("cf_recon: the elements of a recon row must be contiguous")
    ld_row = recon.stride(1) if B > 1 else max(recon.stride(1), N)
    if out is None:
        out = torch.empty(B, 4, dtype=torch.float32, device=x.device)
    _lib.check(lib.ali_cf_recon(_chk(x, "x"), _ptr(recon), ld_row, recon.stride(0), _i32(orig, "orig", B),
                                _i32(target, "target", B), A, B, N, _chk(out, "out"), _stream()), "ali_cf_recon")
    return out


def oracle_scores(pred, ox, ocf):
    """The oracle columns of mnist_oracle_scores.py for B rows (include/ali_hip.h: ali_oracle_scores): pred int32 [B],
    ox and ocf [J, B, C] logits of the J oracles on the originals and on the counterfactuals (contiguous [B, C] planes,
    the same plane stride in both: two halves of one buffer will do).  Returns (os int32
    [B, J] = pred == ocf's first arg-max, lvs [B, J] = the Jensen-Shannon divergence of the two softmaxes)."""
    lib = _lib.load()
    if ox.dim() != 3 or ox.shape != ocf.shape:
        raise ValueError(f"oracle_scores: need two [J, B, C] logit tensors, got {tuple(ox.shape)} and {tuple(ocf.shape)}")
    J, B, C = ox.shape
    for t in (ox, ocf):
        if not (t.is_cuda and t.dtype == torch.float32 and t[0].is_contiguous() and t.stride(0) == ox.stride(0)):
            raise ValueError("oracle_scores: need fp32 CUDA logits with contiguous [B, C] planes and one plane stride")
    os_ = torch.empty(B, J, dtype=torch.int32, device=ox.device)
    lvs = torch.empty(B, J, dtype=torch.float32, device=ox.device)
    _lib.check(lib.ali_oracle_scores(_i32(pred, "pred", B), _ptr(ox), _ptr(ocf), max(ox.stride(0), B * C), J, B, C,
                                     _i32(os_, "os"), _chk(lvs, "lvs"), _stream()), "ali_oracle_scores")
    return os_, lvs


# ---------------------------------------------------------------------- the counterfactual identity metrics (csrc/cfeval.hip)
def _pitched_rows(t, name):
    """a [rows, D] fp32 CUDA view with unit column stride -> (pointer, row pitch in floats)"""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.numel() > 0
            and (t.shape[1] == 1 or t.stride(1) == 1)):
        raise ValueError(f"{name}: need a non-empty [rows, D] fp32 CUDA view with unit column stride, got {t.dtype} "
                         f"{tuple(t.shape)} strides {tuple(t.stride())}")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    if ld < t.shape[1]:
        raise ValueError(f"{name}: rows overlap (row stride {ld} < {t.shape[1]} columns)")
    return c_void_p(t.data_ptr()), ld


def _f64(t, shape, name):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: need a contiguous float64 CUDA tensor of shape {tuple(shape)}")
    return c_void_p(t.data_ptr())


def group_moments(rows, order, start, n_owners, n_classes):
    """The bank of ``manifold_err`` (include/ali_hip.h: ali_group_moments): rows [N, D] (any row pitch), order int32
    [<= N] = the row indices sorted by cell (stable), start int32 [O * C + 1] = the cells' offsets into it, cell =
    owner * C + class.  Returns (S, Q [O * C, D], TS, TQ [C, D]) in float64: column sums and sums of squares per cell
    and per class."""
    lib = _lib.load()
    O, C = int(n_owners), int(n_classes)
    ptr, ld = _pitched_rows(rows, "rows")
    N, D = rows.shape
    dev = rows.device
    S, Q = (torch.empty(O * C, D, dtype=torch.float64, device=dev) for _ in range(2))
    TS, TQ = (torch.empty(C, D, dtype=torch.float64, device=dev) for _ in range(2))
    _lib.check(lib.ali_group_moments(ptr, ld, N, D, _i32(order, "order"), order.numel(), _i32(start, "start", O * C + 1),
                                     O, C, _f64(S, S.shape, "S"), _f64(Q, Q.shape, "Q"), _f64(TS, TS.shape, "TS"),
                                     _f64(TQ, TQ.shape, "TQ"), _stream()), "ali_group_moments")
    return S, Q, TS, TQ


def manifold_err(cf, owner, cls, S, Q, TS, TQ, cnt, tcnt, out=None):
    """(same, other, ratio) per row of cf [M, D] (any row pitch) against the bank of ``group_moments`` (include/ali_hip.h:
    ali_manifold_err): owner, cls int32 [M] on the device, cnt int32 [O * C], tcnt int32 [C].  Returns out [M, 3]."""
    lib = _lib.load()
    ptr, ld = _pitched_rows(cf, "cf")
    M, D = cf.shape
    C = TS.shape[0]
    O = S.shape[0] // max(C, 1)
    if out is None:
        out = torch.empty(M, 3, dtype=torch.float32, device=cf.device)
    if tuple(out.shape) != (M, 3):
        raise ValueError(f"manifold_err: out must be [{M}, 3], got {tuple(out.shape)}")
    ws = workspace(cf.device)
    _lib.check(lib.ali_manifold_err(ptr, ld, M, D, _i32(owner, "owner", M), _i32(cls, "cls", M),
                                    _f64(S, (O * C, D), "S"), _f64(Q, (O * C, D), "Q"), _f64(TS, (C, D), "TS"),
                                    _f64(TQ, (C, D), "TQ"), _i32(cnt, "cnt", O * C), _i32(tcnt, "tcnt", C), O, C,
                                    _chk(out, "out"), c_void_p(ws.data_ptr()), ws.numel(), _stream()),
               "ali_manifold_err")
    return out


# ---------------------------------------------------------------------- the morphomnist family (csrc/morpho.hip)
MORPHO_MAX_SIDE = 512            # H * scale and W * scale of one launch
WS_RESERVED = 4096               # ALI_WS_RESERVED: the head of every workspace, in front of the scratch


def _i32s(t, shape, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: need a contiguous int32 CUDA tensor of shape {tuple(shape)}, got {t.dtype} "
                         f"{tuple(t.shape)}")
    return c_void_p(t.data_ptr())


def _morpho_images(x, scale):
    """x [B, H, W] fp32 CUDA with contiguous images -> (pointer, image pitch, B, H, W, Hh, Wh)"""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0 and x[0].is_contiguous()):
        raise ValueError(f"morpho: need fp32 CUDA images [B, H, W] with contiguous images, got {x.dtype} "
                         f"{tuple(x.shape)} strides {tuple(x.stride())}")
    B, H, W = x.shape
    scale = int(scale)
    if scale < 1 or H * scale > MORPHO_MAX_SIDE or W * scale > MORPHO_MAX_SIDE:
        raise ValueError(f"morpho: {H} x {W} images at scale {scale} exceed the limit of {MORPHO_MAX_SIDE} x "
                         f"{MORPHO_MAX_SIDE} up-sampled pixels")
    ld = x.stride(0) if B > 1 else max(x.stride(0), H * W)
    if ld < H * W:
        raise ValueError("morpho: images overlap")
    return c_void_p(x.data_ptr()), ld, B, H, W, H * scale, W * scale


def _morpho_ws(ws, device):
    ws = workspace(device) if ws is None else ws
    if not (ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
        raise ValueError("morpho: the workspace is a contiguous uint8 CUDA tensor")
    return c_void_p(ws.data_ptr()), ws.numel()


def morpho_binarise(x, scale, AH=None, AW=None, threshold=0.5, ws=None):
    """Up-sample and binarise x [B, H, W] (include/ali_hip.h: ali_morpho_binarise); AH [H * scale, H], AW [W * scale, W]
    fp32 on the device (not needed at scale 1).  Returns (bin int32 [B, Hh, ceil(Wh / 32)] bitmap words, fg int32 [B],
    hstats float64 [B, 8] = min, max and the six raw moment sums of the up-sampled image)."""
    lib = _lib.load()
    ptr, ld, B, H, W, Hh, Wh = _morpho_images(x, scale)
    if scale > 1:
        for a, n in ((AH, H), (AW, W)):
            if a is None or tuple(a.shape) != (n * scale, n):
                raise ValueError(f"morpho_binarise: need an expand operator of shape {(n * scale, n)}")
    dev = x.device
    bits = torch.empty(B, Hh, (Wh + 31) // 32, dtype=torch.int32, device=dev)
    fg = torch.empty(B, dtype=torch.int32, device=dev)
    hstats = torch.empty(B, 8, dtype=torch.float64, device=dev)
    wp, wn = _morpho_ws(ws, dev)
    _lib.check(lib.ali_morpho_binarise(ptr, ld, B, H, W, int(scale), None if scale == 1 else _chk(AH, "AH"),
                                       None if scale == 1 else _chk(AW, "AW"), float(threshold),
                                       _i32(bits, "bin"), _i32(fg, "fg"), _f64(hstats, hstats.shape, "hstats"), wp, wn,
                                       _stream()), "ali_morpho_binarise")
    return bits, fg, hstats


def morpho_edt(bits, Wh, ws=None):
    """The exact squared distance map of the bitmaps bits [B, Hh, ceil(Wh / 32)] (include/ali_hip.h: ali_morpho_edt).
    Returns (d2 int32 [B, Hh, Wh], status int32 [B]: 1 for an image without background, whose d2 is not written)."""
    lib = _lib.load()
    B, Hh, wpr = bits.shape
    if wpr != (Wh + 31) // 32:
        raise ValueError(f"morpho_edt: {wpr} words per row do not hold {Wh} pixels")
    d2 = torch.empty(B, Hh, Wh, dtype=torch.int32, device=bits.device)
    status = torch.empty(B, dtype=torch.int32, device=bits.device)
    wp, wn = _morpho_ws(ws, bits.device)
    _lib.check(lib.ali_morpho_edt(_i32(bits, "bin"), B, Hh, Wh, _i32(d2, "d2"), _i32(status, "status"), wp, wn,
                                  _stream()), "ali_morpho_edt")
    return d2, status


def morpho_thin(bits, d2, fg, status, keep16, seed=0, ws=None):
    """The ordered thinning (include/ali_hip.h: ali_morpho_thin) of the bitmaps under the keys of d2 and seed; keep16: the
    512-bit keep table as a uint32 numpy array [16].  Returns the skeleton bitmaps; ``status`` is updated in place."""
    lib = _lib.load()
    B, Hh, Wh = d2.shape
    keep16 = np.ascontiguousarray(keep16, dtype=np.uint32)
    if keep16.shape != (16,):
        raise ValueError("morpho_thin: keep16 holds 16 words")
    skel = torch.empty_like(bits)
    wp, wn = _morpho_ws(ws, bits.device)
    _lib.check(lib.ali_morpho_thin(_i32s(bits, (B, Hh, (Wh + 31) // 32), "bin"), _i32(d2, "d2"), _i32(fg, "fg", B), B, Hh,
                                   Wh, int(seed) & (2 ** 64 - 1), keep16.ctypes.data_as(c_void_p), _i32(skel, "skel"),
                                   _i32(status, "status", B), wp, wn, _stream()), "ali_morpho_thin")
    return skel


def morpho_measure(x, scale, skel, d2, fg, hstats, status, out=None):
    """The measures of x [B, H, W] (include/ali_hip.h: ali_morpho_measure).  Returns (counts int32 [B, 4] = foreground,
    skeleton, straight pairs, diagonal pairs; values fp32 [B, 5] = area, length, thickness, intensity, shear;
    slant_hires fp32 [B]); ``out``: three such tensors to write into."""
    lib = _lib.load()
    ptr, ld, B, H, W, Hh, Wh = _morpho_images(x, scale)
    dev = x.device
    if out is None:
        out = (torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, 5, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.float32, device=dev))
    counts, values, slant = out
    if tuple(values.shape) != (B, 5) or tuple(slant.shape) != (B,):
        raise ValueError("morpho_measure: out is (counts [B, 4], values [B, 5], slant_hires [B])")
    _lib.check(lib.ali_morpho_measure(ptr, ld, B, H, W, int(scale), _i32s(skel, (B, Hh, (Wh + 31) // 32), "skel"),
                                      _i32s(d2, (B, Hh, Wh), "d2"), _i32(fg, "fg", B), _f64(hstats, (B, 8), "hstats"),
                                      _i32(status, "status", B), _i32s(counts, (B, 4), "counts"), _chk(values, "values"),
                                      _chk(slant, "slant_hires"), _stream()), "ali_morpho_measure")
    return counts, values, slant


MORPHO_BOUNDS_LDS_T = 28 * 448   # floats of ali_morpho_bounds' T kept in LDS; a larger T goes to the workspace


def morpho_bounds_scratch_bytes(H, W, scale):
    """the workspace ali_morpho_bounds needs per image behind the reserved head: T when it does not fit in LDS"""
    return 4 * H * W * scale if scale > 1 and H * W * scale > MORPHO_BOUNDS_LDS_T else 0


def morpho_bounds(x, scale, AH=None, AW=None, bound_frac=0.02, ws=None, debug=False, out=None):
    """The bounding parallelogram of x [B, H, W] (include/ali_hip.h: ali_morpho_bounds) on hires = expand(x - min x);
    AH, AW as ``morpho_binarise`` takes them.  Returns bounds float64 [B, 6] = left, right, top, bottom, shear, middle in
    up-sampled pixels, and with ``debug`` also (hcdf float64 [B, W * scale], vcdf float64 [B, H * scale]); ``out``: the
    bounds tensor to write into."""
    lib = _lib.load()
    ptr, ld, B, H, W, Hh, Wh = _morpho_images(x, scale)
    if scale > 1:
        for a, n in ((AH, H), (AW, W)):
            if a is None or tuple(a.shape) != (n * scale, n):
                raise ValueError(f"morpho_bounds: need an expand operator of shape {(n * scale, n)}")
    bound_frac = float(bound_frac)
    if not 0.0 < bound_frac < 1.0:
        raise ValueError(f"morpho_bounds: 0 < bound_frac < 1, got {bound_frac}")
    dev = x.device
    bounds = torch.empty(B, 6, dtype=torch.float64, device=dev) if out is None else out
    hcdf = torch.empty(B, Wh, dtype=torch.float64, device=dev) if debug else None
    vcdf = torch.empty(B, Hh, dtype=torch.float64, device=dev) if debug else None
    wp, wn = _morpho_ws(ws, dev)
    _lib.check(lib.ali_morpho_bounds(ptr, ld, B, H, W, int(scale), None if scale == 1 else _chk(AH, "AH"),
                                     None if scale == 1 else _chk(AW, "AW"), bound_frac,
                                     _f64(bounds, (B, 6), "bounds"), None if hcdf is None else _f64(hcdf, (B, Wh), "hcdf"),
                                     None if vcdf is None else _f64(vcdf, (B, Hh), "vcdf"), wp, wn, _stream()),
               "ali_morpho_bounds")
    return (bounds, hcdf, vcdf) if debug else bounds


def morpho_width(x, scale, bits, fg, target, AH=None, AW=None, bound_frac=0.02, ws=None, debug=False):
    """The measuring half of ``SetWidth`` (include/ali_hip.h: ali_morpho_width): x, AH, AW as ``morpho_binarise`` takes
    them, bits and fg what it returned for x; target: float64 [B], the target widths.  Returns (sums int64 [B, 6] of the
    bitmaps, wb float64 [B, 6] = left, right, shear, cx, cy, factor, status int32 [B]), and with ``debug`` also hcdf
    float64 [B, W * scale].  The scratch is ``morpho_bounds_scratch_bytes``."""
    lib = _lib.load()
    ptr, ld, B, H, W, Hh, Wh = _morpho_images(x, scale)
    if scale > 1:
        for a, n in ((AH, H), (AW, W)):
            if a is None or tuple(a.shape) != (n * scale, n):
                raise ValueError(f"morpho_width: need an expand operator of shape {(n * scale, n)}")
    bound_frac = float(bound_frac)
    if not 0.0 < bound_frac < 1.0:
        raise ValueError(f"morpho_width: 0 < bound_frac < 1, got {bound_frac}")
    dev = x.device
    sums = torch.empty(B, 6, dtype=torch.int64, device=dev)
    wb = torch.empty(B, 6, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    hcdf = torch.empty(B, Wh, dtype=torch.float64, device=dev) if debug else None
    wp, wn = _morpho_ws(ws, dev)
    _lib.check(lib.ali_morpho_width(ptr, ld, B, H, W, int(scale), None if scale == 1 else _chk(AH, "AH"),
                                    None if scale == 1 else _chk(AW, "AW"),
                                    _i32s(bits, (B, Hh, (Wh + 31) // 32), "bin"), _i32(fg, "fg", B), bound_frac,
                                    _f64(target, (B,), "target"), c_void_p(sums.data_ptr()), c_void_p(wb.data_ptr()),
                                    _i32(status, "status"), None if hcdf is None else _f64(hcdf, (B, Wh), "hcdf"), wp, wn,
                                    _stream()), "ali_morpho_width")
    return (sums, wb, status, hcdf) if debug else (sums, wb, status)


def morpho_affine_reduce(bits, H, W, scale, sums, wb, status, RH=None, RW=None, ws=None, debug=False, out=None):
    """The warp of ``SetWidth`` and ``downscale`` (include/ali_hip.h: ali_morpho_affine_reduce) of the bitmaps bits [B, H
    * scale, ceil(W * scale / 32)] with sums, wb and status as ``morpho_width`` returned them; RH, RW as
    ``morpho_shear_reduce`` takes them.  Returns (q fp32 [B, H, W] grey levels, status int32 [B]: 4 where q is 0
    everywhere), and with ``debug`` also (raw fp32 [B, H, W], the warped bitmaps' words like bits); ``out``: the tensor q
    is written into."""
    lib = _lib.load()
    scale = int(scale)
    Hh, Wh = H * scale, W * scale
    if H < 1 or W < 1 or scale < 1 or Hh > MORPHO_MAX_SIDE or Wh > MORPHO_MAX_SIDE:
        raise ValueError(f"morpho: {H} x {W} images at scale {scale} exceed the limit of {MORPHO_MAX_SIDE} x "
                         f"{MORPHO_MAX_SIDE} up-sampled pixels")
    if not (bits.is_cuda and bits.dim() == 3 and tuple(bits.shape[1:]) == (Hh, (Wh + 31) // 32)):
        raise ValueError(f"morpho_affine_reduce: bits is [B, {Hh}, {(Wh + 31) // 32}]")
    B = bits.shape[0]
    if scale > 1:
        for a, n in ((RH, H), (RW, W)):
            if a is None or tuple(a.shape) != (n, n * scale):
                raise ValueError(f"morpho_affine_reduce: need a reduce operator of shape {(n, n * scale)}")
    dev = bits.device
    q = torch.empty(B, H, W, dtype=torch.float32, device=dev) if out is None else out
    if tuple(q.shape) != (B, H, W):
        raise ValueError(f"morpho_affine_reduce: out is [{B}, {H}, {W}]")
    status_out = torch.empty(B, dtype=torch.int32, device=dev)
    raw = torch.empty(B, H, W, dtype=torch.float32, device=dev) if debug else None
    warped = torch.empty_like(bits) if debug else None
    wp, wn = _morpho_ws(ws, dev)
    _lib.check(lib.ali_morpho_affine_reduce(_i32s(bits, (B, Hh, (Wh + 31) // 32), "bin"),
                                            _typed(sums, torch.int64, (B, 6), "sums"), _f64(wb, (B, 6), "wb"),
                                            _i32(status, "status", B), B, H, W, scale,
                                            None if scale == 1 else _f64(RH, (H, Hh), "RH"),
                                            None if scale == 1 else _f64(RW, (W, Wh), "RW"), _chk(q, "q"), _opt(raw, "raw"),
                                            None if warped is None else _i32(warped, "warped"),
                                            _i32(status_out, "status_out"), wp, wn, _stream()),
               "ali_morpho_affine_reduce")
    return (q, status_out, raw, warped) if debug else (q, status_out)


MORPHO_MAX_RADIUS = 64           # the largest radius of ali_morpho_reshape's half-width table


def _typed(t, dtype, shape, name):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: need a contiguous {dtype} CUDA tensor of shape {tuple(shape)}, got {t.dtype} "
                         f"{tuple(t.shape)}")
    return c_void_p(t.data_ptr())


def morpho_reshape(bits, Wh, thickness, target, status, half, scale, ws=None):
    """``SetThickness`` on the bitmaps bits [B, Hh, ceil(Wh / 32)] (include/ali_hip.h: ali_morpho_reshape).  thickness:
    fp32 [B], any stride (a column of ``morpho_measure``'s values); target: fp32 [B] or None (radius 0); half: int16
    [max_radius + 1, 2 * max_radius + 1] on the device (``morphomnist.perturb.half_width_table``).  Returns (the
    dilated / eroded bitmaps, signed radius int32 [B], moment sums int64 [B, 6], status int32 [B])."""
    lib = _lib.load()
    if not (bits.is_cuda and bits.dtype == torch.int32 and bits.dim() == 3 and bits.is_contiguous()):
        raise ValueError("morpho_reshape: bits is a contiguous int32 CUDA tensor [B, Hh, wpr]")
    B, Hh, wpr = bits.shape
    scale = int(scale)
    if wpr != (Wh + 31) // 32:
        raise ValueError(f"morpho_reshape: {wpr} words per row do not hold {Wh} pixels")
    if scale < 1 or Hh > MORPHO_MAX_SIDE or Wh > MORPHO_MAX_SIDE:
        raise ValueError(f"morpho: {Hh} x {Wh} bitmaps exceed the limit of {MORPHO_MAX_SIDE} x {MORPHO_MAX_SIDE} "
                         f"up-sampled pixels, or scale {scale} < 1")
    if not (thickness.is_cuda and thickness.dtype == torch.float32 and tuple(thickness.shape) == (B,)
            and (B == 1 or thickness.stride(0) >= 1)):
        raise ValueError(f"morpho_reshape: thickness is an fp32 CUDA tensor [{B}]")
    max_radius = half.shape[0] - 1 if half.dim() == 2 else -1
    if not 0 <= max_radius <= MORPHO_MAX_RADIUS:
        raise ValueError(f"morpho_reshape: the half-width table holds radii 0 .. max_radius <= {MORPHO_MAX_RADIUS}")
    dev = bits.device
    out = torch.empty_like(bits)
    radius = torch.empty(B, dtype=torch.int32, device=dev)
    sums = torch.empty(B, 6, dtype=torch.int64, device=dev)
    status_out = torch.empty(B, dtype=torch.int32, device=dev)
    wp, wn = _morpho_ws(ws, dev)
    _lib.check(lib.ali_morpho_reshape(c_void_p(bits.data_ptr()), c_void_p(thickness.data_ptr()),
                                      max(thickness.stride(0), 1), None if target is None else
                                      _typed(target, torch.float32, (B,), "target"), _i32(status, "status", B),
                                      _typed(half, torch.int16, (max_radius + 1, 2 * max_radius + 1), "half"),
                                      max_radius, B, Hh, Wh, scale, _i32(out, "out"), _i32(radius, "radius"),
                                      c_void_p(sums.data_ptr()), _i32(status_out, "status_out"), wp, wn, _stream()),
               "ali_morpho_reshape")
    return out, radius, sums, status_out


def morpho_shear_reduce(bits, H, W, scale, sums, target_shear, status, RH=None, RW=None, ws=None, debug=False):
    """``SetSlant`` and ``downscale`` (include/ali_hip.h: ali_morpho_shear_reduce) of the bitmaps bits [B, H * scale,
    ceil(W * scale / 32)] with moment sums int64 [B, 6]; target_shear: float64 [B] = -tan(slant), or None (no shear);
    RH [H, H * scale], RW [W, W * scale] float64 on the device (not needed at scale 1).  Returns (q fp32 [B, H, W] grey
    levels, shear float64 [B] = u11 / u02 of the bitmaps), and with ``debug`` also (raw fp32 [B, H, W], shifts int32
    [B, H * scale])."""
    lib = _lib.load()
    scale = int(scale)
    Hh, Wh = H * scale, W * scale
    if H < 1 or W < 1 or scale < 1 or Hh > MORPHO_MAX_SIDE or Wh > MORPHO_MAX_SIDE:
        raise ValueError(f"morpho: {H} x {W} images at scale {scale} exceed the limit of {MORPHO_MAX_SIDE} x "
                         f"{MORPHO_MAX_SIDE} up-sampled pixels")
    if not (bits.is_cuda and bits.dim() == 3 and tuple(bits.shape[1:]) == (Hh, (Wh + 31) // 32)):
        raise ValueError(f"morpho_shear_reduce: bits is [B, {Hh}, {(Wh + 31) // 32}]")
    B = bits.shape[0]
    if scale > 1:
        for a, n in ((RH, H), (RW, W)):
            if a is None or tuple(a.shape) != (n, n * scale):
                raise ValueError(f"morpho_shear_reduce: need a reduce operator of shape {(n, n * scale)}")
    dev = bits.device
    q = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    shear = torch.empty(B, dtype=torch.float64, device=dev)
    raw = torch.empty(B, H, W, dtype=torch.float32, device=dev) if debug else None
    shifts = torch.empty(B, Hh, dtype=torch.int32, device=dev) if debug else None
    wp, wn = _morpho_ws(ws, dev)
    _lib.check(lib.ali_morpho_shear_reduce(_i32s(bits, (B, Hh, (Wh + 31) // 32), "bin"),
                                           _typed(sums, torch.int64, (B, 6), "sums"), None if target_shear is None else
                                           _f64(target_shear, (B,), "target_shear"), _i32(status, "status", B), B, H, W,
                                           scale, None if scale == 1 else _f64(RH, (H, Hh), "RH"),
                                           None if scale == 1 else _f64(RW, (W, Wh), "RW"), _chk(q, "q"), _opt(raw, "raw"),
                                           None if shifts is None else _i32(shifts, "shifts"),
                                           c_void_p(shear.data_ptr()), wp, wn, _stream()), "ali_morpho_shear_reduce")
    return (q, shear, raw, shifts) if debug else (q, shear)


def morpho_set_intensity(q, target, status, out=None):
    """``SetIntensity`` on grey-level images q [B, ...] (include/ali_hip.h: ali_morpho_set_intensity); target: fp32 [B]
    or None (no rescale).  Returns (images like q in 0 .. 255, median fp32 [B], status int32 [B]); ``out``: the tensor
    the images are written into."""
    lib = _lib.load()
    if q.dim() < 2 or q.numel() == 0:
        raise ValueError("morpho_set_intensity: q is [B, ...]")
    B = q.shape[0]
    N = q.numel() // B
    if N > MORPHO_MAX_SIDE * MORPHO_MAX_SIDE:
        raise ValueError(f"morpho: images of {N} pixels exceed the limit of {MORPHO_MAX_SIDE} x {MORPHO_MAX_SIDE}")
    out = torch.empty_like(q) if out is None else out
    if tuple(out.shape) != tuple(q.shape) or out.data_ptr() == q.data_ptr():
        raise ValueError("morpho_set_intensity: out is a tensor of q's shape, and not q")
    median = torch.empty(B, dtype=torch.float32, device=q.device)
    status_out = torch.empty(B, dtype=torch.int32, device=q.device)
    _lib.check(lib.ali_morpho_set_intensity(_chk(q, "q"), None if target is None else
                                            _typed(target, torch.float32, (B,), "target"), _i32(status, "status", B), B,
                                            N, _chk(out, "out"), _chk(median, "median"),
                                            _i32(status_out, "status_out"), _stream()), "ali_morpho_set_intensity")
    return out, median, status_out


MORPHO_MAX_DRAWS = 8             # locations one image draws per ali_morpho_locate (rng.MAX_DRAWS)
MORPHO_MAX_STAMP = 1024          # the largest brush radius of ali_morpho_local's fracture
MORPHO_KINDS = ("plain", "thin", "thick", "swell", "fracture")


def _morpho_bits(bits, Wh, who):
    if not (bits.is_cuda and bits.dtype == torch.int32 and bits.dim() == 3 and bits.is_contiguous()):
        raise ValueError(f"{who}: need a contiguous int32 CUDA tensor [B, Hh, wpr] of bitmap words")
    B, Hh, wpr = bits.shape
    if wpr != (Wh + 31) // 32:
        raise ValueError(f"{who}: {wpr} words per row do not hold {Wh} pixels")
    if B < 1 or Hh > MORPHO_MAX_SIDE or Wh > MORPHO_MAX_SIDE:
        raise ValueError(f"morpho: {Hh} x {Wh} bitmaps exceed the limit of {MORPHO_MAX_SIDE} x {MORPHO_MAX_SIDE} "
                         f"up-sampled pixels")
    return B, Hh, wpr


def morpho_complement(bits, Wh):
    """the complement of the bitmaps bits [B, Hh, ceil(Wh / 32)], pad bits 0 (what ``morpho_edt`` takes for ``d2c``)"""
    wpr = bits.shape[-1]
    mask = torch.full((wpr,), -1, dtype=torch.int32, device=bits.device)
    if Wh & 31:
        mask[-1:].fill_((1 << (Wh & 31)) - 1)                         # (a fill, not a host copy: capturable)
    return torch.bitwise_not(bits) & mask


def morpho_locate(skel, d2, status, kind, scale, prune_tips=None, prune_forks=None, num=3, seed=0, dev_counter=None,
                  offset=0):
    """Skeleton locations for the swellings and fractures of a batch (include/ali_hip.h: ali_morpho_locate).  skel, d2,
    status as ``morpho_thin`` / ``morpho_edt`` left them; kind int32 [B] (``MORPHO_KINDS``); prune_tips / prune_forks:
    the erase radii of a fracture in up-sampled pixels, or None; num: the locations of a fracture (a swelling draws
    one); (seed, dev_counter, offset): the "locate" stream, ``offset`` the images in front of image 0.  Returns
    (n_candidates int32 [B], fallback int32 [B], centres int32 [B, 8, 2] = (row, column), -1 where unused, endpoints
    int32 [B, 8, 4] = r0, c0, r1, c1)."""
    lib = _lib.load()
    B, Hh, Wh = d2.shape
    _morpho_bits(skel, Wh, "morpho_locate")
    if not 1 <= int(num) <= MORPHO_MAX_DRAWS:
        raise ValueError(f"morpho_locate: num in 1 .. {MORPHO_MAX_DRAWS}")
    radius = lambda r: -1 if r is None else int(r)
    if (prune_tips is not None and int(prune_tips) < 0) or (prune_forks is not None and int(prune_forks) < 0):
        raise ValueError("morpho_locate: a prune radius is >= 0, or None")
    dev = skel.device
    n_cand = torch.empty(B, dtype=torch.int32, device=dev)
    fallback = torch.empty(B, dtype=torch.int32, device=dev)
    centres = torch.empty(B, MORPHO_MAX_DRAWS, 2, dtype=torch.int32, device=dev)
    endpoints = torch.empty(B, MORPHO_MAX_DRAWS, 4, dtype=torch.int32, device=dev)
    seed, ctr, offset = _rng_args(seed, dev_counter, offset)
    _lib.check(lib.ali_morpho_locate(_i32s(skel, (B, Hh, (Wh + 31) // 32), "skel"), _i32s(d2, (B, Hh, Wh), "d2"),
                                     _i32(status, "status", B), _i32s(kind, (B,), "kind"), B, Hh, Wh, int(scale),
                                     radius(prune_tips), radius(prune_forks), int(num), seed, ctr, offset,
                                     _i32(n_cand, "n_candidates"), _i32(fallback, "fallback"), _i32(centres, "centres"),
                                     _i32(endpoints, "endpoints"), _stream()), "ali_morpho_locate")
    return n_cand, fallback, centres, endpoints


def morpho_local(bits, Wh, d2, d2c, thickness, status, kind, n_candidates, centres, endpoints, scale, thin_amount=.7,
                 thick_amount=1., swell_strength=3., swell_radius=7., frac_radius=12, num_frac=3):
    """The five Morpho-MNIST perturbations on the bitmaps bits [B, Hh, ceil(Wh / 32)] by kind int32 [B] (include/
    ali_hip.h: ali_morpho_local).  d2: the distance map; d2c: that of ``morpho_complement(bits)``, or None when no image
    is thickened; thickness: fp32 [B], any stride; n_candidates, centres, endpoints: ``morpho_locate``'s; frac_radius:
    the brush radius in up-sampled pixels (``morphomnist.perturb.fracture_radius``).  Returns (the new bitmaps, radius
    int32 [B], moment sums int64 [B, 6], status int32 [B])."""
    lib = _lib.load()
    B, Hh, wpr = _morpho_bits(bits, Wh, "morpho_local")
    if not (thickness.is_cuda and thickness.dtype == torch.float32 and tuple(thickness.shape) == (B,)
            and (B == 1 or thickness.stride(0) >= 1)):
        raise ValueError(f"morpho_local: thickness is an fp32 CUDA tensor [{B}]")
    if not 0 <= int(frac_radius) <= MORPHO_MAX_STAMP:
        raise ValueError(f"morpho_local: frac_radius in 0 .. {MORPHO_MAX_STAMP}")
    if not 1 <= int(num_frac) <= MORPHO_MAX_DRAWS:
        raise ValueError(f"morpho_local: num_frac in 1 .. {MORPHO_MAX_DRAWS}")
    if not (float(swell_strength) >= 1 and float(thin_amount) >= 0 and float(thick_amount) >= 0
            and float(swell_radius) >= 0):
        raise ValueError("morpho_local: swell_strength >= 1, and the amounts and swell_radius >= 0")
    dev = bits.device
    out = torch.empty_like(bits)
    radius = torch.empty(B, dtype=torch.int32, device=dev)
    sums = torch.empty(B, 6, dtype=torch.int64, device=dev)
    status_out = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.ali_morpho_local(c_void_p(bits.data_ptr()), _i32s(d2, (B, Hh, Wh), "d2"),
                                    None if d2c is None else _i32s(d2c, (B, Hh, Wh), "d2c"),
                                    c_void_p(thickness.data_ptr()), max(thickness.stride(0), 1),
                                    _i32(status, "status", B), _i32s(kind, (B,), "kind"),
                                    _i32(n_candidates, "n_candidates", B),
                                    _i32s(centres, (B, MORPHO_MAX_DRAWS, 2), "centres"),
                                    _i32s(endpoints, (B, MORPHO_MAX_DRAWS, 4), "endpoints"), float(thin_amount),
                                    float(thick_amount), float(swell_strength), float(swell_radius), int(frac_radius),
                                    int(num_frac), B, Hh, Wh, int(scale), _i32(out, "out"), _i32(radius, "radius"),
                                    c_void_p(sums.data_ptr()), _i32(status_out, "status_out"), _stream()),
               "ali_morpho_local")
    return out, radius, sums, status_out
