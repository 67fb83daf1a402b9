"""The launch plan of ali_conv_fwd / ali_conv_bwd_data (csrc/gconv.hip: plan_conv, include/ali_hip.h: ali_conv_plan) and
the four host queries that are views of it, against tests/golden/gconv_plans.json -- recorded from the launch code as
it was before its rules were gathered into one planner, with every launch replaced by a dump of its decisions.  Runs
without a GPU: the planner makes no HIP call and dereferences no operand.

The grid: every geometry of tests/test_gpu_conv_geometry.py and tests/test_gpu_conv_geometry_f16.py and every conv /
ConvT layer of the MorphoMNIST and audio-spectrogram E, G, D at the bench batch sizes (plus a few that only exist to
reach an error), both directions, in three precisions (f32, f16, f16 with twins).  At f32 and at f16 with twins each is
also planned with every epilogue kind, workspace size, as a ``gemm_batch`` job, and under every tuning set below -- one
factor at a time.  ``python tests/test_conv_plan_cpu.py FILE`` writes what the loaded library answers to FILE."""
import ctypes
import hashlib
import json
import os
import sys

import pytest

import test_gpu_conv_geometry as geo
import test_gpu_conv_geometry_f16 as geo16

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gconv_plans.json")
PTR = 0x1000          # operands of an epilogue are null-checked only

# (B, H, W, C, P, Q, K, R, S, stride, pad); a ConvTranspose2d is the Conv2d it is the data gradient of
LAYERS = {
    # MorphoMNIST, bs = 512; D runs its two passes back to back (1024 images, bn_groups = 2)
    "mnist-E1": (512, 28, 28, 8, 14, 14, 64, 3, 3, 2, 1), "mnist-E2": (512, 14, 14, 64, 7, 7, 128, 4, 4, 2, 1),
    "mnist-E3": (512, 7, 7, 128, 3, 3, 256, 4, 4, 2, 1), "mnist-E4": (512, 3, 3, 256, 1, 1, 512, 4, 4, 2, 1),
    "mnist-E5": (512, 1, 1, 512, 1, 1, 512, 1, 1, 2, 0),
    "mnist-G1": (512, 3, 3, 512, 1, 1, 800, 3, 3, 1, 0), "mnist-G2": (512, 7, 7, 256, 3, 3, 512, 3, 3, 2, 0),
    "mnist-G3": (512, 13, 13, 128, 7, 7, 256, 3, 3, 2, 1), "mnist-G4": (512, 25, 25, 64, 13, 13, 128, 3, 3, 2, 1),
    "mnist-G5": (512, 28, 28, 4, 25, 25, 64, 4, 4, 1, 0),
    "mnist-Dx1": (1024, 28, 28, 8, 24, 24, 32, 5, 5, 1, 0), "mnist-Dx2": (1024, 24, 24, 32, 11, 11, 64, 4, 4, 2, 0),
    "mnist-Dx3": (1024, 11, 11, 64, 8, 8, 128, 4, 4, 1, 0), "mnist-Dx4": (1024, 8, 8, 128, 3, 3, 256, 4, 4, 2, 0),
    "mnist-Dx5": (1024, 3, 3, 256, 1, 1, 512, 3, 3, 1, 0), "mnist-Dz": (1024, 1, 1, 512, 1, 1, 512, 1, 1, 1, 0),
    "mnist-Dxz": (1024, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
    # audio spectrograms (128 x 128), bs = 256, d = 64: E and D share their stack
    "audio-E1": (256, 128, 128, 8, 63, 63, 64, 5, 5, 2, 1), "audio-E2": (256, 63, 63, 64, 31, 31, 128, 5, 5, 2, 1),
    "audio-E3": (256, 31, 31, 128, 15, 15, 256, 5, 5, 2, 1), "audio-E4": (256, 15, 15, 256, 7, 7, 512, 5, 5, 2, 1),
    "audio-E5": (256, 7, 7, 512, 3, 3, 1024, 5, 5, 2, 1), "audio-E6": (256, 3, 3, 1024, 1, 1, 512, 5, 5, 2, 1),
    "audio-G0": (256, 4, 4, 1024, 1, 1, 576, 4, 4, 1, 0), "audio-G1": (256, 8, 8, 512, 4, 4, 1024, 5, 5, 2, 2),
    "audio-G2": (256, 16, 16, 256, 8, 8, 512, 5, 5, 2, 2), "audio-G3": (256, 32, 32, 128, 16, 16, 256, 5, 5, 2, 2),
    "audio-G4": (256, 64, 64, 64, 32, 32, 128, 5, 5, 2, 2), "audio-G5": (256, 128, 128, 4, 64, 64, 64, 5, 5, 2, 2),
    "audio-Dxz": (256, 1, 1, 1024, 1, 1, 1024, 1, 1, 1, 0),
    # the first conv of the 512 x 512 stacks (bs = 64); operands too large for 32-bit offsets; too many rows; bad geometry
    "esrf-E1": (64, 512, 512, 4, 255, 255, 64, 5, 5, 2, 1),
    "too-large": (2048, 64, 64, 32, 64, 64, 256, 1, 1, 1, 0), "too-many-rows": (4096, 64, 64, 32, 64, 64, 32, 1, 1, 1, 0),
    "bad-geometry": (4, 8, 8, 32, 8, 8, 32, 6, 1, 1, 0),
}

PRECISIONS = ("f32", "f16", "f16+twins")
EPILOGUES = ("none", "mask", "bn1", "bn1-slots=B", "bn1-slots=B+1", "bn1-groups2", "bn2", "bn2-no-x", "ld", "ld-short", "order", "order+1")
WORKSPACES = {"none": 0, "1MiB": 1 << 20, "256MiB": 256 << 20}
TUNINGS = [{}, {"ALI_SPLITK": 2}, {"ALI_BM": 128, "ALI_BN": 128}, {"ALI_BM": 256, "ALI_BN": 256}, {"ALI_TILE_M_SCALE": 8},
           {"ALI_NO_XCD": 1}, {"ALI_NO_ORDER": 1}, {"ALI_NO_UNIFORM": 1}, {"ALI_NO_DMA16": 1},
           {"ALI_BM": 128, "ALI_BN": 256}, {"ALI_BM": 256, "ALI_BN": 128}]        # (the last two: no kernel has that tile)


def _ops():
    from ali_hip import ops
    return ops


def geometries():
    ops = _ops()
    out = {}
    for c in geo.CASES + [c for c, _ in geo16.CASES]:
        g = c.geom(ops)
        out[c.id] = tuple(getattr(g, n) for n, _ in type(g)._fields_)
    out.update(LAYERS)
    return out


def grid():
    """[(tuning, geometry id, which, precision, epilogue, workspace, as_job)], grouped by tuning set"""
    cases = []
    for gid in geometries():
        for which in (0, 1):
            for prec in PRECISIONS:
                cases.append((0, gid, which, prec, "none", "256MiB", 0))
                if prec == "f16":
                    continue
                cases += [(0, gid, which, prec, ep, "256MiB", 0) for ep in EPILOGUES[1:]]
                cases += [(0, gid, which, prec, "none", ws, 0) for ws in ("none", "1MiB")]
                cases += [(0, gid, which, prec, "none", "256MiB", 1), (0, gid, which, prec, "order", "256MiB", 1)]
                cases += [(t, gid, which, prec, ep, "256MiB", 0) for t in range(1, len(TUNINGS)) for ep in ("none", "order")]
    return sorted(cases, key=lambda c: c[0])


def _epilogue(lib, g, which, prec, kind):
    from ali_hip._lib import AliEpilogue
    f16 = int(prec != "f32")
    ep = AliEpilogue(mfma_f16=f16)
    if prec == "f16+twins":
        ep.in16 = ep.w16 = ep.out16 = PTR
    cin, cout = (g.C, g.K) if which == 0 else (g.K, g.C)
    if kind == "mask":
        ep.mask, ep.mask_ld = PTR, cout
    elif kind.startswith("bn1"):
        ep.bn_part, ep.bn_mode, ep.bn_groups = PTR, 1, 2 if kind == "bn1-groups2" else 1
        ep.bn_slots = {"bn1-slots=B": g.B, "bn1-slots=B+1": g.B + 1}.get(kind, 0)
    elif kind.startswith("bn2"):
        ep.bn_part, ep.bn_mode, ep.bn_groups, ep.bn_mean, ep.bn_invstd = PTR, 2, 1, PTR, PTR
        ep.bn_x = PTR if kind == "bn2" else None
    elif kind == "ld":
        ep.in_ld, ep.out_ld = cin + 8, cout + 8
    elif kind == "ld-short":
        ep.in_ld = cin - 1
    elif kind.startswith("order"):       # a table as long as the query says the launch has M-tiles, or one longer
        n = lib.ali_conv_mtiles(ctypes.byref(g), which, f16, None, None)
        ep.tile_order, ep.tile_order_n = PTR, n + (1 if kind == "order+1" else 0)
    return ep


def _plan(lib, g, which, ep, ws_bytes, as_job):
    from ali_hip._lib import AliConvPlan
    p = AliConvPlan()
    rc = lib.ali_conv_plan(ctypes.byref(g), which, ctypes.byref(ep), ws_bytes, int(ws_bytes > 0), as_job, ctypes.byref(p))
    if rc != 0:
        return [rc, lib.ali_last_error().decode()]
    return [getattr(p, n) for n, _ in AliConvPlan._fields_]


def _queries(lib, g, which, f16):
    """[M-tiles, tile rows, pixel-major, order entries, digest of the order, uses_f16 (plain epilogue), writes_out16]"""
    from ali_hip._lib import AliEpilogue
    rows, pm = ctypes.c_int32(0), ctypes.c_int32(0)
    n = lib.ali_conv_mtiles(ctypes.byref(g), which, f16, ctypes.byref(rows), ctypes.byref(pm))
    buf = (ctypes.c_int32 * 65536)()
    no = lib.ali_conv_tile_order(ctypes.byref(g), which, f16, ctypes.cast(buf, ctypes.c_void_p), 65536)
    ep = AliEpilogue(mfma_f16=f16)
    return [n, rows.value, pm.value, no, hashlib.sha256(bytes(buf)[:4 * no]).hexdigest()[:16],
            lib.ali_conv_uses_f16(ctypes.byref(g), which, ctypes.byref(ep)), lib.ali_conv_writes_out16(ctypes.byref(g), which)]


def collect():
    """{"plans": {case key: plan fields or [rc, message]}, "queries": {key: _queries}} of the loaded library"""
    import ali_hip
    ops = _ops()
    lib = ali_hip.load()
    geoms = geometries()
    plans, queries = {}, {}
    try:
        current = None
        ctx = None
        for t, gid, which, prec, epk, wsk, job in grid():
            if t != current:
                if ctx is not None:
                    ctx.__exit__(None, None, None)
                ctx = ops.tuning(**TUNINGS[t])
                ctx.__enter__()
                current = t
            g = ops.geom(*geoms[gid])
            tname = ",".join(f"{k}={v}" for k, v in TUNINGS[t].items()) or "-"
            ep = _epilogue(lib, g, which, prec, epk)
            plans[f"{tname}|{gid}|{which}|{prec}|{epk}|{wsk}|{job}"] = _plan(lib, g, which, ep, WORKSPACES[wsk], job)
            f16 = int(prec != "f32")
            qk = f"{tname}|{gid}|{which}|{f16}"
            if qk not in queries:
                queries[qk] = _queries(lib, g, which, f16)
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return {"plans": plans, "queries": queries}


def pack(rec):
    """golden file layout: every distinct answer once, the cases (sorted by key) as indices into them"""
    out = {}
    for name, table in rec.items():
        keys = sorted(table)
        uniq = sorted({json.dumps(table[k]) for k in keys})
        index = {u: i for i, u in enumerate(uniq)}
        out[name] = {"keys_sha256": hashlib.sha256("\n".join(keys).encode()).hexdigest(),
                     "answers": [json.loads(u) for u in uniq], "cases": [index[json.dumps(table[k])] for k in keys]}
    return out


def unpack(packed, rec):
    """the golden answers keyed like ``rec`` (the grid of this module must be the grid the file was recorded on)"""
    out = {}
    for name, table in rec.items():
        keys, p = sorted(table), packed[name]
        assert hashlib.sha256("\n".join(keys).encode()).hexdigest() == p["keys_sha256"] and len(keys) == len(p["cases"]), \
            f"{name}: the grid of this module is not the one {GOLDEN} was recorded on"
        out[name] = {k: p["answers"][i] for k, i in zip(keys, p["cases"])}
    return out


@pytest.fixture(scope="module")
def answers():
    rec = collect()
    with open(GOLDEN) as f:
        return rec, unpack(json.load(f), rec)


def test_plans_are_the_recorded_ones(answers):
    from ali_hip._lib import AliConvPlan
    fields = [n for n, _ in AliConvPlan._fields_]
    got, want = answers[0]["plans"], answers[1]["plans"]
    bad = []
    for k in sorted(got):
        if got[k] != want[k]:
            if len(got[k]) == len(want[k]) == len(fields):
                bad.append((k, {f: (a, b) for f, a, b in zip(fields, got[k], want[k]) if a != b}))
            else:
                bad.append((k, got[k], want[k]))
    assert not bad, (len(bad), bad[:10])


def test_queries_are_the_recorded_ones(answers):
    got, want = answers[0]["queries"], answers[1]["queries"]
    bad = [(k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:10])


def test_golden_plans_cover_every_branch(answers):
    """on the golden file itself: no rule of the planner goes untested because the grid never reaches it"""
    from ali_hip._lib import AliConvPlan
    fields = [n for n, _ in AliConvPlan._fields_]
    want = answers[1]["plans"]
    geoms = geometries()
    ok = {k: dict(zip(fields, v)) for k, v in want.items() if len(v) == len(fields)}
    errors = {v[1] for v in want.values() if len(v) == 2}

    def some(pred):
        return any(pred(k.split("|"), p) for k, p in ok.items())
    gemm = lambda p: p["route"] == 0                                                          # noqa: E731
    dense = lambda k: k[2] == "0" and geoms[k[1]][10] == 0        # forward without padding: split-K by the cost search # noqa: E731
    assert some(lambda k, p: gemm(p) and p["splitk"] > 1 and k[0] == "-" and dense(k))
    assert some(lambda k, p: gemm(p) and p["splitk"] > 1 and k[0] == "-" and not dense(k))     # the plain rule
    assert some(lambda k, p: p["tail_split"] > 1)
    assert some(lambda k, p: p["ordered"] == 1)
    assert some(lambda k, p: p["xcd_chunk"] > 0)
    assert some(lambda k, p: p["uni"] == 1)
    for mode in (0, 1, 2, 3):
        assert some(lambda k, p: gemm(p) and p["mode"] == mode), mode
    for f16 in (1, 2, 3):
        assert some(lambda k, p: gemm(p) and p["f16"] == f16 and p["threads"] == (512 if f16 == 3 else 256)), f16
    assert some(lambda k, p: p["route"] == 1) and some(lambda k, p: p["route"] == 2)
    assert some(lambda k, p: p["job_variant"] == 0) and some(lambda k, p: p["job_variant"] == 1)
    # "nothing to launch" (no M-tile or an empty output) is kept from the launch code as it was, but no geometry that
    # passes the argument checks reaches it: every extent is positive.  The field is 0 throughout the file.
    assert not some(lambda k, p: p["empty"] != 0)
    for text in ("ali_conv_fwd: bad argument", "ali_conv_bwd_data: bad argument",
                 "ali_conv_fwd: bn_part was sized for", "ali_conv_fwd: epilogue not supported for this first-layer geometry",
                 "ali_conv_bwd_data: stride 3 unsupported", "gconv: more than 2^24 rows in one phase",
                 "gconv: bad fused BatchNorm epilogue", "gconv: bn_part was sized for", "gconv: bad in_ld / out_ld",
                 "gconv: tensor too large for 32-bit byte offsets", "gconv: no kernel for this tile"):
        assert any(e.startswith(text) for e in errors), text


def test_conv_plan_wrapper_follows_precision_and_workspace():
    """ops.conv_plan: a named tuple of the current precision and of the workspace ops allocates"""
    ops = _ops()
    ops.reload_tuning()
    g = ops.geom(*geometries()["tail"])
    p = ops.conv_plan(g, 0)
    assert (p.route, p.bm, p.bn, p.mode, p.f16, p.uni, p.tail_split, p.tail_u0, p.lin1d) == (0, 64, 64, 2, 0, 1, 2, 512, 1)
    assert p.grid_x == 512 + 2 * 88 and (p.grid_y, p.grid_z) == (1, 1)
    assert ops.conv_plan(g, 0, ws_bytes=0).tail_split == 1                   # no workspace: nothing is split
    assert ops.conv_plan(g, 0, as_job=True).job_variant == 0
    with ops.precision("f16"):
        p = ops.conv_plan(g, 0)
        assert (p.bm, p.bn, p.f16, p.ntile_m) == (128, 128, 1, 150) and p.splitk > 1
    with pytest.raises(RuntimeError, match="stride 3 unsupported"):
        ops.conv_plan(ops.geom(*geometries()["stride3"]), 1)


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(pack(collect()), f, separators=(",", ":"))
        f.write("\n")
