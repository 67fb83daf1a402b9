"""The route of every parity case of the routed kernel families, held to a record: tests/golden/routes_recorded.json
lists, for each case of tests/test_gpu_direct_routes.py (ali_tconv1_fwd / _dgrad / _wgrad), of
tests/test_gpu_scatter_routes.py (ali_tconv_scatter / ali_tconv_scatter_wgrad) and of tests/bn_cases.py (the
stand-alone BatchNorm passes, ali_colsum, ali_act_bwd; every row case with aligned and with misaligned operands), what
the launches' own queries -- ``ops.tconv1_route``, ``ops.tconv_scatter_plan`` and ``ops.ew_plan`` -- answered when it
was written: the route and, for the element-wise family, the two block counts, for the scatter family the LDS bytes
and the block count.  A change of the dispatch code that is meant to keep every route
runs against it; no GPU is needed.  ``python tests/test_routes_recorded_cpu.py`` rewrites the record from the queries
(after a deliberate change of a route, or with new cases)."""
import contextlib
import json
import os
import sys

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routes_recorded.json")
WS_BYTES = 256 << 20         # the workspace the launches of ``ops`` hand over by default


def _ops():
    from ali_hip import ops
    return ops


def cases():
    """(case id, family, shape, env): family and shape as a family-agnostic query would take them -- tconv1_<op>: B, P, Q,
    K, R, S, pad (wgrad: + nc, workspace bytes); tconv_scatter_<op>: the arguments of ``ops.tconv_scatter_plan`` after the
    op; the element-wise entries: rows per group, rows per image, C, ld, groups, aligned"""
    import bn_cases as bc
    import test_gpu_direct_routes as dr
    import test_gpu_scatter_routes as sr
    for c in dr.CASES:
        yield "direct:" + c.id, "tconv1_" + c.op, list(c.dims()) + ([c.nc, WS_BYTES] if c.op == "wgrad" else []), c.env
    for op, dims, nc in dr.REFUSED:
        yield (f"direct:refused-{op}-{'x'.join(map(str, dims))}", "tconv1_" + op,
               list(dims) + ([nc, WS_BYTES] if op == "wgrad" else []), {})
    for c in sr.FWD + sr.WGRAD:
        yield "scatter:" + c.id, "tconv_scatter_" + c.op, list(c.query()[1:]), {}
    for what, q, _ in sr.REFUSED:
        yield "scatter:refused-" + what, "tconv_scatter_" + q[0], list(q[1:]), {}
    for c in bc.ROW_CASES + bc.WIDE_CASES:
        for op in ("bn_stats", "bn_apply", "bn_bwd", "bn_bwd_from_partials"):
            g = c.groups if op in ("bn_stats", "bn_apply") else 1
            for aligned in (1, 0):
                yield (f"bn:{c.id}:{op}:{'aligned' if aligned else 'misaligned'}", op,
                       [c.B // g * c.rpi, c.rpi, c.C, c.C, g, aligned], {})
    for cid, rows, C, ld, aligned, _ in bc.COLSUM_CASES:
        yield "bn:" + cid, "colsum", [rows, 1, C, ld, 1, int(aligned)], {}
    for n in bc.ACT_N:
        yield f"bn:act-{n}", "act_bwd", [n, 1, 1, 1, 1, 0], {}


def query(ops, family, shape, env):
    """(route or None, [reduction blocks, element-wise blocks]) from the family's query under the tuning ``env``"""
    with (ops.tuning(**env) if env else contextlib.nullcontext()):
        if family.startswith("tconv1_"):
            nc, ws = shape[7:] or (1, None)
            return ops.tconv1_route(family[7:], *shape[:7], nc=nc, ws_bytes=ws), [0, 0]
        if family.startswith("tconv_scatter_"):
            got = ops.tconv_scatter_plan(family[14:], *shape)
            return (None, [0, 0]) if got is None else (got.name, [got.lds, got.blocks])
        rows, rpi, C, ld, groups, aligned = shape
        got = ops.ew_plan(family, rows, rpi, C, ld=ld, groups=groups, aligned=bool(aligned))
    return (None, [0, 0]) if got is None else (got[0], [got[1], got[2]])


def test_every_case_is_recorded_with_its_shape():
    with open(RECORD) as f:
        recorded = {r["case"]: r for r in json.load(f)}
    now = {cid: (family, shape, env) for cid, family, shape, env in cases()}
    assert set(now) == set(recorded), set(now) ^ set(recorded)
    for cid, (family, shape, env) in now.items():
        r = recorded[cid]
        assert (r["family"], r["shape"], r["env"]) == (family, shape, env), cid


def test_queries_answer_the_recorded_routes():
    ops = _ops()
    ops.reload_tuning()
    with open(RECORD) as f:
        records = json.load(f)
    assert len(records) > 200
    for r in records:
        route, plan = query(ops, r["family"], r["shape"], r["env"])
        assert (route, plan) == (r["route"], r["plan"]), (r["case"], route, plan)


def test_the_record_agrees_with_the_case_tables():
    """the route a case table names for a case is the recorded one (the direct and the scatter cases, the aligned row
    cases, colsum)"""
    import bn_cases as bc
    import test_gpu_direct_routes as dr
    import test_gpu_scatter_routes as sr
    with open(RECORD) as f:
        recorded = {r["case"]: r for r in json.load(f)}
    for c in dr.CASES:
        assert recorded["direct:" + c.id]["route"] == c.route, c.id
    for c in sr.FWD + sr.WGRAD:
        assert recorded["scatter:" + c.id]["route"] == c.plan, c.id
    for what, _, _ in sr.REFUSED:
        assert recorded["scatter:refused-" + what]["route"] is None, what
    for c in bc.ROW_CASES + bc.WIDE_CASES:
        for op in ("bn_apply", "bn_bwd_from_partials"):
            assert recorded[f"bn:{c.id}:{op}:aligned"]["route"] == c.route, (c.id, op)
            assert recorded[f"bn:{c.id}:{op}:misaligned"]["route"] == "scalar", (c.id, op)
    for case in bc.COLSUM_CASES:
        assert recorded["bn:" + case[0]]["route"] == case[5], case[0]


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "imagecfgen-pytorch_amd"), os.path.dirname(os.path.abspath(__file__))]
    ops = _ops()
    ops.reload_tuning()
    rows = []
    for cid, family, shape, env in cases():
        route, plan = query(ops, family, shape, env)
        rows.append({"case": cid, "family": family, "shape": shape, "env": env, "route": route, "plan": plan})
    with open(RECORD, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print(len(rows), "records ->", RECORD)
